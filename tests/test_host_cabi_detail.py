"""CPU: the C ABI of the detail run (acg_ldpc_mc_run_detail, acg_ldpc_mc_detail_merge in include/acg_ldpc.h): symbols,
struct layouts, the argument errors (all refused before anything touches a device) and the shard merge."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import acg_alp_ldpc_amd as A
    A.build()
    return A.lib()


def test_symbols_and_struct_layouts(L):
    from acg_alp_ldpc_amd import _lib
    from acg_alp_ldpc_amd.experiment import EVENT_DTYPE
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("acg_ldpc_mc_run_detail", "acg_ldpc_mc_detail_merge"):
        assert hasattr(raw, name) and name in _lib.SYMBOLS
    assert C.sizeof(_lib.McEvent) == 32 and EVENT_DTYPE.itemsize == 32
    assert [(f, EVENT_DTYPE.fields[f][1]) for f in EVENT_DTYPE.names] == [(f, getattr(_lib.McEvent, f).offset) for f, _ in _lib.McEvent._fields_]
    assert C.sizeof(_lib.McDetail) == 72 + 7 * 8 + 2 * 4
    assert _lib.McDetail.base.offset == 0 and _lib.McDetail.word_frames.offset == 72 and _lib.McDetail.min_pseudo_weight.offset == 128
    hdr = open(os.path.join(ROOT, "include", "acg_ldpc.h")).read()
    # the header's event struct: 1 x int64 + 6 x int32, the enum values the mirrors use, and the citation it extends
    body = re.search(r"typedef struct acg_ldpc_mc_event \{(.*?)\} acg_ldpc_mc_event;", hdr, flags=re.S).group(1)
    assert len(re.findall(r"\bint64_t\b", body)) == 1 and len(re.findall(r"\bint32_t\b", body)) == 6
    for name, val in (("PSEUDO", _lib.EVENT_PSEUDO), ("NO_WORD", _lib.EVENT_NO_WORD), ("NONCODEWORD", _lib.EVENT_NONCODEWORD)):
        assert re.search(r"ACG_LDPC_EVENT_%s = %d\b" % (name, val), hdr)
    assert "experiment.h:109-120" in hdr


def test_argument_errors_need_no_device(L):
    from acg_alp_ldpc_amd import _lib
    cfg, out = _lib.McCfg(), _lib.McDetail()
    cfg.frames, cfg.snr = 10, 1.0
    ev = (_lib.McEvent * 4)()
    fake = C.create_string_buffer(64)     # stands for a decoder: every case below must be refused before it is looked at
    dec = C.cast(fake, C.c_void_p)

    def refused(*args):
        rc = L.acg_ldpc_mc_run_detail(*args)
        msg = L.acg_ldpc_last_error().decode()
        assert rc != 0 and msg, (rc, msg)
        return msg
    assert "null" in refused(None, C.byref(cfg), C.byref(out), ev, None, 4)
    assert "null" in refused(dec, None, C.byref(out), ev, None, 4)
    assert "null" in refused(dec, C.byref(cfg), None, ev, None, 4)
    assert "cap" in refused(dec, C.byref(cfg), C.byref(out), ev, None, -1)
    assert "events" in refused(dec, C.byref(cfg), C.byref(out), None, None, 4)
    cfg.frames = -1
    assert "cfg" in refused(dec, C.byref(cfg), C.byref(out), ev, None, 4)
    cfg.frames = 10
    cw = (C.c_uint8 * 8)()
    cfg.codewords, cfg.n_codewords = C.addressof(cw), 0
    assert "cfg" in refused(dec, C.byref(cfg), C.byref(out), None, None, 0)
    assert fake.raw == b"\0" * 64


def detail(**kw):
    from acg_alp_ldpc_amd import _lib
    d = _lib.McDetail()
    d.min_pseudo_weight = d.min_pseudo_frame = -1
    for k, v in kw.items():
        if k in ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong", "sum_iters", "time_sec", "kernel_ms"):
            setattr(d.base, k, v)
        else:
            setattr(d, k, v)
    return d


def test_detail_merge(L):
    a = detail(correct=5, pseudo=1, total=8, sum_hamming=80, sum_hamming_ok=40, sum_hamming_wrong=40, sum_iters=99, time_sec=1.0,
               kernel_ms=2.0, word_frames=6, bit_errors=17, noncodeword_frames=0, sum_syndrome_weight=0, n_events=3, n_stored=2,
               min_pseudo_weight=17, min_pseudo_frame=7)
    b = detail(correct=1, pseudo=2, total=4, sum_hamming=30, sum_hamming_ok=10, sum_hamming_wrong=20, sum_iters=11, time_sec=0.5,
               kernel_ms=1.0, word_frames=4, bit_errors=40, noncodeword_frames=1, sum_syndrome_weight=6, n_events=3, n_stored=3,
               min_pseudo_weight=12, min_pseudo_frame=1003)
    L.acg_ldpc_mc_detail_merge(C.byref(a), C.byref(b))
    assert (a.base.correct, a.base.pseudo, a.base.total, a.base.sum_hamming, a.base.sum_hamming_ok, a.base.sum_hamming_wrong,
            a.base.sum_iters) == (6, 3, 12, 110, 50, 60, 110)
    assert (a.base.time_sec, a.base.kernel_ms) == (1.5, 3.0)
    assert (a.word_frames, a.bit_errors, a.noncodeword_frames, a.sum_syndrome_weight, a.n_events) == (10, 57, 1, 6, 6)
    assert a.n_stored == 2                                    # the caller owns the event buffers
    assert (a.min_pseudo_weight, a.min_pseudo_frame) == (12, 1003)   # the smaller weight


def test_detail_merge_min_pseudo_rules(L):
    def merged(wa, fa, wb, fb):
        a, b = detail(min_pseudo_weight=wa, min_pseudo_frame=fa), detail(min_pseudo_weight=wb, min_pseudo_frame=fb)
        L.acg_ldpc_mc_detail_merge(C.byref(a), C.byref(b))
        return a.min_pseudo_weight, a.min_pseudo_frame
    assert merged(-1, -1, -1, -1) == (-1, -1)
    assert merged(-1, -1, 9, 50) == (9, 50)                  # -1 is "none", not a small weight
    assert merged(9, 50, -1, -1) == (9, 50)
    assert merged(9, 50, 9, 20) == (9, 20)                   # tie: the lower frame
    assert merged(9, 20, 9, 50) == (9, 20)
    assert merged(9, 20, 10, 1) == (9, 20)
    assert merged(14, (1 << 33) + 9, 14, (1 << 33) + 2) == (14, (1 << 33) + 2)
    # an accumulator the caller zeroed holds no pseudo frame either
    from acg_alp_ldpc_amd import _lib
    z, b = _lib.McDetail(), detail(min_pseudo_weight=9, min_pseudo_frame=50, total=3)
    L.acg_ldpc_mc_detail_merge(C.byref(z), C.byref(b))
    assert (z.min_pseudo_weight, z.min_pseudo_frame, z.base.total) == (9, 50, 3)
    z = _lib.McDetail()
    L.acg_ldpc_mc_detail_merge(C.byref(z), C.byref(detail()))
    assert (z.min_pseudo_weight, z.min_pseudo_frame) == (-1, -1)
