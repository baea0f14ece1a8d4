"""CPU: the C ABI of two-stage decoding (acg_ldpc_cascade_* in include/acg_ldpc.h): the struct layout of the Python mirror, and
the refusals that need no device — null arguments return non-zero with a message and do not crash."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data")


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    A.build()
    return A


def _err(A):
    return A.lib().acg_ldpc_last_error().decode()


def test_struct_layout_matches_the_header(A):
    from acg_alp_ldpc_amd import _lib
    # acg_ldpc_cascade_result: total, first (acg_ldpc_mc_result each), four int64, one double
    assert C.sizeof(_lib.CascadeResult) == 2 * C.sizeof(_lib.McResult) + 4 * 8 + 8 == 184
    assert _lib.CascadeResult.first.offset == C.sizeof(_lib.McResult)
    assert _lib.CascadeResult.second_frames.offset == 2 * C.sizeof(_lib.McResult)
    assert _lib.CascadeResult.second_kernel_ms.offset == 2 * C.sizeof(_lib.McResult) + 32
    hdr = open(os.path.join(ROOT, "include", "acg_ldpc.h")).read()
    body = hdr[hdr.index("typedef struct acg_ldpc_cascade_result {"):hdr.index("} acg_ldpc_cascade_result;")]
    order = [body.index(f) for f in ("acg_ldpc_mc_result total;", "acg_ldpc_mc_result first;", "int64_t second_frames;",
                                     "int64_t second_correct, second_pseudo, second_sum_iters;", "double  second_kernel_ms;")]
    assert order == sorted(order)


def test_every_cascade_symbol_is_bound(A):
    from acg_alp_ldpc_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("create", "destroy", "stage", "name", "describe", "decode_batch_dev", "decode_batch", "decode_batch_f32",
                 "last_call", "mc_run", "merge"):
        assert hasattr(raw, "acg_ldpc_cascade_" + name) and "acg_ldpc_cascade_" + name in _lib.SYMBOLS


def test_null_arguments_are_refused_with_a_message(A):
    from acg_alp_ldpc_amd import _lib
    L = A.lib()
    H = A.read_pcm(os.path.join(DATA, "H05.txt"))
    p = _lib.Params()
    L.acg_ldpc_params_default(C.byref(p))
    out = C.c_void_p()
    for args in ((None, C.byref(p), None, C.byref(p), None, C.byref(out)),
                 (H._h, None, None, C.byref(p), None, C.byref(out)),
                 (H._h, C.byref(p), None, None, None, C.byref(out)),
                 (H._h, C.byref(p), None, C.byref(p), None, None)):
        assert L.acg_ldpc_cascade_create(*args) != 0 and "null argument" in _err(A)
        assert not out.value
    # every call on a null cascade: non-zero and a message (destroy, name and describe: harmless)
    buf = (C.c_uint8 * 64)()
    assert L.acg_ldpc_cascade_decode_batch_dev(None, buf, 0, 1, 0.0, buf, buf, None, None, None) != 0 and "null cascade" in _err(A)
    assert L.acg_ldpc_cascade_decode_batch(None, buf, 1, 0.0, buf, buf, None, None) != 0 and "null cascade" in _err(A)
    assert L.acg_ldpc_cascade_decode_batch_f32(None, buf, 1, 0.0, buf, buf, None, None) != 0 and "null cascade" in _err(A)
    assert L.acg_ldpc_cascade_last_call(None, None, None, None) != 0 and "null cascade" in _err(A)
    assert not L.acg_ldpc_cascade_stage(None, 0) and "null cascade" in _err(A)
    cfg, res = _lib.McCfg(), _lib.CascadeResult()
    assert L.acg_ldpc_cascade_mc_run(None, C.byref(cfg), C.byref(res)) != 0 and "null argument" in _err(A)
    L.acg_ldpc_cascade_destroy(None)
    assert L.acg_ldpc_cascade_name(None) == b""
    assert L.acg_ldpc_cascade_describe(None, None, 0) == 0


def test_create_reports_which_stage_refused(A):
    """a refusal of one of the two create calls carries its message behind "first: " / "second: " — here refusals that are
    made before a device is looked for, so they read the same with and without a GPU"""
    from acg_alp_ldpc_amd import _lib
    L = A.lib()
    H = A.read_pcm(os.path.join(DATA, "H05.txt"))
    good, bad = _lib.Params(), _lib.Params()
    L.acg_ldpc_params_default(C.byref(good))
    L.acg_ldpc_params_default(C.byref(bad))
    bad.max_iter = -1
    out = C.c_void_p()
    if A.device_available():
        assert L.acg_ldpc_cascade_create(H._h, C.byref(good), None, C.byref(bad), None, C.byref(out)) != 0
        assert _err(A) == "second: max_iter must be >= 0" and not out.value
    assert L.acg_ldpc_cascade_create(H._h, C.byref(bad), None, C.byref(good), None, C.byref(out)) != 0
    assert _err(A) == "first: max_iter must be >= 0" and not out.value
    q = _lib.Quant()
    L.acg_ldpc_quant_default(C.byref(q))
    q.msg_bits = 99
    assert L.acg_ldpc_cascade_create(H._h, C.byref(good), C.byref(q), C.byref(good), None, C.byref(out)) != 0
    assert _err(A).startswith("first: ") and "msg_bits" in _err(A) and not out.value
    # two devices
    other = _lib.Params()
    L.acg_ldpc_params_default(C.byref(other))
    good.device, other.device = 0, 1
    assert L.acg_ldpc_cascade_create(H._h, C.byref(good), None, C.byref(other), None, C.byref(out)) != 0
    assert "different devices (0 and 1)" in _err(A) and not out.value


def test_merge_adds_everything(A):
    from acg_alp_ldpc_amd import _lib
    a, b = _lib.CascadeResult(), _lib.CascadeResult()
    for k, r in enumerate((a, b), 1):
        for f, _ in _lib.McResult._fields_:
            setattr(r.total, f, 10 * k)
            setattr(r.first, f, 100 * k)
        r.second_frames, r.second_correct, r.second_pseudo, r.second_sum_iters, r.second_kernel_ms = k, 2 * k, 3 * k, 4 * k, 0.5 * k
    A.lib().acg_ldpc_cascade_merge(C.byref(a), C.byref(b))
    assert all(getattr(a.total, f) == 30 and getattr(a.first, f) == 300 for f, _ in _lib.McResult._fields_)
    assert (a.second_frames, a.second_correct, a.second_pseudo, a.second_sum_iters, a.second_kernel_ms) == (3, 6, 9, 12, 1.5)
