"""CPU: the C ABI of ordered-statistics decoding (include/acg_ldpc.h, "OSD"): the new symbols are bound, null and negative
arguments are refused with a message and without a crash, and every rule acg_ldpc_decoder_create states for algo = ACG_LDPC_OSD
is checked on the host, before a device is looked for.  (The refusal of a handle that is not OSD needs a handle, hence a device:
tests/test_osd_gpu.py.)"""
import ctypes as C
import os

import numpy as np
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


def test_symbols_and_enum(A):
    from acg_alp_ldpc_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("acg_ldpc_osd_decode_batch_dev", "acg_ldpc_osd_decode_batch", "acg_ldpc_debug_osd_soft"):
        assert hasattr(raw, name) and name in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "acg_ldpc.h")).read()
    assert "ACG_LDPC_OSD = 3" in hdr and _lib.ALGO_OSD == 3
    assert A.OSDDecoder(1).name() == "OSD" and A.OSDDecoder()._params().max_iter == 1 and A.OSDDecoder(0)._params().algo == 3


def test_null_and_negative_arguments_are_refused(A):
    L = A.lib()
    buf = (C.c_uint8 * 64)()
    assert L.acg_ldpc_osd_decode_batch_dev(None, buf, 1, buf, buf, None, None) != 0 and "null decoder" in _err(A)
    assert L.acg_ldpc_osd_decode_batch_dev(None, None, 0, None, None, None, None) != 0 and "null decoder" in _err(A)
    assert L.acg_ldpc_osd_decode_batch(None, buf, 1, buf, buf, None) != 0 and "null decoder" in _err(A)
    assert L.acg_ldpc_osd_decode_batch(None, buf, -1, buf, buf, None) != 0
    out = np.zeros(4, np.int16)
    y = np.zeros(4)
    assert L.acg_ldpc_debug_osd_soft(None, 1, 4, out.ctypes.data) != 0 and "bad argument" in _err(A)
    assert L.acg_ldpc_debug_osd_soft(y.ctypes.data, 1, 4, None) != 0 and "bad argument" in _err(A)
    assert L.acg_ldpc_debug_osd_soft(y.ctypes.data, 1, -1, out.ctypes.data) != 0 and "bad argument" in _err(A)
    assert L.acg_ldpc_debug_osd_soft(y.ctypes.data, 1, 0, out.ctypes.data) == 0


def test_create_checks_the_rules_on_the_host(A):
    from acg_alp_ldpc_amd import _lib
    L = A.lib()
    H = A.read_pcm(os.path.join(DATA, "H05.txt"))

    def create(code=H, **kw):
        p = _lib.Params()
        L.acg_ldpc_params_default(C.byref(p))
        p.algo, p.max_iter = _lib.ALGO_OSD, 1
        for k, v in kw.items():
            setattr(p, k, v)
        out = C.c_void_p()
        rc = L.acg_ldpc_decoder_create(code._h, C.byref(p), C.byref(out))
        if rc == 0:
            L.acg_ldpc_decoder_destroy(out)
        else:
            assert not out.value
        return rc, _err(A)
    for kw, text in ((dict(max_iter=2), "OSD: max_iter is the order and must be 0 or 1"),
                     (dict(max_iter=50), "OSD: max_iter is the order"),
                     (dict(precision=_lib.PREC_F32), "OSD: precision must be ACG_LDPC_PREC_DEFAULT"),
                     (dict(precision=_lib.PREC_F16), "OSD: precision must be"),
                     (dict(engine=_lib.ENGINE_STREAMED), "OSD: engine must be ACG_LDPC_ENGINE_AUTO or ACG_LDPC_ENGINE_FUSED"),
                     (dict(schedule=_lib.SCHEDULE_LAYERED), "OSD: schedule must be ACG_LDPC_SCHEDULE_FLOODING"),
                     (dict(lanes_per_frame=512), "OSD: lanes_per_frame must be 0, 64, 128 or 256"),
                     (dict(lanes_per_frame=32), "OSD: lanes_per_frame must be")):
        rc, msg = create(**kw)
        assert rc == 3 and text in msg, (kw, rc, msg)
    assert create(max_iter=-1)[0] != 0
    wide = np.zeros((1, 65536), dtype=np.uint8)
    wide[0, :3] = 1
    rc, msg = create(A.ParityCheckMatrix(wide))
    assert rc == 3 and "OSD: n must be <= 65535" in msg
    big = np.zeros((600, 3000), dtype=np.uint8)          # the shape of qc2x10z300: 3000 columns of 19 words
    big[np.arange(600), np.arange(600)] = 1
    rc, msg = create(A.ParityCheckMatrix(big))
    assert rc == 3 and "OSD: a frame" in msg and "does not fit in LDS" in msg
    # what passes the rules reaches the device: a handle where there is one, "no HIP device" where there is none
    for kw in (dict(), dict(max_iter=0), dict(lanes_per_frame=64), dict(engine=_lib.ENGINE_FUSED), dict(early_exit=0, alpha=3.0, ms_scale=0.5)):
        rc, msg = create(**kw)
        assert rc == 0 or (rc == 20 and "no HIP device" in msg), (kw, rc, msg)
