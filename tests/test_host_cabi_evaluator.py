"""CPU: the evaluator entry points of the C ABI (acg_ldpc_mc_run_codes) exist and check their arguments; without a device
an evaluator cannot be created."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    A.build()
    return A


def qpadmm_params(A):
    from acg_alp_ldpc_amd import _lib
    p = _lib.Params()
    A.lib().acg_ldpc_params_default(C.byref(p))
    p.algo = _lib.ALGO_QPADMM
    return p


def test_symbols_exist(A):
    from acg_alp_ldpc_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("acg_ldpc_evaluator_create", "acg_ldpc_evaluator_destroy", "acg_ldpc_mc_run_codes", "acg_ldpc_evaluator_describe"):
        assert hasattr(raw, name) and name in _lib.SYMBOLS
    assert callable(A.run_experiment_codes) and callable(A.CodesEvaluator)


def test_create_without_a_device_fails_with_a_message(A):
    p = qpadmm_params(A)
    if A.device_available():  # (the GPU box: the same call succeeds)
        ev = A.CodesEvaluator(p)
        assert "mc_codes=none" in ev.describe()
        ev.close()
        return
    h = C.c_void_p()
    assert A.lib().acg_ldpc_evaluator_create(C.byref(p), C.byref(h)) != 0
    assert b"no HIP device" in A.lib().acg_ldpc_last_error()
    assert not h.value
    with pytest.raises(A.LdpcError, match="no HIP device"):
        A.CodesEvaluator(p)


def test_argument_checks(A):
    from acg_alp_ldpc_amd import _lib
    L = A.lib()
    h = C.c_void_p()
    assert L.acg_ldpc_evaluator_create(None, C.byref(h)) != 0 and b"null" in L.acg_ldpc_last_error()
    p = qpadmm_params(A)
    assert L.acg_ldpc_evaluator_create(C.byref(p), None) != 0 and b"null" in L.acg_ldpc_last_error()
    p.algo = _lib.ALGO_BP
    assert L.acg_ldpc_evaluator_create(C.byref(p), C.byref(h)) != 0 and b"QP-ADMM" in L.acg_ldpc_last_error()
    cfg, res = _lib.McCfg(), _lib.McResult()
    codes = (C.c_void_p * 1)()
    assert L.acg_ldpc_mc_run_codes(None, codes, 1, C.byref(cfg), C.byref(res)) != 0 and b"null" in L.acg_ldpc_last_error()
    assert L.acg_ldpc_mc_run_codes(None, codes, 0, C.byref(cfg), C.byref(res)) != 0 and b"n_codes" in L.acg_ldpc_last_error()
    L.acg_ldpc_evaluator_destroy(None)  # a no-op
    assert L.acg_ldpc_evaluator_describe(None, None, 0) == 0
    if A.device_available():
        ev = A.CodesEvaluator(qpadmm_params(A))
        assert L.acg_ldpc_mc_run_codes(ev._h, codes, 0, C.byref(cfg), C.byref(res)) != 0 and b"n_codes" in L.acg_ldpc_last_error()
        assert L.acg_ldpc_mc_run_codes(ev._h, None, 1, C.byref(cfg), C.byref(res)) != 0 and b"null" in L.acg_ldpc_last_error()
        assert L.acg_ldpc_mc_run_codes(ev._h, codes, 1, C.byref(cfg), C.byref(res)) != 0 and b"null" in L.acg_ldpc_last_error()
        ev.close()
