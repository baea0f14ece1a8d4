"""CPU: what the streamed fixed-point layered min-sum engine offers and refuses without a device —
acg_ldpc_decoder_create_quantized_streamed, acg_ldpc_debug_layers_any, StreamedQuantizedMinSumDecoder,
ParityCheckMatrix.layers_any().  Every refusal below is made before a device is looked for, so it carries its own message
here and on a machine with a GPU alike.  The kernel is held to its restatement in tests/test_streamed_q_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import layered_q_cases as Q
import streamed_q_cases as S


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    return A


def _create(A, H, quant=Q.QUANTS["default"], null=(), **params):
    """-> (return code, message); the handle, should one be made, is destroyed"""
    L = A.lib()
    p = A._lib.Params()
    L.acg_ldpc_params_default(C.byref(p))
    p.algo, p.schedule, p.max_iter = A._lib.ALGO_MINSUM, A.SCHEDULE_LAYERED, 5
    for k, v in params.items():
        setattr(p, k, v)
    q = A._lib.Quant(*quant)
    h = C.c_void_p()
    rc = L.acg_ldpc_decoder_create_quantized_streamed(None if "code" in null else H._h, None if "params" in null else C.byref(p),
                                                      None if "quant" in null else C.byref(q), None if "out" in null else C.byref(h))
    msg = L.acg_ldpc_last_error().decode()
    if rc == 0:
        L.acg_ldpc_decoder_destroy(h)
    return rc, msg


def test_symbols_are_bound(A):
    L = A.lib()
    for name in ("acg_ldpc_decoder_create_quantized_streamed", "acg_ldpc_debug_layers_any"):
        assert name in A._lib.SYMBOLS and getattr(L, name).restype is C.c_int
    assert issubclass(A.StreamedQuantizedMinSumDecoder, A.QuantizedMinSumDecoder)
    assert A.StreamedQuantizedMinSumDecoder(5).name() == "QMS"


def test_null_arguments_are_refused(A):
    H = A.ParityCheckMatrix(Q.diag10())
    for what in ("code", "params", "quant", "out"):
        rc, msg = _create(A, H, null=(what,))
        assert rc != 0 and "null" in msg, (what, rc, msg)
    nl = C.c_int32()
    assert A.lib().acg_ldpc_debug_layers_any(None, C.byref(nl), None, None, None, 0) != 0
    assert "null argument" in A.lib().acg_ldpc_last_error().decode()


@pytest.mark.parametrize("params,quant,text", [
    (dict(algo=0), None, "algo must be ACG_LDPC_BP_MINSUM"),
    (dict(schedule=0), None, "schedule must be ACG_LDPC_SCHEDULE_LAYERED"),
    (dict(precision="PREC_F16"), None, "precision must be ACG_LDPC_PREC_DEFAULT"),
    (dict(precision="PREC_F64"), None, "precision must be ACG_LDPC_PREC_DEFAULT"),
    (dict(engine="ENGINE_FUSED"), None, "engine must be ACG_LDPC_ENGINE_AUTO or ACG_LDPC_ENGINE_STREAMED"),
    (dict(lanes_per_frame=64), None, "lanes_per_frame must be 0"),
    (dict(lanes_per_frame=1), None, "lanes_per_frame must be 0"),
    (dict(max_iter=-1), None, "max_iter must be >= 0"),
    (dict(), (0.0, 6, 6, 8, 1, 0, 1), "llr_step must be finite and > 0"),
    (dict(), (0.5, 6, 9, 16, 1, 0, 1), "msg_bits must be 2 ... 8"),
    (dict(), (0.5, 6, 6, 17, 1, 0, 1), "post_bits must be 2 ... 16"),
    (dict(), (0.5, 9, 6, 8, 1, 0, 1), "ch_bits must be 2 ... post_bits"),
    (dict(), (0.5, 6, 6, 8, 3, 1, 0), "scale_num must be 1 ... 2^scale_shift"),
    (dict(), (0.5, 6, 6, 8, 1, 0, 32), "offset must be 0 ... 2^(msg_bits-1) - 1"),
])
def test_host_only_refusals_carry_their_message(A, params, quant, text):
    H = A.ParityCheckMatrix(Q.diag10())
    params = {k: getattr(A, v) if isinstance(v, str) else v for k, v in params.items()}
    rc, msg = _create(A, H, quant or Q.QUANTS["default"], **params)
    assert rc != 0 and text in msg, (rc, msg)
    if quant is None and "max_iter" not in params:
        assert msg.startswith("streamed quantized layered min-sum: "), msg


def test_degree_and_size_are_not_refused_on_the_host(A):
    """a check of 48 variables: the existing create call refuses it on the host, the new one gets as far as looking for a device"""
    w = S.wide(A, "deg48")
    L = A.lib()
    p = A._lib.Params()
    L.acg_ldpc_params_default(C.byref(p))
    p.algo, p.schedule, p.max_iter = A._lib.ALGO_MINSUM, A.SCHEDULE_LAYERED, 5
    q = A._lib.Quant(*Q.QUANTS["default"])
    h = C.c_void_p()
    assert L.acg_ldpc_decoder_create_quantized(w.H._h, C.byref(p), C.byref(q), C.byref(h)) != 0
    assert "check degree above 32" in L.acg_ldpc_last_error().decode()
    rc, msg = _create(A, w.H)
    assert rc == 0 or "no HIP device" in msg, (rc, msg)


@pytest.mark.parametrize("name", sorted(Q.CASES))
def test_layers_any_is_layers_wide_where_that_accepts(A, name):
    c = Q.case(A, name)
    Z, layers = c.H.layers_any()
    assert Z == c.Z and layers.dtype == c.layers.dtype and np.array_equal(layers, c.layers)


@pytest.mark.parametrize("name", ["deg48", "deg40"])
def test_layers_any_on_wide_checks(A, name):
    """sets of one degree whose checks share no variable, every check in exactly one of them; layers_wide refuses the matrix"""
    w = S.wide(A, name)
    with pytest.raises(A.LdpcError, match="check degree above 32"):
        w.H.layers_wide()
    assert w.Z == 0 and w.layers.ndim == 2
    seen = []
    for layer in w.layers:
        ids = layer[layer >= 0]
        assert len(ids) and (layer[:len(ids)] >= 0).all()              # occupied slots first
        assert len({len(w.edges[k]) for k in ids}) == 1
        v = np.concatenate([w.edges[k] for k in ids])
        assert len(np.unique(v)) == len(v)
        seen.extend(int(k) for k in ids)
    assert sorted(seen) == list(range(w.m))
    # first fit in row order: a check sits in the first set of its degree with which it shares no variable
    first = w.layers[:, 0]
    assert (np.diff(first) > 0).all()


def test_cxx_mirror_compiles_and_links(A, tmp_path):
    """acg_ldpc::StreamedQuantizedMinSumDecoder with plain g++ against the C-ABI library; the program decodes only where it finds a
    device (tests/test_streamed_q_gpu.py)"""
    import os
    import subprocess
    A.lib()
    exe = S.build_cxx_check(tmp_path)
    out = subprocess.run([exe, os.path.join(Q.ROOT, "data", "H05.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "m=160 n=280 E=860 name=QMS" in out.stdout
    assert "fused: rc=1 streamed quantized layered min-sum: engine must be ACG_LDPC_ENGINE_AUTO or ACG_LDPC_ENGINE_STREAMED" in out.stdout
