"""CPU: what the streamed float layered engine offers and refuses without a device — acg_ldpc_decoder_create_layered_streamed,
StreamedLayeredBPDecoder, StreamedLayeredMinSumDecoder.  Every refusal below is made before a device is looked for, so it carries
its own message here and on a machine with a GPU alike.  Also here: the restatements of tests/layered_ref.py decode some frames
of the wide cases and fail others (with layered_ref.host_phi).  The kernel is held to them in tests/test_streamed_layered_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

import layered_q_cases as Q
import streamed_layered_cases as SL


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    return A


def _create(A, H, null=(), **params):
    """-> (return code, message); the handle, should one be made, is destroyed"""
    L = A.lib()
    p = A._lib.Params()
    L.acg_ldpc_params_default(C.byref(p))
    p.algo, p.schedule, p.max_iter = A._lib.ALGO_BP, A.SCHEDULE_LAYERED, 5
    for k, v in params.items():
        setattr(p, k, v)
    h = C.c_void_p()
    rc = L.acg_ldpc_decoder_create_layered_streamed(None if "code" in null else H._h, None if "params" in null else C.byref(p),
                                                    None if "out" in null else C.byref(h))
    msg = L.acg_ldpc_last_error().decode()
    if rc == 0:
        L.acg_ldpc_decoder_destroy(h)
    return rc, msg


def test_symbol_is_declared_and_bound(A):
    L = A.lib()
    name = "acg_ldpc_decoder_create_layered_streamed"
    assert name in A._lib.SYMBOLS and getattr(L, name).restype is C.c_int
    header = open(os.path.join(SL.ROOT, "include", "acg_ldpc.h")).read()
    assert re.search(r"\bint %s\(const acg_ldpc_code \*code, const acg_ldpc_params \*params, acg_ldpc_decoder \*\*out\);" % name, header)
    assert issubclass(A.StreamedLayeredBPDecoder, A.BeliefPropagationDecoder)
    assert issubclass(A.StreamedLayeredMinSumDecoder, A.MinSumDecoder)
    assert A.StreamedLayeredBPDecoder(5).name() == "BP" and A.StreamedLayeredMinSumDecoder(5, 0.75).name() == "MS"
    assert A.StreamedLayeredMinSumDecoder(5, 0.75).scale == 0.75
    for d in (A.StreamedLayeredBPDecoder(5), A.StreamedLayeredMinSumDecoder(5)):
        assert d.schedule == A.SCHEDULE_LAYERED and d.lanes_per_frame == 0


def test_null_arguments_are_refused(A):
    H = A.ParityCheckMatrix(Q.diag10())
    for what in ("code", "params", "out"):
        rc, msg = _create(A, H, null=(what,))
        assert rc != 0 and "null" in msg, (what, rc, msg)


@pytest.mark.parametrize("params,text", [
    (dict(algo="ALGO_QPADMM"), "algo must be ACG_LDPC_BP_SUMPRODUCT or ACG_LDPC_BP_MINSUM"),
    (dict(algo=77), "algo must be ACG_LDPC_BP_SUMPRODUCT or ACG_LDPC_BP_MINSUM"),
    (dict(schedule="SCHEDULE_FLOODING"), "schedule must be ACG_LDPC_SCHEDULE_LAYERED"),
    (dict(precision="PREC_F16"), "precision must be ACG_LDPC_PREC_DEFAULT"),
    (dict(precision="PREC_F64"), "precision must be ACG_LDPC_PREC_DEFAULT"),
    (dict(engine="ENGINE_FUSED"), "engine must be ACG_LDPC_ENGINE_AUTO or ACG_LDPC_ENGINE_STREAMED"),
    (dict(lanes_per_frame=256), "lanes_per_frame must be 0"),
    (dict(lanes_per_frame=1), "lanes_per_frame must be 0"),
    (dict(algo="ALGO_MINSUM", lanes_per_frame=64), "lanes_per_frame must be 0"),
    (dict(algo="ALGO_MINSUM", engine="ENGINE_FUSED"), "engine must be ACG_LDPC_ENGINE_AUTO or ACG_LDPC_ENGINE_STREAMED"),
    (dict(max_iter=-1), "max_iter must be >= 0"),
])
def test_host_only_refusals_carry_their_message(A, params, text):
    H = A.ParityCheckMatrix(Q.diag10())
    params = {k: (getattr(A, v) if hasattr(A, v) else getattr(A._lib, v)) if isinstance(v, str) else v for k, v in params.items()}
    rc, msg = _create(A, H, **params)
    assert rc != 0 and text in msg, (rc, msg)
    if "max_iter" not in params:
        assert msg.startswith("streamed layered BP: "), msg


@pytest.mark.parametrize("algo", ["ALGO_BP", "ALGO_MINSUM"])
@pytest.mark.parametrize("engine", ["ENGINE_AUTO", "ENGINE_STREAMED"])
def test_what_it_accepts_gets_as_far_as_the_device(A, algo, engine):
    """a check of 48 variables is not refused on the host: the call gets as far as looking for a device.  (The existing create
    call refuses the matrix once it has a device: tests/test_streamed_layered_gpu.py.)"""
    c = SL.wide(A, "deg48")
    rc, msg = _create(A, c.H, algo=getattr(A._lib, algo), engine=getattr(A, engine))
    assert rc == 0 or "no HIP device" in msg, (rc, msg)


@pytest.mark.parametrize("algo", SL.ALGOS)
@pytest.mark.parametrize("name", ["deg48", "deg40", "big"])
def test_restatement_decodes_some_frames_and_fails_others(A, name, algo):
    """layered_minsum(0.75) / layered_sumproduct_exact(host_phi) over layers_any() on the library's own frames"""
    c = SL.wide(A, name)
    bits, ok, iters = c.ref(algo)
    print("%s %s: %.1f dB, %d iterations, %d of %d frames decoded" % (name, algo, c.snr(algo), c.iters, int(ok.sum()), c.frames))
    assert 0 < ok.sum() < c.frames, int(ok.sum())
    assert not bits[ok == 0].any() and (iters[ok == 0] == c.iters).all() and (iters >= 1).all()
    if name == "big":
        assert 5.0 <= c.snr(algo) <= 5.6


def test_cxx_mirror_compiles_and_links(A, tmp_path):
    """acg_ldpc::StreamedLayeredBPDecoder / StreamedLayeredMinSumDecoder with plain g++ against the C-ABI library; the program
    decodes only where it finds a device (tests/test_streamed_layered_gpu.py)"""
    A.lib()
    exe = SL.build_cxx_check(tmp_path)
    out = subprocess.run([exe, os.path.join(SL.ROOT, "data", "H05.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "m=160 n=280 E=860 names=BP,MS" in out.stdout
    assert "fused: rc=1 streamed layered BP: engine must be ACG_LDPC_ENGINE_AUTO or ACG_LDPC_ENGINE_STREAMED" in out.stdout
