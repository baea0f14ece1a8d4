"""CPU: the LLR entrance of the streamed float layered engine (acg_ldpc_decode_batch_llr, _llr_dev;
StreamedLayeredBPDecoder / StreamedLayeredMinSumDecoder.decode_llr_batch) — its restatement tests/streamed_layered_io_ref.py tied
to the pinned restatements of tests/layered_ref.py, the sign rule of the posteriors, the frames of the GPU tests (some decode,
some fail, in every form), and what the library and the Python wrapper refuse without a device.  The kernel is held to the
restatement, value for value, in tests/test_streamed_layered_io_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import layered_ref
import streamed_layered_cases as SL
import streamed_layered_io_cases as IO
from layered_ref import channel_llr_f32, host_phi, layered_minsum, layered_sumproduct_exact
from streamed_layered_io_ref import LLR_CLAMP, LN2_F32, decode_llr, prepare_llr


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    return A


@pytest.mark.parametrize("algo", SL.ALGOS)
def test_restatement_on_the_symbol_entrances_llrs_is_the_pinned_restatement(A, algo):
    """deg48: fed channel_llr_f32(y, snr, True) the restatement returns word, flag and iteration of layered_minsum /
    layered_sumproduct_exact(..., symbols_f32=True) on y, and their posteriors (sum-product: times (float) ln 2)"""
    c = SL.wide(A, "deg48")
    y = c.y(algo).astype(np.float32)
    L = channel_llr_f32(y, c.snr(algo), True)
    assert L.dtype == np.float32 and np.abs(L).max() < LLR_CLAMP and (prepare_llr(L).view(np.uint32) == L.view(np.uint32)).all()
    post = []
    if algo == "minsum":
        want = layered_minsum(c.Hm, c.layers, y, c.snr(algo), c.iters, SL.MS_SCALE, symbols_f32=True, posteriors=post)
    else:
        want = layered_sumproduct_exact(c.Hm, c.layers, y, c.snr(algo), c.iters, host_phi, symbols_f32=True, posteriors=post)
    got = decode_llr(c.Hm, c.layers, L, c.iters, algo, SL.MS_SCALE, host_phi)
    for g, w in zip(got[:3], want):
        assert (g == w).all()
    wp = post[0] if algo == "minsum" else post[0] * LN2_F32
    assert got[3].dtype == np.float32 and (got[3].view(np.uint32) == wp.view(np.uint32)).all()
    assert 0 < want[1].sum() < c.frames
    # and the substitution of the channel step is undone: the pinned restatements form their own LLRs again
    assert layered_ref.channel_llr_f32 is channel_llr_f32


def test_prepare_llr():
    """NaN -> +0 whatever its sign, +-inf and +-3e38 -> +-2^20, +-0 and everything within +-2^20 as they are, bit for bit"""
    x = np.array([np.nan, -np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, -0.0, 1048576.0, -1048576.0, 1048576.125, 1e-45, -7.25], dtype=np.float32)
    want = np.array([0.0, 0.0, 1048576.0, -1048576.0, 1048576.0, -1048576.0, 0.0, -0.0, 1048576.0, -1048576.0, 1048576.0, 1e-45, -7.25], dtype=np.float32)
    got = prepare_llr(x)
    assert got.dtype == np.float32 and (got.view(np.uint32) == want.view(np.uint32)).all()
    assert np.isnan(x[:2]).all() and float(LLR_CLAMP) == 2.0 ** 20            # (the input is not touched)
    assert (prepare_llr(np.array([[3, -4]], dtype=np.int64)) == np.array([[3.0, -4.0]], dtype=np.float32)).all()


# (case, form, algorithm) of every GPU test
USED = [(name, "plain", algo) for name in ("deg48", "deg40", "H05") for algo in SL.ALGOS] + \
       [("deg40", form, algo) for form in ("special", "punctured") for algo in SL.ALGOS] + [("big", "plain", "minsum")]


@pytest.mark.parametrize("name,form,algo", USED)
def test_frames_of_the_gpu_tests_decode_and_fail(A, name, form, algo):
    """the restatement (sum-product: with host_phi) decodes some frames of the case and fails others; signbit(post) is the word
    of every frame with ok = 1 and no posterior is NaN; max_iter = 0 fails every frame and returns the clamped input"""
    c = IO.case(A, name)
    L = IO.llr(c, algo, form)
    bits, ok, iters, post = IO.ref(c, algo, form)
    assert 0 < ok.sum() < c.frames, (name, form, algo, int(ok.sum()))
    assert post.dtype == np.float32 and post.shape == L.shape and not np.isnan(post).any()
    good = ok == 1
    assert (np.signbit(post)[good] == (bits[good] == 1)).all()
    assert (iters[~good] == c.iters).all() and not bits[~good].any()
    if form == "special":
        for v in IO.SPECIAL:
            assert ((L.view(np.uint32) == np.float32(v).view(np.uint32)).any() if not np.isnan(v) else np.isnan(L).any()), v
        assert ok[0] == 1 and not bits[0].any() and ok[1] == 1 and bits[1].all()          # all NaN: all +0; all -inf: all ones
    if form == "punctured":
        punctured, shortened = IO.positions(c.n)
        assert len(punctured) == IO.PUNCTURED and not set(punctured) & set(shortened)
        assert (L[:, punctured] == 0).all() and (L[:, shortened] == LLR_CLAMP).all()
        assert not bits[:, shortened].any() and (post[:, shortened] > 1e5).all()
    if name != "big":
        b0, ok0, it0, p0 = IO.ref(c, algo, form, 0)
        assert not ok0.any() and not b0.any() and (it0 == 0).all()
        pl = prepare_llr(L)
        if algo == "minsum":
            assert (p0.view(np.uint32) == pl.view(np.uint32)).all()
        else:
            assert (p0 == pl * np.float32(1.44269504088896341) * LN2_F32).all() and np.allclose(p0, pl, rtol=3e-7, atol=0)
            assert (np.signbit(p0) == np.signbit(pl)).all()


def test_library_has_the_two_symbols_and_refuses_without_a_device(A):
    """no device needed: each entry point returns non-zero with a message for a null handle, whatever else it is handed"""
    L = A.lib()
    llr = np.zeros(8, dtype=np.float32)
    out = np.zeros(8, dtype=np.uint8)
    for what, rc in (("llr_dev", L.acg_ldpc_decode_batch_llr_dev(None, llr.ctypes.data, 1, out.ctypes.data, out.ctypes.data, None, None, None)),
                     ("llr", L.acg_ldpc_decode_batch_llr(None, llr.ctypes.data, 1, out.ctypes.data, out.ctypes.data, None, None)),
                     ("llr, no frames", L.acg_ldpc_decode_batch_llr(None, None, 0, None, None, None, None)),
                     ("llr_dev, no frames", L.acg_ldpc_decode_batch_llr_dev(None, None, 0, None, None, None, None, None)),
                     ("llr, negative frames", L.acg_ldpc_decode_batch_llr(None, llr.ctypes.data, -1, out.ctypes.data, out.ctypes.data, None, None))):
        msg = L.acg_ldpc_last_error().decode()
        assert rc != 0 and "null decoder" in msg, (what, rc, msg)
    assert not out.any()
    for name in ("acg_ldpc_decode_batch_llr_dev", "acg_ldpc_decode_batch_llr"):
        assert name in A._lib.SYMBOLS and getattr(L, name).restype is C.c_int
    header = open(os.path.join(IO.ROOT, "include", "acg_ldpc.h")).read()
    assert "int acg_ldpc_decode_batch_llr_dev(" in header and "int acg_ldpc_decode_batch_llr(" in header


@pytest.mark.parametrize("algo", SL.ALGOS)
def test_python_wrapper_refuses_before_any_handle_is_made(A, algo):
    """an array that is not real is a TypeError, one that is not two-dimensional a ValueError; the quantized class keeps refusing
    floats"""
    dec = SL.decoder(A, algo, 5)
    Hm = SL.wide(A, "deg48").Hm
    n = Hm.shape[1]
    with pytest.raises(TypeError, match="real LLRs"):
        dec.decode_llr_batch(Hm, np.zeros((2, n), dtype=np.complex64))
    with pytest.raises(TypeError, match="real LLRs"):
        dec.decode_llr_batch(Hm, np.array([["a"] * n]))
    for bad in (np.zeros(n, dtype=np.float32), np.zeros((1, 2, n))):
        with pytest.raises(ValueError, match="frames x n"):
            dec.decode_llr_batch(Hm, bad)
    assert dec.live_handles() == 0
    q = A.QuantizedMinSumDecoder(5)
    with pytest.raises(TypeError, match="integer channel values"):
        q.decode_llr_batch(Hm, np.zeros((2, n), dtype=np.float32))
    assert q.live_handles() == 0


def test_cxx_mirror_compiles_and_links(A, tmp_path):
    """the LLR entrance's members of acg_ldpc::StreamedLayeredBPDecoder / StreamedLayeredMinSumDecoder with plain g++ against the
    C-ABI library; the program decodes only where it finds a device (tests/test_streamed_layered_io_gpu.py)"""
    A.lib()
    exe = IO.build_cxx_check(tmp_path)
    out = subprocess.run([exe, os.path.join(IO.ROOT, "data", "H05.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "m=160 n=280 E=860 null handle: null decoder" in out.stdout, out.stdout
