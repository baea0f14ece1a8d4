"""GPU: the integer entrance of the fixed-point layered min-sum engine — int16 channel values in, int16 posteriors out
(acg_ldpc_quantize_dev, acg_ldpc_decode_batch_q_dev, acg_ldpc_decode_batch_q; the IO instances of bp_layered_q_kernel) — against
the restatement tests/layered_q_io_ref.py: word, flag, exit iteration and EVERY posterior of EVERY frame identical, nothing
tolerated.  Codes, frames, SNRs and quantisers are those of tests/layered_q_cases.py; tests/test_layered_q_io.py ties the
restatement to the pinned one on the CPU and shows on which cases a latched posterior differs from the final state."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import layered_q_cases as Q
import layered_q_io_cases as IO
from layered_q_io_ref import clamp_channel, decode_int
from layered_q_ref import limits
from test_layered_block_gpu import _assert_same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "bp_layered_q_kernel"


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


def _dec(A, it, qname="default", L=0, ee=True):
    return A.QuantizedMinSumDecoder(it, quant=A.QuantConfig(*Q.QUANTS[qname]), lanes_per_frame=L, early_exit=ee)


def _assert_same4(got, want, ctx):
    """word, flag and iteration as everywhere, then every posterior; the message names the first differing frame"""
    _assert_same(got[:3], want[:3], ctx)
    post, wpost = got[3], want[3]
    assert post.dtype == np.int16 and post.shape == wpost.shape, ctx
    bad = (post != wpost).any(axis=1)
    if bad.any():
        f = int(np.nonzero(bad)[0][0])
        v = np.nonzero(post[f] != wpost[f])[0]
        pytest.fail("%s: posteriors of %d of %d frames differ; first: frame %d (ok=%d iters=%d), %d values, e.g. variable %d: kernel %d, "
                    "restatement %d" % (ctx, int(bad.sum()), len(bad), f, want[1][f], want[2][f], len(v), v[0], post[f, v[0]], wpost[f, v[0]]))


def _dev_decode(dec, H, c, want_post=True, want_iters=True, stream=None):
    """acg_ldpc_decode_batch_q_dev on the channel values c [F, n] -> bits [F, n], ok, iters or None, post or None (host arrays);
    outputs not asked for are handed over as null pointers"""
    import torch
    F, n = c.shape
    nw = (n + 31) // 32
    cd = torch.from_numpy(np.array(c, dtype=np.int16, order="C")).cuda() if F else torch.zeros(1, dtype=torch.int16, device="cuda")
    bits = torch.full((max(F, 1), nw), -1, dtype=torch.int32, device="cuda")
    ok = torch.full((max(F, 1),), 7, dtype=torch.uint8, device="cuda")
    it = torch.full((max(F, 1),), -7, dtype=torch.int32, device="cuda")
    post = torch.full((max(F, 1), n), -777, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    dec.decode_llr_batch_dev(H, cd.data_ptr() if F else None, F, bits.data_ptr(), ok.data_ptr(), it.data_ptr() if want_iters else None,
                             post.data_ptr() if want_post else None, stream)
    torch.cuda.synchronize()
    words = bits.cpu().numpy().view(np.uint32)[:F]
    unpacked = ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.uint8).reshape(F, nw * 32)[:, :n]
    if F == 0:                                   # nothing was launched: nothing was written
        assert int(ok[0]) == 7 and int(it[0]) == -7 and int(post[0, 0]) == -777
    if not want_iters:
        assert (it == -7).all()
    if not want_post:
        assert (post == -777).all()
    return (unpacked, ok.cpu().numpy()[:F], it.cpu().numpy()[:F] if want_iters else None, post.cpu().numpy()[:F] if want_post else None)


# ------------------------------------------------------------------------------------------- 1. equality of all four outputs
@pytest.mark.parametrize("qname", sorted(Q.QUANTS))
@pytest.mark.parametrize("name", sorted(Q.CASES))
def test_io_equals_restatement(A, name, qname):
    """every case x quantiser at lanes_per_frame 0, 64 and 1024 (256 too where a set takes two passes), early exit and fixed
    work; then 0 and 1 iterations.  diag10 (n = 169): rows that are only 2-byte aligned, every chunk boundary, the one-variable
    check.  On the cases of IO.MOVING the fixed-work runs tell the latched posterior from the final state."""
    c = Q.case(A, name)
    ch = IO.channel(A, name, qname)
    want = IO.ref(A, name, qname)
    for L in (0, 64, 1024) + ((256,) if name == "qc2x10z300" else ()):
        for ee in (True, False):
            dec = _dec(A, c.iters, qname, L, ee)
            try:
                _assert_same4(dec.decode_llr_batch(c.H, ch), want, (name, qname, L, "early exit" if ee else "fixed work"))
                assert "kernel=%s " % KERNEL in dec.describe(c.H)
            finally:
                dec.close()
    for it in (0, 1):
        w = IO.ref(A, name, qname, it)
        for ee in (True, False):
            dec = _dec(A, it, qname, 0, ee)
            try:
                _assert_same4(dec.decode_llr_batch(c.H, ch), w, (name, qname, "max_iter", it, ee))
            finally:
                dec.close()
    ok = want[1] == 1
    assert ((want[3] < 0)[ok] == (want[0][ok] == 1)).all()
    if qname == "default":
        assert 0 < ok.sum() < len(ok)


# --------------------------------------------------------------------------------------------------- 2. the symbol entrance
@pytest.mark.parametrize("qname", ["default", "saturating"])
@pytest.mark.parametrize("f64", [True, False])
def test_symbol_entrance_is_quantize_dev_then_the_integer_entrance(A, f64, qname):
    """acg_ldpc_decode_batch_dev(y) = acg_ldpc_quantize_dev(y) followed by acg_ldpc_decode_batch_q_dev, for double and float
    symbols with NaN, +-inf and +-1e30 among them (those of test_layered_q_gpu.test_q_extreme_symbols); quantize_dev =
    acg_ldpc_debug_quantize"""
    import torch
    c = Q.case(A, "H05")
    rng = np.random.default_rng(11)
    y = c.y[:120].copy()
    special = np.array([1e30, -1e30, np.inf, -np.inf, np.nan])
    for f in range(len(y)):
        k = 1 + f % 9
        y[f, rng.choice(c.n, k, replace=False)] = rng.choice(special, k)
    y[0, :] = np.nan
    y[1, :] = -np.inf
    y = y if f64 else y.astype(np.float32)
    F, nw = len(y), (c.n + 31) // 32
    dec = _dec(A, c.iters, qname)
    try:
        yd = torch.from_numpy(y).cuda()
        cd = torch.full((F, c.n), -777, dtype=torch.int16, device="cuda")
        bits = torch.zeros((F, nw), dtype=torch.int32, device="cuda")
        ok = torch.zeros(F, dtype=torch.uint8, device="cuda")
        it = torch.zeros(F, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dec.decode_batch_dev(c.H, yd.data_ptr(), f64, F, c.snr, bits.data_ptr(), ok.data_ptr(), it.data_ptr())
        dec.quantize_dev(c.H, yd.data_ptr(), f64, F * c.n, c.snr, cd.data_ptr())
        dec.sync(c.H)
        ch = cd.cpu().numpy()
        assert (ch == dec.quantize(c.H, y, c.snr)).all()
        words = bits.cpu().numpy().view(np.uint32)
        sym = (((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.uint8).reshape(F, nw * 32)[:, :c.n], ok.cpu().numpy(), it.cpu().numpy())
        got = _dev_decode(dec, c.H, ch)
        _assert_same(got[:3], sym, ("symbol entrance", qname, f64))
        _assert_same4(got, decode_int(c.Hm, c.layers, ch, c.iters, Q.QUANTS[qname]), ("restatement", qname, f64))
        if qname == "default":
            assert 0 < sym[1].sum() < F
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------------------ 3. input range
def test_values_beyond_cmax_are_clamped(A):
    """channel values up to the ends of int16, -32768 and 32767 among them: the restatement on the clamped frames"""
    c = Q.case(A, "H")
    quant = Q.QUANTS["default"]
    cmax = limits(quant)[0]
    wide = IO.channel(A, "H", "default").astype(np.int32).copy()
    wide[:, ::3] *= 700
    wide[:, 1::7] *= 40
    wide = np.clip(wide, -32768, 32767)
    wide[np.arange(len(wide)), np.arange(len(wide)) % c.n] = np.where(np.arange(len(wide)) % 2, -32768, 32767)
    assert wide.min() == -32768 and wide.max() == 32767 and (np.abs(wide) > cmax).mean() > 0.3
    want = decode_int(c.Hm, c.layers, clamp_channel(wide, quant), c.iters, quant)
    assert 0 < want[1].sum() < len(wide)
    dec = _dec(A, c.iters)
    try:
        _assert_same4(dec.decode_llr_batch(c.H, wide), want, "beyond +-Cmax, int32 array")
        _assert_same4(_dev_decode(dec, c.H, wide.astype(np.int16)), want, "beyond +-Cmax, device call")
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------- 4. puncturing and shortening
def test_puncturing_and_shortening_are_channel_values(A):
    """the recipe of INTEGRATION.md on H05: punctured columns carry 0, shortened ones +Cmax where the known bit is 0 and -Cmax
    where it is 1.  Nothing in the kernel knows about either: the restatement on the same values."""
    c = Q.case(A, "H05")
    quant = Q.QUANTS["default"]
    cmax = limits(quant)[0]
    ch = IO.channel(A, "H05", "default").copy()
    punctured, shortened = np.arange(3, c.n, 29), np.arange(10, c.n, 17)
    ch[:, punctured] = 0
    ch[:, shortened] = np.where(c.cws[:, shortened] == 1, -cmax, cmax)
    want = decode_int(c.Hm, c.layers, ch, c.iters, quant)
    assert 0 < want[1].sum() < len(ch)
    assert (want[0][want[1] == 1][:, shortened] == c.cws[want[1] == 1][:, shortened]).mean() > 0.99
    dec = _dec(A, c.iters)
    try:
        _assert_same4(dec.decode_llr_batch(c.H, ch), want, "punctured and shortened")
    finally:
        dec.close()


# ---------------------------------------------------------------------------------- 5. optional outputs and batch shapes
def test_optional_outputs_batch_shapes_and_a_callers_stream(A):
    """post_dev = NULL and iters_dev = NULL leave the other outputs as they are (and the buffers untouched); 0, 1 and 63 frames
    on one handle; one launch on a stream of the caller's; the Python wrapper without posteriors and with caller arrays"""
    import torch
    c = Q.case(A, "ragged")
    ch = IO.channel(A, "ragged", "default")
    want = IO.ref(A, "ragged", "default")
    dec = _dec(A, c.iters)
    try:
        for F in (0, 1, 63):
            _assert_same4(_dev_decode(dec, c.H, ch[:F]), tuple(a[:F] for a in want), ("frames", F))
        b, ok, it, post = _dev_decode(dec, c.H, ch, want_post=False)
        assert post is None
        _assert_same((b, ok, it), want[:3], "no posteriors")
        b, ok, it, post = _dev_decode(dec, c.H, ch, want_iters=False)
        assert it is None and (b == want[0]).all() and (ok == want[1]).all() and (post == want[3]).all()
        s = torch.cuda.Stream()
        _assert_same4(_dev_decode(dec, c.H, ch, stream=s.cuda_stream), want, "caller's stream")
        _assert_same(dec.decode_llr_batch(c.H, ch, posteriors=False), want[:3], "wrapper, no posteriors")
        out = (np.empty_like(want[0]), np.empty_like(want[1]), np.empty_like(want[2]), np.empty_like(want[3]))
        got = dec.decode_llr_batch(c.H, ch.astype(np.int64), out=out)
        assert all(g is o for g, o in zip(got, out))
        _assert_same4(got, want, "wrapper, caller arrays, int64 input")
        assert dec.live_handles() == 1
    finally:
        dec.close()


def test_refusals_on_a_live_handle(A):
    """a handle of acg_ldpc_decoder_create, negative frames, frames without input, the host call without bits or ok: non-zero and
    a message each; no frames: 0"""
    c = Q.case(A, "H05")
    L = A.lib()
    ch = IO.channel(A, "H05", "default")
    bits = np.zeros((4, c.n), dtype=np.uint8)
    ok = np.zeros(4, dtype=np.uint8)
    ms = A.MinSumDecoder(5, schedule=A.SCHEDULE_LAYERED)
    dec = _dec(A, 5)
    try:
        h, hq = ms.handle(c.H)[0], dec.handle(c.H)[0]
        for what, rc, word in (
                ("float handle, host", L.acg_ldpc_decode_batch_q(h, ch.ctypes.data, 4, bits.ctypes.data, ok.ctypes.data, None, None), "create_quantized"),
                ("float handle, device", L.acg_ldpc_decode_batch_q_dev(h, ch.ctypes.data, 4, None, None, None, None, None), "create_quantized"),
                ("float handle, quantiser", L.acg_ldpc_quantize_dev(h, ch.ctypes.data, 1, 4, 0.0, ch.ctypes.data, None), "create_quantized"),
                ("float handle, no frames", L.acg_ldpc_decode_batch_q(h, None, 0, None, None, None, None), "create_quantized"),
                ("negative frames, host", L.acg_ldpc_decode_batch_q(hq, ch.ctypes.data, -1, bits.ctypes.data, ok.ctypes.data, None, None), "null buffer"),
                ("negative frames, device", L.acg_ldpc_decode_batch_q_dev(hq, ch.ctypes.data, -1, None, None, None, None, None), "bad frames"),
                ("negative count", L.acg_ldpc_quantize_dev(hq, ch.ctypes.data, 1, -1, 0.0, ch.ctypes.data, None), "bad count"),
                ("no input, host", L.acg_ldpc_decode_batch_q(hq, None, 4, bits.ctypes.data, ok.ctypes.data, None, None), "null buffer"),
                ("no input, device", L.acg_ldpc_decode_batch_q_dev(hq, None, 4, None, None, None, None, None), "bad frames"),
                ("no input, quantiser", L.acg_ldpc_quantize_dev(hq, None, 1, 4, 0.0, ch.ctypes.data, None), "bad count"),
                ("no output, quantiser", L.acg_ldpc_quantize_dev(hq, ch.ctypes.data, 1, 4, 0.0, None, None), "bad count"),
                ("no bits", L.acg_ldpc_decode_batch_q(hq, ch.ctypes.data, 4, None, ok.ctypes.data, None, None), "null buffer"),
                ("no ok", L.acg_ldpc_decode_batch_q(hq, ch.ctypes.data, 4, bits.ctypes.data, None, None, None), "null buffer")):
            assert rc != 0, what
        assert not bits.any() and not ok.any()
        # (the messages: one call each, read before the next call replaces it)
        assert L.acg_ldpc_decode_batch_q(h, ch.ctypes.data, 4, bits.ctypes.data, ok.ctypes.data, None, None) != 0
        assert "create_quantized" in L.acg_ldpc_last_error().decode()
        assert L.acg_ldpc_decode_batch_q_dev(hq, None, 4, None, None, None, None, None) != 0
        assert "bad frames" in L.acg_ldpc_last_error().decode()
        assert L.acg_ldpc_decode_batch_q(hq, ch.ctypes.data, 4, None, ok.ctypes.data, None, None) != 0
        assert "null buffer" in L.acg_ldpc_last_error().decode()
        assert L.acg_ldpc_decode_batch_q(hq, None, 0, None, None, None, None) == 0
        assert L.acg_ldpc_decode_batch_q_dev(hq, None, 0, None, None, None, None, None) == 0
        assert L.acg_ldpc_quantize_dev(hq, None, 1, 0, 0.0, None, None) == 0
    finally:
        ms.close()
        dec.close()


# ------------------------------------------------------------------------------------------- 6. dynamic LDS above 64 KiB
def test_a_frame_above_64_kib_of_lds(A):
    """6000 disjoint checks of degree 4 on 24 000 variables: 75 016 bytes of LDS, one set in six passes at L = 1024.  Every check
    holds the magnitudes 3, 9, 15, 21 in some order: an even check is quiet at once, an odd one flips its weakest variable in
    iteration 1 and is quiet in iteration 2 — frame 0 (all positive) latches at 1, the others at 2."""
    Hm = IO.disjoint4()
    n = Hm.shape[1]
    H = A.ParityCheckMatrix(Hm)
    Z, layers = H.layers_wide()
    assert len(layers) == 1 and int((layers[0] >= 0).sum()) == 6000
    rng = np.random.default_rng(3)
    mags = np.array([3, 9, 15, 21])
    ch = np.stack([np.concatenate([rng.permutation(mags) for _ in range(6000)]) for _ in range(4)])
    ch = (ch * rng.choice([-1, 1], size=ch.shape)).astype(np.int16)
    ch[0] = np.abs(ch[0])
    want = decode_int(Hm, layers, ch, 3)
    assert list(want[1]) == [1, 1, 1, 1] and list(want[2]) == [1, 2, 2, 2] and want[0][1:].any()
    dec = A.QuantizedMinSumDecoder(3, lanes_per_frame=1024)
    try:
        d = dec.describe(H)
        assert "lds_block=75016 " in d and "lanes_per_frame=1024 " in d, d
        _assert_same4(dec.decode_llr_batch(H, ch), want, "75 016 bytes of LDS, host call")
        _assert_same4(_dev_decode(dec, H, ch), want, "75 016 bytes of LDS, device call")
        b, ok, it = dec.decode_batch(H, np.where(want[0] == 1, -1.0, 1.0), 0.0)          # the symbol entrance's instance still runs
        assert (b == want[0]).all() and ok.all()
    finally:
        dec.close()


# ------------------------------------------------------------------------------------- 7. host pipeline across a chunk boundary
def test_host_pipeline_across_a_chunk_boundary(A):
    """65 536 + 300 frames of H through acg_ldpc_decode_batch_q (one chunk is 65 536 frames for n = 128): the case's 300 frames
    tiled, with and without posteriors, against the tiled restatement"""
    c = Q.case(A, "H")
    ch = IO.channel(A, "H", "default")
    want = IO.ref(A, "H", "default")
    F = 65536 + 300
    idx = np.arange(F) % len(ch)
    big = np.ascontiguousarray(ch[idx])
    dec = _dec(A, c.iters)
    try:
        for posteriors in (True, False):
            got = dec.decode_llr_batch(c.H, big, posteriors=posteriors)
            for k, name in enumerate(("word", "flag", "iteration", "posterior")[:len(got)]):
                same = got[k] == want[k][idx]
                if not same.all():
                    f = int(np.nonzero(~(same.reshape(F, -1).all(axis=1)))[0][0])
                    pytest.fail("%s of frame %d (copy of frame %d) differs, posteriors=%s" % (name, f, idx[f], posteriors))
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------------------ 8. C++ mirror
def test_cxx_mirror_agrees_with_python(A, tmp_path):
    """tests/cxx_quant_io_check.cpp: QuantizedMinSumDecoder::quantize and decode_llr_batch of include/acg_ldpc_decoder.hpp on the
    first 100 frames of H05 = the Python mirror's channel values and the restatement's four outputs"""
    exe = IO.build_cxx_io_check(tmp_path)
    c = Q.case(A, "H05")
    F = 100
    sym, outp = str(tmp_path / "y.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(c.y[:F], dtype=np.float64).tofile(sym)
    out = subprocess.run([exe, os.path.join(ROOT, "data", "H05.txt"), str(c.iters), repr(c.snr), sym, outp], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "m=160 n=280 E=860 null handle: null decoder" in out.stdout, out.stdout
    want = tuple(a[:F] for a in IO.ref(A, "H05", "default"))
    assert "QMS frames=%d ok=%d sign_mismatch=0 handles=1" % (F, int(want[1].sum())) in out.stdout, out.stdout
    raw = np.fromfile(outp, dtype=np.uint8)
    sizes = [F * c.n * 2, F * c.n, F, F * 4, F * c.n * 2]
    assert len(raw) == sum(sizes)
    parts = np.split(raw, np.cumsum(sizes)[:-1])
    ch = parts[0].view(np.int16).reshape(F, c.n)
    dec = _dec(A, c.iters)
    try:
        assert (ch == dec.quantize(c.H, c.y[:F], c.snr)).all() and (ch == IO.channel(A, "H05", "default")[:F]).all()
    finally:
        dec.close()
    got = (parts[1].reshape(F, c.n), parts[2], parts[3].view(np.int32), parts[4].view(np.int16).reshape(F, c.n))
    _assert_same4(got, want, "C++ mirror")
