"""GPU: the LLR entrance of the streamed float layered engine — fp32 LLRs in, fp32 posterior LLRs out (acg_ldpc_decode_batch_llr,
_llr_dev; the IO instances of bp_streamed_layered_kernel) — against the restatement tests/streamed_layered_io_ref.py with the
device's own phi: word, flag, exit iteration and EVERY posterior of EVERY frame identical bit for bit, nothing tolerated; against
the symbol entrance of the same handle; and against the slab the kernel leaves behind.  Codes, frames and SNRs are those of
tests/streamed_layered_cases.py; tests/test_streamed_layered_io.py ties the restatement to the pinned ones on the CPU."""
import os
import subprocess

import numpy as np
import pytest

import streamed_layered_cases as SL
import streamed_layered_io_cases as IO
from streamed_layered_io_ref import LLR_CLAMP, LN2_F32, prepare_llr
from test_layered_spa_exact_gpu import _assert_same, device_phi  # noqa: F401 (device_phi: a fixture)

pytestmark = pytest.mark.gpu

KERNEL = {"bp": "bp_streamed_layered_kernel<sum-product>", "minsum": "bp_streamed_layered_kernel<minsum>"}
GUARD = 96          # elements behind every output buffer of _dev_decode that no launch may touch


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


def _assert_same4(got, want, ctx):
    """word, flag and iteration as everywhere, then the bits of every posterior; the message names the first differing frame"""
    _assert_same(got[:3], want[:3], ctx)
    post, wpost = got[3], want[3]
    assert post.dtype == np.float32 and post.shape == wpost.shape, ctx
    bad = (post.view(np.uint32) != wpost.view(np.uint32)).any(axis=1)
    if bad.any():
        f = int(np.nonzero(bad)[0][0])
        v = np.nonzero(post[f].view(np.uint32) != wpost[f].view(np.uint32))[0]
        pytest.fail("%s: posteriors of %d of %d frames differ; first: frame %d (ok=%d iters=%d), %d values, e.g. variable %d: kernel %r, "
                    "restatement %r" % (ctx, int(bad.sum()), len(bad), f, want[1][f], want[2][f], len(v), v[0], float(post[f, v[0]]), float(wpost[f, v[0]])))


def _signs_are_the_word(r):
    good = r[1] == 1
    assert (np.signbit(r[3])[good] == (r[0][good] == 1)).all()


class _DevBuffers:
    """device buffers of one acg_ldpc_decode_batch_llr_dev call on L [F, n], each followed by GUARD elements of a pattern"""

    def __init__(self, L):
        import torch
        self.F, self.n = L.shape
        self.nw = (self.n + 31) // 32
        F, n, nw = self.F, self.n, self.nw
        self.llr = torch.from_numpy(np.array(L, dtype=np.float32, order="C")).cuda()
        self.bits = torch.full((F * nw + GUARD,), -1, dtype=torch.int32, device="cuda")
        self.ok = torch.full((F + GUARD,), 7, dtype=torch.uint8, device="cuda")
        self.it = torch.full((F + GUARD,), -7, dtype=torch.int32, device="cuda")
        self.post = torch.full((F * n + GUARD,), -777.0, dtype=torch.float32, device="cuda")

    def launch(self, dec, H, want_post=True, want_iters=True, stream=None):
        dec.decode_llr_batch_dev(H, self.llr.data_ptr(), self.F, self.bits.data_ptr(), self.ok.data_ptr(),
                                 self.it.data_ptr() if want_iters else None, self.post.data_ptr() if want_post else None, stream)

    def results(self, want_post=True, want_iters=True):
        """-> bits [F, n], ok, iters or None, post or None (host arrays); what was not asked for and every guard is untouched"""
        F, n, nw = self.F, self.n, self.nw
        words = self.bits.cpu().numpy().view(np.uint32)
        ok, it, post = self.ok.cpu().numpy(), self.it.cpu().numpy(), self.post.cpu().numpy()
        assert (words[F * nw:] == 0xFFFFFFFF).all() and (ok[F:] == 7).all() and (it[F:] == -7).all() and (post[F * n:] == -777.0).all()
        if not want_iters:
            assert (it == -7).all()
        if not want_post:
            assert (post == -777.0).all()
        w = words[:F * nw].reshape(F, nw)
        unpacked = ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.uint8).reshape(F, nw * 32)[:, :n]
        return (unpacked, ok[:F], it[:F] if want_iters else None, post[:F * n].reshape(F, n) if want_post else None)


def _dev_decode(dec, H, L, want_post=True, want_iters=True, stream=None):
    import torch
    b = _DevBuffers(L)
    torch.cuda.synchronize()
    b.launch(dec, H, want_post, want_iters, stream)
    torch.cuda.synchronize()
    return b.results(want_post, want_iters)


# ------------------------------------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("algo", SL.ALGOS)
@pytest.mark.parametrize("name", ["deg48", "deg40"])
def test_io_equals_restatement(A, device_phi, name, algo):
    """deg48: n = 192 = 6 trips of 32 variables through the transposing buffer; deg40: n = 400, a last trip of 16, and 200 frames,
    a last tile of 8.  Early exit and fixed work: the latched posterior, not the final state."""
    c = IO.case(A, name)
    L = IO.llr(c, algo)
    want = IO.ref(c, algo, phi=device_phi)
    for ee in (True, False):
        dec = SL.decoder(A, algo, c.iters, ee)
        try:
            _assert_same4(dec.decode_llr_batch(c.H, L), want, (name, algo, "early exit" if ee else "fixed work"))
            d = dec.describe(c.H)
            assert "kernel=%s " % KERNEL[algo] in d and d.endswith(" io=llr,post"), d
        finally:
            dec.close()
    _signs_are_the_word(want)
    assert 0 < want[1].sum() < c.frames, int(want[1].sum())


# --------------------------------------------------------------------------------------------- 2. against the symbol entrance
@pytest.mark.parametrize("algo", SL.ALGOS)
@pytest.mark.parametrize("name", ["H05", "deg48"])
def test_io_equals_symbol_entrance(A, name, algo):
    """on one handle, float symbols and the LLRs the symbol entrance forms from them, (float) ((double) y * (2 / sigma^2)): word,
    flag and iteration equal frame for frame.  H05: check degree <= 8, the one-pass step; deg48: the chunked one."""
    c = IO.case(A, name)
    y = c.y(algo).astype(np.float32)
    for ee in (True, False):
        dec = SL.decoder(A, algo, c.iters, ee)
        try:
            sym = dec.decode_batch(c.H, y, c.snr(algo))
            got = dec.decode_llr_batch(c.H, IO.llr(c, algo))
            _assert_same(got[:3], sym, (name, algo, ee))
            _signs_are_the_word(got)
            assert dec.live_handles() == 1
        finally:
            dec.close()
    assert 0 < sym[1].sum() < c.frames, int(sym[1].sum())


# --------------------------------------------------------------------------------------------- 3. the posterior and the slab
@pytest.mark.parametrize("algo", SL.ALGOS)
def test_posterior_is_the_slab_and_slab_reuse(A, device_phi, monkeypatch, algo):
    """one tile (ACG_STREAML_TILES=1): after 70 frames the slab holds the last tile, frames 64 ... 69 in lanes 0 ... 5 and zeros in
    the lanes of the frames that do not exist; its P — sum-product: times (float) ln 2 — is post[64:70], bit for bit.  Then 200
    frames: four tiles through the one slab."""
    monkeypatch.setenv("ACG_STREAML_TILES", "1")
    c = IO.case(A, "deg40")
    L = IO.llr(c, algo)
    want = IO.ref(c, algo, phi=device_phi)
    for ee in (True, False):
        dec = SL.decoder(A, algo, c.iters, ee)
        try:
            assert " tiles=1 " in dec.describe(c.H)
            got = dec.decode_llr_batch(c.H, L[:70])
            P, _ = dec.streamed_slab(c.H, 0)
            assert P.dtype == np.float32 and P.shape == (64, c.n)
            out = P[:6] if algo == "minsum" else P[:6] * LN2_F32
            assert (out.view(np.uint32) == got[3][64:70].view(np.uint32)).all(), (algo, ee)
            assert (P[6:].view(np.uint32) == 0).all()
            _assert_same4(got, tuple(a[:70] for a in want), (algo, ee, "70 frames"))
            _assert_same4(dec.decode_llr_batch(c.H, L), want, (algo, ee, "four tiles through one slab"))
        finally:
            dec.close()


# ------------------------------------------------------------------------------------------------- 4. no and one iteration
@pytest.mark.parametrize("algo", SL.ALGOS)
def test_zero_and_one_iteration(A, device_phi, algo):
    """max_iter = 0: every frame fails with 0 iterations and its posterior is the clamped input (sum-product: scaled and scaled
    back); max_iter = 1 with early_exit = 0: one iteration's posteriors"""
    c = IO.case(A, "deg40")
    L = IO.llr(c, algo, "special")
    for it, ees in ((0, (True, False)), (1, (False,))):
        want = IO.ref(c, algo, "special", it, device_phi)
        for ee in ees:
            dec = SL.decoder(A, algo, it, ee)
            try:
                _assert_same4(dec.decode_llr_batch(c.H, L), want, (algo, "max_iter", it, ee))
            finally:
                dec.close()
        if it == 0:
            assert not want[1].any() and not want[0].any() and (want[2] == 0).all()
            pl = prepare_llr(L)
            if algo == "minsum":
                assert (want[3].view(np.uint32) == pl.view(np.uint32)).all()
            else:
                assert np.allclose(want[3], pl, rtol=3e-7, atol=0) and (np.signbit(want[3]) == np.signbit(pl)).all()


# ----------------------------------------------------------------------------------------------------- 5. special values
@pytest.mark.parametrize("algo", SL.ALGOS)
@pytest.mark.parametrize("form", ["special", "punctured"])
def test_special_values_puncturing_and_shortening(A, device_phi, form, algo):
    """NaN, +-inf, +-3e38, +0 and -0 among the LLRs; 6 punctured positions (0) and 16 shortened ones (+2^20).  Nothing in the
    kernel knows about either: the restatement on the same values."""
    c = IO.case(A, "deg40")
    L = IO.llr(c, algo, form)
    want = IO.ref(c, algo, form, phi=device_phi)
    for ee in (True, False):
        dec = SL.decoder(A, algo, c.iters, ee)
        try:
            _assert_same4(dec.decode_llr_batch(c.H, L), want, (form, algo, ee))
        finally:
            dec.close()
    _signs_are_the_word(want)
    assert not np.isnan(want[3]).any() and 0 < want[1].sum() < c.frames, int(want[1].sum())
    if form == "punctured":
        _, shortened = IO.positions(c.n)
        assert not want[0][:, shortened].any() and (want[3][:, shortened] > 1e5).all() and float(LLR_CLAMP) == 2.0 ** 20


# --------------------------------------------------------------------------- 6. optional outputs, guards, a caller's stream
@pytest.mark.parametrize("algo", SL.ALGOS)
def test_optional_outputs_guards_and_streams(A, device_phi, monkeypatch, algo):
    """post_dev = NULL and iters_dev = NULL leave the other outputs as they are, and nothing is written behind frames * n floats
    (or behind any other output); 0, 1 and 65 frames; two launches back to back on two streams of the caller's, neither waited for:
    the two tiles' slabs belong to the handle, so the second is ordered behind the first on the device; the Python wrapper without
    posteriors and with caller arrays"""
    import torch
    monkeypatch.setenv("ACG_STREAML_TILES", "2")
    c = IO.case(A, "deg40")
    L = IO.llr(c, algo)
    want = IO.ref(c, algo, phi=device_phi)
    dec = SL.decoder(A, algo, c.iters)
    try:
        assert " tiles=2 " in dec.describe(c.H)
        for F in (1, 65):
            _assert_same4(_dev_decode(dec, c.H, L[:F]), tuple(a[:F] for a in want), (algo, "frames", F))
        b, ok, it, post = _dev_decode(dec, c.H, L, want_post=False)
        assert post is None
        _assert_same((b, ok, it), want[:3], (algo, "no posteriors"))
        b, ok, it, post = _dev_decode(dec, c.H, L, want_iters=False)
        assert it is None and (b == want[0]).all() and (ok == want[1]).all() and (post.view(np.uint32) == want[3].view(np.uint32)).all()
        h = c.frames // 2
        part = [slice(0, h), slice(h, c.frames)]
        bufs = [_DevBuffers(L[p]) for p in part]
        s = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        for k in (0, 1):
            bufs[k].launch(dec, c.H, stream=s[k].cuda_stream)
        torch.cuda.synchronize()
        for k in (0, 1):
            _assert_same4(bufs[k].results(), tuple(a[part[k]] for a in want), (algo, "stream", k))
        # no frames: nothing is launched, nothing is written
        none = _DevBuffers(L[:1])
        none.F = 0
        torch.cuda.synchronize()
        none.launch(dec, c.H)
        torch.cuda.synchronize()
        assert (none.ok.cpu().numpy() == 7).all() and (none.post.cpu().numpy() == -777.0).all()
        _assert_same(dec.decode_llr_batch(c.H, L, posteriors=False), want[:3], (algo, "wrapper, no posteriors"))
        out = tuple(np.empty_like(a) for a in want)
        got = dec.decode_llr_batch(c.H, L.astype(np.float64), out=out)
        assert all(g is o for g, o in zip(got, out))
        _assert_same4(got, want, (algo, "wrapper, caller arrays, float64 input"))
        e = dec.decode_llr_batch(c.H, L[:0])
        assert e[0].shape == (0, c.n) and e[3].shape == (0, c.n)
        with pytest.raises(ValueError, match="frames x n"):
            dec.decode_llr_batch(c.H, L[:, :-1])
        assert dec.live_handles() == 1
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------ 7. refusals with a device
def test_refusals_on_live_handles(A, device_phi):
    """handles of acg_ldpc_decoder_create, _create_quantized and _create_quantized_streamed: non-zero and a message that names the
    create call; on the proper handle negative frames, frames without input, the host call without bits or ok: non-zero; no frames:
    0.  Nothing is written, and the handle decodes afterwards."""
    import torch
    c = IO.case(A, "H05")
    lib = A.lib()
    L = IO.llr(c, "minsum")
    bits = np.zeros((4, c.n), dtype=np.uint8)
    ok = np.zeros(4, dtype=np.uint8)
    post = np.zeros((4, c.n), dtype=np.float32)
    ld = torch.from_numpy(np.array(L[:4])).cuda()
    bd = torch.zeros((4, (c.n + 31) // 32), dtype=torch.int32, device="cuda")
    od = torch.zeros(4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    others = [A.MinSumDecoder(5, schedule=A.SCHEDULE_LAYERED), A.QuantizedMinSumDecoder(5), A.StreamedQuantizedMinSumDecoder(5)]
    dec = SL.decoder(A, "minsum", c.iters)
    try:
        for o in others:
            h = o.handle(c.H)[0]
            for what, call in (("host", lambda: lib.acg_ldpc_decode_batch_llr(h, L.ctypes.data, 4, bits.ctypes.data, ok.ctypes.data, None, post.ctypes.data)),
                               ("device", lambda: lib.acg_ldpc_decode_batch_llr_dev(h, ld.data_ptr(), 4, bd.data_ptr(), od.data_ptr(), None, None, None)),
                               ("no frames", lambda: lib.acg_ldpc_decode_batch_llr(h, None, 0, None, None, None, None))):
                assert call() != 0, (type(o).__name__, what)
                assert "acg_ldpc_decoder_create_layered_streamed" in lib.acg_ldpc_last_error().decode(), (type(o).__name__, what)
        h = dec.handle(c.H)[0]
        for what, call, word in (
                ("negative frames, host", lambda: lib.acg_ldpc_decode_batch_llr(h, L.ctypes.data, -1, bits.ctypes.data, ok.ctypes.data, None, None), "null buffer"),
                ("negative frames, device", lambda: lib.acg_ldpc_decode_batch_llr_dev(h, ld.data_ptr(), -1, bd.data_ptr(), od.data_ptr(), None, None, None), "bad frames"),
                ("no input, host", lambda: lib.acg_ldpc_decode_batch_llr(h, None, 4, bits.ctypes.data, ok.ctypes.data, None, None), "null buffer"),
                ("no input, device", lambda: lib.acg_ldpc_decode_batch_llr_dev(h, None, 4, bd.data_ptr(), od.data_ptr(), None, None, None), "bad frames"),
                ("no bits", lambda: lib.acg_ldpc_decode_batch_llr(h, L.ctypes.data, 4, None, ok.ctypes.data, None, None), "null buffer"),
                ("no ok", lambda: lib.acg_ldpc_decode_batch_llr(h, L.ctypes.data, 4, bits.ctypes.data, None, None, None), "null buffer")):
            assert call() != 0, what
            assert word in lib.acg_ldpc_last_error().decode(), what
        assert lib.acg_ldpc_decode_batch_llr(h, None, 0, None, None, None, None) == 0
        assert lib.acg_ldpc_decode_batch_llr_dev(h, None, 0, None, None, None, None, None) == 0
        torch.cuda.synchronize()
        assert not bits.any() and not ok.any() and not post.any() and not bd.any() and not od.any()
        want = IO.ref(c, "minsum", phi=device_phi)
        _assert_same4(dec.decode_llr_batch(c.H, L[:70]), tuple(a[:70] for a in want), "after the refusals")
        # the integer entrances keep refusing the float handle
        ch = np.zeros((2, c.n), dtype=np.int16)
        assert lib.acg_ldpc_decode_batch_q(h, ch.ctypes.data, 2, bits.ctypes.data, ok.ctypes.data, None, None) != 0
        assert "acg_ldpc_decoder_create_quantized" in lib.acg_ldpc_last_error().decode()
    finally:
        dec.close()
        for o in others:
            o.close()


# ------------------------------------------------------------------------------------------------------------ 8. beyond LDS
def test_big_posteriors(A, monkeypatch):
    """2050 x 41 000, check degree 40, min-sum, 32 frames, 8 iterations, posteriors on: 1282 trips through the transposing buffer
    (the last of 8 variables) for half a tile.  (Eight tiles: the 32 frames need one.)"""
    monkeypatch.setenv("ACG_STREAML_TILES", "8")
    c = IO.case(A, "big")
    L = IO.llr(c, "minsum")
    want = IO.ref(c, "minsum")
    dec = SL.decoder(A, "minsum", c.iters)
    try:
        _assert_same4(dec.decode_llr_batch(c.H, L), want, "big")
        assert " tiles=8 " in dec.describe(c.H)
    finally:
        dec.close()
    _signs_are_the_word(want)
    assert 0 < want[1].sum() < c.frames, int(want[1].sum())


# ------------------------------------------------------------------------------------------------------------ 9. C++ mirror
def test_cxx_mirror_decodes(A, tmp_path):
    """tests/cxx_streamed_layered_io_check.cpp: two H05 frames through decode_batch and decode_llr_batch of
    acg_ldpc::StreamedLayeredBPDecoder / StreamedLayeredMinSumDecoder, words and flags equal, the posteriors' signs the words"""
    exe = IO.build_cxx_check(tmp_path)
    out = subprocess.run([exe, os.path.join(IO.ROOT, "data", "H05.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "null handle: null decoder" in out.stdout, out.stdout
    for name in ("BP", "MS"):
        assert "%s frames=2 same=1 sign_mismatch=0 " % name in out.stdout, out.stdout
    assert "kernel=%s " % KERNEL["bp"] in out.stdout and out.stdout.rstrip().endswith(" io=llr,post"), out.stdout
