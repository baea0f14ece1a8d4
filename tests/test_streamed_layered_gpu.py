"""GPU: the streamed float layered engine (acg_ldpc_decoder_create_layered_streamed, bp_streamed_layered_kernel;
StreamedLayeredBPDecoder, StreamedLayeredMinSumDecoder) against the operation-exact restatements of tests/layered_ref.py over the
sets of ParityCheckMatrix.layers_any() — sum-product with the device's own phi — and against the workgroup-per-frame LDS engines
on every code both accept: word, flag and iteration of EVERY frame identical, nothing tolerated."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import layered_wide_cases as W
import streamed_layered_cases as SL
from layered_ref import layered_minsum, layered_sumproduct_exact
from test_layered_spa_exact_gpu import _assert_same, _extreme_frames, device_phi, ragged_graph  # noqa: F401 (device_phi: a fixture)

pytestmark = pytest.mark.gpu

KERNEL = {"bp": "bp_streamed_layered_kernel<sum-product>", "minsum": "bp_streamed_layered_kernel<minsum>"}
ITERS = 25


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


class Case:
    """a matrix, its sets, symbols, and the restatements on them, computed once each"""

    def __init__(self, A, Hm, y, snr):
        self.Hm, self.y, self.snr = np.asarray(Hm), y, snr
        self.H = A.ParityCheckMatrix(self.Hm)
        self.Z, self.layers = self.H.layers_any()
        self.frames, self.n = y.shape
        self._ref = {}

    def ref(self, algo, it, phi, f32=False):
        k = (algo, it, f32)
        if k not in self._ref:
            y = self.y.astype(np.float32) if f32 else self.y
            if algo == "minsum":
                r = layered_minsum(self.Hm, self.layers, y, self.snr, it, SL.MS_SCALE, symbols_f32=f32)
            else:
                r = layered_sumproduct_exact(self.Hm, self.layers, y, self.snr, it, phi, symbols_f32=f32)
            for a in r:
                a.setflags(write=False)
            self._ref[k] = r
        return self._ref[k]


@pytest.fixture(scope="module")
def cases(A, oracle, matrices):
    made = {}

    def get(name):
        if name in made:
            return made[name]
        if name in ("H05", "optimalH"):
            Hm, snr = matrices[name], -2.0
            G, _ = oracle.get_orthogonal(Hm)
            y = oracle.transmit_frames(oracle.gen_codewords(G, 5, 300), snr, first_seed=1)
        elif name == "ragged_graph":
            Hm, snr = ragged_graph(A), 1.0
            y = oracle.transmit_frames(np.zeros((200, Hm.shape[1]), dtype=np.uint8), snr, first_seed=9)
        else:
            Hm, snr = np.array(W.matrix(name)), W.CASES[name][2]
            y = oracle.transmit_frames(np.zeros((200, Hm.shape[1]), dtype=np.uint8), snr, first_seed=1)
        made[name] = Case(A, Hm, y, snr)
        return made[name]
    return get


def _unpack(words, n):
    w = words.cpu().numpy().view(np.uint32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.uint8).reshape(w.shape[0], -1)[:, :n]


def _describe_ok(dec, H, algo):
    d = dec.describe(H)
    assert "engine=streamed" in d and "kernel=%s " % KERNEL[algo] in d and "schedule=layered" in d and "messages=fp32" in d, d
    assert d.startswith("minsum" if algo == "minsum" else "sum-product"), d
    for word in (" T=64 ", " tiles=", " state_bytes_per_frame=", " sets="):
        assert word in d, (word, d)
    assert dec.name() == ("MS" if algo == "minsum" else "BP")
    return d


# ------------------------------------------------------------------------------------------------ 1. equals the restatement
@pytest.mark.parametrize("algo", SL.ALGOS)
@pytest.mark.parametrize("name", ["H05", "optimalH"])
def test_equals_restatement(A, cases, device_phi, name, algo):
    """300 frames at -2 dB, 25 / 3 / 1 / 0 iterations, early exit and fixed work: some frames stop after a quiet round, some pass
    the final syndrome pass, some fail; max_iter = 0 fails every frame with 0 iterations"""
    c = cases(name)
    for it in (ITERS, 3, 1, 0):
        want = c.ref(algo, it, device_phi)
        for ee in (True, False):
            dec = SL.decoder(A, algo, it, ee)
            try:
                _assert_same(dec.decode_batch(c.H, c.y, c.snr), want, (name, algo, it, "early exit" if ee else "fixed work"))
                _describe_ok(dec, c.H, algo)
            finally:
                dec.close()
        if it == ITERS:
            assert 0 < want[1].sum() < c.frames, int(want[1].sum())
        if it == 0:
            assert not want[1].any() and not want[0].any() and (want[2] == 0).all()


@pytest.mark.parametrize("algo", SL.ALGOS)
def test_equals_restatement_on_the_ragged_graph(A, cases, device_phi, algo):
    """check degrees 1 ... 8 (every instance of the one-pass step, the one-variable check's saturation), an empty check, an
    isolated variable: 200 frames at +1 dB"""
    c = cases("ragged_graph")
    degs = {int(c.Hm[l[l >= 0]].sum(axis=1)[0]) for l in c.layers}
    assert degs == {1, 2, 3, 4, 5, 6, 7, 8} and (c.Hm.sum(axis=1) == 0).any() and (c.Hm.sum(axis=0) == 0).any()
    want = c.ref(algo, ITERS, device_phi)
    for ee in (True, False):
        dec = SL.decoder(A, algo, ITERS, ee)
        try:
            _assert_same(dec.decode_batch(c.H, c.y, c.snr), want, ("ragged graph", algo, ee))
        finally:
            dec.close()
    assert 0 < want[1].sum() < c.frames, int(want[1].sum())


# ------------------------------------------------------------------------------------------------ 2. equals the LDS engines
@pytest.mark.parametrize("algo", SL.ALGOS)
@pytest.mark.parametrize("name,kernel", [("H05", "bp_layered_block_kernel"), ("qc6x32z64", "bp_layered_wide_kernel"),
                                         ("ragged", "bp_layered_wide_kernel")])
def test_equals_lds_engine(A, cases, name, kernel, algo):
    """the same symbols through the workgroup-per-frame engine (schedule = LAYERED, lanes_per_frame = 256), which walks the same
    sets: check degree 3 ... 6 (H05), 32 — four full chunks — and 3 ... 19 with 8, 9, 16, 17 among them (both sides of every
    chunk boundary).  On the wide ones the chunked prefix and suffix order meets an independent implementation."""
    c = cases(name)
    for ee in (True, False):
        lds, dec = SL.lds_decoder(A, algo, ITERS, ee), SL.decoder(A, algo, ITERS, ee)
        try:
            want = lds.decode_batch(c.H, c.y, c.snr)
            assert "kernel=%s " % kernel in lds.describe(c.H) and "lanes_per_frame=256 " in lds.describe(c.H), lds.describe(c.H)
            _assert_same(dec.decode_batch(c.H, c.y, c.snr), want, (name, algo, ee))
            _describe_ok(dec, c.H, algo)
        finally:
            lds.close()
            dec.close()
    assert 0 < want[1].sum() < c.frames, int(want[1].sum())


# ------------------------------------------------------------------------------------------------------------ 3. wide checks
@pytest.mark.parametrize("algo", SL.ALGOS)
@pytest.mark.parametrize("name", ["deg48", "deg40"])
def test_wide_checks(A, device_phi, name, algo):
    """checks of 48 and 40 variables: six and five full chunks; no LDS engine takes them"""
    c = SL.wide(A, name)
    lds = SL.lds_decoder(A, algo, c.iters)
    with pytest.raises(A.LdpcError, match="degree above 32"):
        lds.handle(c.H)
    assert lds.live_handles() == 0
    want = c.ref(algo, device_phi)
    for ee in (True, False):
        dec = SL.decoder(A, algo, c.iters, ee)
        try:
            _assert_same(dec.decode_batch(c.H, c.y(algo), c.snr(algo)), want, (name, algo, ee))
        finally:
            dec.close()
    assert 0 < want[1].sum() < c.frames, int(want[1].sum())


def test_wide_sumproduct_knife_edges(A, device_phi):
    """layered_wide_cases.knife_edge_case_wide: eight checks of degree 9, 12, 16, 17, 24, 25, 31, 32 on disjoint variables,
    max_iter = 1 — one message of the first iteration decides each frame's flag to the last bit, so a prefix or suffix sum taken
    in another order across a chunk boundary, or a short last chunk that contributes anything, shows here"""
    Hm, y, knife, high = W.knife_edge_case_wide(device_phi, 1.0, 320, 3)
    H = A.ParityCheckMatrix(Hm)
    Z, layers = H.layers_any()
    assert sorted(int(Hm[l[l >= 0]].sum(axis=1)[0]) for l in layers) == W.KNIFE_DEGREES
    post = []
    want = layered_sumproduct_exact(Hm, layers, y, 1.0, 1, device_phi, posteriors=post)
    pk = post[0][np.arange(len(y)), knife]
    assert len(y) >= 200 and (pk[~high] == 0).all() and not np.signbit(pk[~high]).any() and (pk[high] < 0).all()
    assert 0 < want[1].sum() < len(y)
    for ee in (True, False):
        dec = SL.decoder(A, "bp", 1, ee)
        try:
            _assert_same(dec.decode_batch(H, y, 1.0), want, ("knife edges", "early exit" if ee else "fixed work"))
        finally:
            dec.close()


# ------------------------------------------------------------------------------------------------------------- 4. beyond LDS
@pytest.mark.parametrize("algo", SL.ALGOS)
def test_beyond_lds(A, device_phi, monkeypatch, algo):
    """2050 x 41 000, check degree 40: 492 000 bytes of state per frame.  (Eight tiles: the 32 frames need one.)"""
    monkeypatch.setenv("ACG_STREAML_TILES", "8")
    c = SL.wide(A, "big")
    want = c.ref(algo, device_phi)
    dec = SL.decoder(A, algo, c.iters)
    try:
        _assert_same(dec.decode_batch(c.H, c.y(algo), c.snr(algo)), want, ("big", algo))
        d = _describe_ok(dec, c.H, algo)
        assert " state_bytes_per_frame=492000 " in d and " tiles=8 " in d, d
        lay = dec.layout(c.H)
        assert lay["lds_bytes_per_frame"] == 0 and lay["lanes_per_frame"] == 1 and lay["frames_per_block"] % 64 == 0, lay
        assert lay["frames_per_block"] > 0 and lay["grid_blocks"] == 8
    finally:
        dec.close()
    assert 0 < want[1].sum() < c.frames, int(want[1].sum())


# ---------------------------------------------------------------------------------------- 5. frame counts and reuse of a slab
@pytest.mark.parametrize("algo", SL.ALGOS)
def test_frame_counts_and_slab_reuse(A, cases, device_phi, monkeypatch, algo):
    """1, 63, 64, 65 frames, and 3 T + 5 on a handle of TWO tiles (ACG_STREAML_TILES=2): every slab is used twice, by frames that
    latch at other iterations and fail elsewhere.  Then another decode of other frames on the same handle, then the batch reversed:
    a slab's second occupant is not the one it had before."""
    monkeypatch.setenv("ACG_STREAML_TILES", "2")
    c = cases("H05")
    want = c.ref(algo, ITERS, device_phi)
    dec = SL.decoder(A, algo, ITERS)
    try:
        d = dec.describe(c.H)
        assert " tiles=2 " in d, d
        T = dec.layout(c.H)["frames_per_block"]
        assert T == 64 and dec.layout(c.H)["grid_blocks"] == 2
        for F in (1, 63, 64, 65, 3 * T + 5):
            assert F <= c.frames
            _assert_same(dec.decode_batch(c.H, c.y[:F], c.snr), tuple(a[:F] for a in want), (algo, "frames", F))
        lo = c.frames - (3 * T + 5)
        _assert_same(dec.decode_batch(c.H, c.y[lo:], c.snr), tuple(a[lo:] for a in want), (algo, "second decode"))
        _assert_same(dec.decode_batch(c.H, c.y[::-1], c.snr), tuple(a[::-1] for a in want), (algo, "reversed"))
        assert dec.live_handles() == 1
    finally:
        dec.close()


# --------------------------------------------------------------------------------------------------------------- 6. entrances
@pytest.mark.parametrize("algo", SL.ALGOS)
@pytest.mark.parametrize("f32", [False, True])
def test_symbol_entrances(A, cases, device_phi, algo, f32):
    """double and float symbols — two roundings of the channel LLR — through the host calls and through decode_batch_dev; a null
    iters_dev; zero frames"""
    import torch
    c = cases("H05")
    y = c.y.astype(np.float32) if f32 else c.y
    want = c.ref(algo, ITERS, device_phi, f32)
    dec = SL.decoder(A, algo, ITERS)
    try:
        _assert_same(dec.decode_batch(c.H, y, c.snr), want, (algo, "host", f32))
        F, nw = c.frames, (c.n + 31) // 32
        yd = torch.from_numpy(y).cuda()
        bits = torch.zeros((F, nw), dtype=torch.int32, device="cuda")
        ok = torch.zeros(F, dtype=torch.uint8, device="cuda")
        it = torch.zeros(F, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dec.decode_batch_dev(c.H, yd.data_ptr(), not f32, F, c.snr, bits.data_ptr(), ok.data_ptr(), it.data_ptr())
        dec.sync(c.H)
        _assert_same((_unpack(bits, c.n), ok.cpu().numpy(), it.cpu().numpy()), want, (algo, "device", f32))
        bits.zero_(), ok.zero_(), it.fill_(-7)
        torch.cuda.synchronize()
        dec.decode_batch_dev(c.H, yd.data_ptr(), not f32, F, c.snr, bits.data_ptr(), ok.data_ptr(), None)
        dec.decode_batch_dev(c.H, yd.data_ptr(), not f32, 0, c.snr, bits.data_ptr(), ok.data_ptr(), it.data_ptr())
        dec.sync(c.H)
        assert (_unpack(bits, c.n) == want[0]).all() and (ok.cpu().numpy() == want[1]).all() and (it.cpu().numpy() == -7).all()
        b0, ok0, it0 = dec.decode_batch(c.H, y[:0], c.snr)
        assert b0.shape == (0, c.n) and ok0.shape == (0,) and it0.shape == (0,)
    finally:
        dec.close()
    if not f32:
        assert 0 < want[1].sum() < c.frames


@pytest.mark.parametrize("algo", SL.ALGOS)
def test_two_streams(A, cases, device_phi, monkeypatch, algo):
    """two launches of one handle on two streams, neither waited for in between: the slabs belong to the handle, so the second
    is ordered behind the first on the device, and both are right.  (Two tiles: the launches would share every slab.)"""
    import torch
    monkeypatch.setenv("ACG_STREAML_TILES", "2")
    c = cases("H05")
    want = c.ref(algo, ITERS, device_phi)
    F, nw, h = c.frames, (c.n + 31) // 32, c.frames // 2
    dec = SL.decoder(A, algo, ITERS)
    try:
        dec.handle(c.H)
        s = [torch.cuda.Stream(), torch.cuda.Stream()]
        part = [slice(0, h), slice(h, F)]
        yd = [torch.from_numpy(np.array(c.y[p])).cuda() for p in part]
        bits = [torch.zeros((p.stop - p.start, nw), dtype=torch.int32, device="cuda") for p in part]
        ok = [torch.zeros(p.stop - p.start, dtype=torch.uint8, device="cuda") for p in part]
        it = [torch.zeros(p.stop - p.start, dtype=torch.int32, device="cuda") for p in part]
        torch.cuda.synchronize()
        for k in (0, 1, 0, 1):
            dec.decode_batch_dev(c.H, yd[k].data_ptr(), True, part[k].stop - part[k].start, c.snr, bits[k].data_ptr(), ok[k].data_ptr(),
                                 it[k].data_ptr(), s[k].cuda_stream)
        torch.cuda.synchronize()
        for k in (0, 1):
            _assert_same((_unpack(bits[k], c.n), ok[k].cpu().numpy(), it[k].cpu().numpy()), tuple(a[part[k]] for a in want), (algo, "stream", k))
    finally:
        dec.close()


# --------------------------------------------------------------------------------------------------------- 7. extreme symbols
@pytest.mark.parametrize("algo", SL.ALGOS)
def test_extreme_symbols_equal_the_lds_engine(A, oracle, matrices, algo):
    """the zero / huge / infinite symbols of test_layered_spa_exact_gpu (sum-product: all four kinds and a symbol of 1e300 whose
    LLR overflows to infinity; min-sum: zero and +-1e6, as there) give what the LDS engine gives on them"""
    Hm = matrices["H05"]
    H = A.ParityCheckMatrix(Hm)
    if algo == "bp":
        cws, y = _extreme_frames(oracle, Hm, (0, 1, 2, 3))
        last = oracle.transmit_frames(cws[:1], 1.0, first_seed=999).copy()
        last[0, 11] = 1e300 * (1.0 - 2.0 * cws[0, 11])
        y = np.vstack([y, last])
        assert np.isinf(y).any() and (y == 0).any() and not np.isnan(y).any()
    else:
        cws, y = _extreme_frames(oracle, Hm, (0, 1))
        assert (y == 0).any() and (np.abs(y) == 1e6).any() and np.isfinite(y).all()
    lds, dec = SL.lds_decoder(A, algo, ITERS), SL.decoder(A, algo, ITERS)
    try:
        want = lds.decode_batch(H, y, 1.0)
        assert "kernel=bp_layered_block_kernel " in lds.describe(H)
        _assert_same(dec.decode_batch(H, y, 1.0), want, ("extreme symbols", algo))
    finally:
        lds.close()
        dec.close()
    assert want[1].any()


# -------------------------------------------------------------------------------------------------------------- 8. Monte-Carlo
@pytest.mark.parametrize("algo", SL.ALGOS)
def test_monte_carlo_counters_equal_the_lds_engine(A, oracle, cases, algo):
    """acg_ldpc_mc_run and _detail with device noise on H05, frames beyond 2^33: the seven counters, the bit errors and the event
    frames of an LDS-engine handle with the same parameters"""
    c = cases("H05")
    G, _ = oracle.get_orthogonal(c.Hm)
    cws = oracle.gen_codewords(G, 5, 7)
    F, first, seed = 1024, (1 << 33) + 5, 2
    fields = ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong", "sum_iters")
    res = []
    for dec in (SL.lds_decoder(A, algo, ITERS), SL.decoder(A, algo, ITERS)):
        try:
            r = A.run_experiment(dec, cws, c.H, c.snr, frames=F, first_frame=first, noise="device", seed=seed)
            d = A.run_experiment_detail(dec, cws, c.H, c.snr, frames=F, first_frame=first, noise="device", seed=seed, cap=5)
            res.append((tuple(getattr(r, f) for f in fields), tuple(getattr(d, f) for f in fields), d.bit_errors, list(d.events["frame"])))
        finally:
            dec.close()
    assert res[0] == res[1], res
    assert res[1][0] == res[1][1] and res[1][0][2] == F and 0 < res[1][0][0] < F


# ----------------------------------------------------------------------------------------------------------------- 9. refusals
@pytest.mark.parametrize("algo", SL.ALGOS)
def test_refusals_on_a_live_handle(A, cases, device_phi, algo):
    """the integer entrances and the grid runs refuse the handle as one that is not quantized / not QP-ADMM; it still decodes"""
    import torch
    c = cases("H05")
    L = A.lib()
    dec = SL.decoder(A, algo, ITERS)
    try:
        h, _ = dec.handle(c.H)
        buf = np.zeros((2, c.n), dtype=np.int16)
        out = np.zeros((2, c.n), dtype=np.uint8)
        rc = L.acg_ldpc_decode_batch_q(h, buf.ctypes.data, 2, out.ctypes.data, out.ctypes.data, None, None)
        assert rc != 0 and "acg_ldpc_decoder_create_quantized" in L.acg_ldpc_last_error().decode()
        cd = torch.zeros((2, c.n), dtype=torch.int16, device="cuda")
        bd = torch.zeros((2, (c.n + 31) // 32), dtype=torch.int32, device="cuda")
        od = torch.zeros(2, dtype=torch.uint8, device="cuda")
        yd = torch.zeros((2, c.n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc = L.acg_ldpc_decode_batch_q_dev(h, cd.data_ptr(), 2, bd.data_ptr(), od.data_ptr(), None, None, None)
        assert rc != 0 and "acg_ldpc_decoder_create_quantized" in L.acg_ldpc_last_error().decode()
        rc = L.acg_ldpc_quantize_dev(h, yd.data_ptr(), 1, 2 * c.n, c.snr, cd.data_ptr(), None)
        assert rc != 0 and "acg_ldpc_decoder_create_quantized" in L.acg_ldpc_last_error().decode()
        with pytest.raises(A.LdpcError, match="QuantizedMinSumDecoder"):
            A.run_experiment_quants(dec, None, c.H, c.snr, [A.QuantConfig()], frames=64, noise="device")
        cfg, res, q = A._lib.McCfg(), A._lib.McResult(), A.QuantConfig().as_struct()
        cfg.frames, cfg.snr, cfg.seed, cfg.noise = 64, c.snr, 1, A._lib.NOISE_DEVICE_PHILOX
        rc = L.acg_ldpc_mc_run_quants(h, C.byref(cfg), C.byref(q), 1, C.byref(res))
        assert rc != 0 and "needs a decoder of acg_ldpc_decoder_create_quantized" in L.acg_ldpc_last_error().decode()
        with pytest.raises(A.LdpcError, match="QP-ADMM"):
            A.run_experiment_grid(dec, None, c.H, c.snr, [1.0], [0.5], frames=64, noise="device")
        # and the handle still decodes
        want = c.ref(algo, ITERS, device_phi)
        _assert_same(dec.decode_batch(c.H, c.y[:70], c.snr), tuple(a[:70] for a in want), (algo, "after the refusals"))
        assert dec.live_handles() == 1
    finally:
        dec.close()
    for what, d, word in (("fused", SL.decoder(A, algo, 10, engine=A.ENGINE_FUSED), "engine"),
                          ("lanes", SL.decoder(A, algo, 10, lanes_per_frame=256), "lanes_per_frame"),
                          ("flooding", SL.decoder(A, algo, 10, schedule=A.SCHEDULE_FLOODING), "schedule"),
                          ("fp16", SL.decoder(A, algo, 10, precision=A.PREC_F16), "precision")):
        with pytest.raises(A.LdpcError, match=word):
            d.handle(c.H)
        assert d.live_handles() == 0, what
    ok = SL.decoder(A, algo, 10, engine=A.ENGINE_STREAMED)
    try:
        assert "engine=streamed" in ok.describe(c.H)
    finally:
        ok.close()


# ------------------------------------------------------------------------------------------------------------ 10. C++ mirror
def test_cxx_mirror_decodes(A, tmp_path):
    """tests/cxx_streamed_layered_check.cpp: two H05 frames through acg_ldpc::StreamedLayeredBPDecoder / StreamedLayeredMinSumDecoder
    and through the LDS layered classes, words and flags equal"""
    exe = SL.build_cxx_check(tmp_path)
    out = subprocess.run([exe, os.path.join(SL.ROOT, "data", "H05.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "same=1 " in out.stdout, out.stdout
    for k in KERNEL.values():
        assert "kernel=%s " % k in out.stdout, out.stdout
    assert "kernel=bp_layered_block_kernel " in out.stdout, out.stdout
