"""GPU: every flooding min-sum kernel against the numpy restatement of its own storage type (tests/minsum_ref.py), EXACTLY:
word, flag and exit iteration of every frame.  Min-sum is not in the reference (parity unpinned) and the double
oracle sums in another order, which is why test_gpu_parity.py holds these kernels to agreement rates only; their arithmetic
(adds, min / med3, one multiply per minimum, bit operations) is fully determined, so against an operation-exact restatement
there is nothing to tolerate.  tests/test_minsum_ref.py ties the restatement to the oracle on the CPU.

Each instance is identified through layout() / describe(), so a silent fallback to another kernel fails the test.
Non-finite symbols are left to test_gpu_parity.py."""
import contextlib
import os

import numpy as np
import pytest

from awgn_ref import classify, sent_words
from minsum_ref import Graph, flooding_minsum
from spa_cases import irregular as _irregular, ragged as _ragged

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


@contextlib.contextmanager
def _env(**kw):
    """developer switches read when a decoder handle is created"""
    for k in kw:
        os.environ[k] = "1"
    try:
        yield
    finally:
        for k in kw:
            del os.environ[k]


def _noisy(n, frames, snr, seed):
    """all-zero codeword (the decoders are symmetric) + AWGN at Es/N0 = snr dB"""
    return 1.0 + np.sqrt(10.0 ** (-snr / 10.0) / 2.0) * np.random.default_rng(seed).standard_normal((frames, n))


def _decode(A, H, y, snr, iters, scale, want, **kw):
    """decode through the public API; `want`: substrings describe() must contain / layout() entries that must match"""
    dec = A.MinSumDecoder(iters, scale, **kw)
    try:
        out = dec.decode_batch(H, y, snr)
        d, lay = dec.describe(H), dec.layout(H)
        assert d.startswith("minsum ") and " f64=0 " in d + " ", d
        for w in want:
            if isinstance(w, str):
                assert w in d + " ", (w, d)
            else:
                assert lay == dict(lay, **w), (w, lay)
        return out
    finally:
        dec.close()


class _Refs:
    """restatement results, computed once per (graph, symbols, snr, sweeps, scale, type) and shared by the instances compared"""

    def __init__(self):
        self.graphs, self.memo = {}, {}

    def __call__(self, key, Hm, y, snr, iters, scale, dt):
        k = (key, y.dtype.str, float(snr), iters, float(scale), np.dtype(dt).str)
        if k not in self.memo:
            if key not in self.graphs:
                self.graphs[key] = Graph(Hm)
            self.memo[k] = flooding_minsum(self.graphs[key], y, snr, iters, scale, dt)
        return self.memo[k]


@pytest.fixture(scope="module")
def refs():
    return _Refs()


@pytest.fixture(scope="module")
def big(A):
    """BASELINE configs[4]: (3,6)-regular 5000 x 10000; symbols at +2 dB (exits after a few sweeps), at the threshold (-1.6 dB)
    and below it (-1.75 dB: anywhere from 20 sweeps to never), 64 frames each"""
    Hm = A.regular_ldpc(5000, 10000, 3, 6, seed=1)
    return Hm, A.ParityCheckMatrix(Hm), {snr: _noisy(10000, 64, snr, 7 + i) for i, snr in enumerate((2.0, -1.6, -1.75))}


@pytest.fixture(scope="module")
def mid(A):
    """(3,6)-regular 1500 x 3000: 256 threads per frame (pair); threshold about -1.9 dB, 1500 x 3000 needs a little more"""
    Hm = A.regular_ldpc(1500, 3000, 3, 6, seed=5)
    return Hm, A.ParityCheckMatrix(Hm)


# ------------------------------------------------------------------------------------------ fp32, wave-group kernel
# below the waterfall / in it / far above it (Es/N0, dB)
SNRS = {"H": (-3.0, -1.0, 6.0), "H05": (-3.0, -1.5, 6.0), "optimalH": (-3.5, -2.0, 6.0)}


@pytest.mark.parametrize("lpf", [16, 32, 64])
@pytest.mark.parametrize("name", ["H", "H05", "optimalH"])
def test_wave_group_fp32_exact(A, oracle, matrices, refs, name, lpf):
    """bp_fused_kernel<float, ..., ALGO=1>, 16 / 32 / 64 lanes per frame: 2003 frames per matrix over three SNRs, scales 1.0 /
    0.75 / 0.8, early exit and fixed work, double and float symbols, batches of 1, 63, 65 and the whole ragged count"""
    Hm = matrices[name]
    H = A.ParityCheckMatrix(Hm)
    G, _ = oracle.get_orthogonal(Hm)
    want = ["kernel=bp_fused_kernel ", dict(lanes_per_frame=lpf)]
    oks = []
    for i, (snr, F) in enumerate(zip(SNRS[name], (701, 699, 603))):
        cws = oracle.gen_codewords(G, 31 + i, F)
        y64 = oracle.transmit_frames(cws, snr, first_seed=5000 + 1000 * i)
        for y in (y64, y64.astype(np.float32)):
            for scale in (1.0, 0.75, 0.8):
                rb, rok, rit = refs(name, Hm, y, snr, 50, scale, np.float32)
                for ee in (True, False):
                    bits, ok, iters = _decode(A, H, y, snr, 50, scale, want, lanes_per_frame=lpf, early_exit=ee)
                    assert (bits == rb).all() and (ok == rok).all() and (iters == rit).all(), (snr, y.dtype, scale, ee)
                oks.append(rok.mean())
            for n in (1, 63, 65):
                rb, rok, rit = (a[:n] for a in refs(name, Hm, y, snr, 50, 0.75, np.float32))
                bits, ok, iters = _decode(A, H, y[:n], snr, 50, 0.75, want, lanes_per_frame=lpf)
                assert (bits == rb).all() and (ok == rok).all() and (iters == rit).all(), (snr, y.dtype, n)
    assert min(oks) < 0.5 and max(oks) == 1.0          # the SNRs reach from mostly failing to always decoding


# ------------------------------------------------------------------------------------------ fp32, one workgroup per frame
def test_block_fp32_exact_h05_256_lanes(A, oracle, matrices, refs):
    Hm = matrices["H05"]
    H = A.ParityCheckMatrix(Hm)
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 41, 515)
    for snr in (-2.0, -1.0):
        y64 = oracle.transmit_frames(cws, snr, first_seed=9000)
        for y in (y64, y64.astype(np.float32)):
            for scale in (0.75, 1.0):
                rb, rok, rit = refs("H05", Hm, y, snr, 50, scale, np.float32)
                for ee in (True, False):
                    bits, ok, iters = _decode(A, H, y, snr, 50, scale, ["kernel=bp_block_kernel ", dict(lanes_per_frame=256)],
                                              lanes_per_frame=256, early_exit=ee)
                    assert (bits == rb).all() and (ok == rok).all() and (iters == rit).all(), (snr, y.dtype, scale, ee)


def test_block_fp32_exact_on_the_configs4_code(A, big, refs):
    """the headline kernel (bp_block_kernel, 1024 threads per frame, index table in registers, regular instance) and its plain
    variants, plus the wave-group kernel forced onto this code, at +2 dB, at the threshold and below it"""
    Hm, H, ys = big
    blk = [dict(lanes_per_frame=1024, frames_per_block=1)]
    spread = {}
    for snr, y in ys.items():
        it = 60 if snr == -1.75 else 50
        rb, rok, rit = refs("big", Hm, y, snr, it, 0.75, np.float32)
        spread[snr] = (rok, rit)
        for ee in (True, False):
            bits, ok, iters = _decode(A, H, y, snr, it, 0.75, blk + ["kernel=bp_block_kernel ", "idx_reg=1 "], early_exit=ee)
            assert (bits == rb).all() and (ok == rok).all() and (iters == rit).all(), (snr, ee)
        for sw, w in ((("ACG_BP_NO_IDXREG",), "idx_reg=0 "), (("ACG_BP_NO_PLACEMENT",), "idx_reg=1 "), (("ACG_BP_NO_REGULAR",), "idx_reg=1 "),
                      (("ACG_BP_NO_IDXREG", "ACG_BP_NO_PLACEMENT", "ACG_BP_NO_REGULAR"), "idx_reg=0 ")):
            with _env(**dict.fromkeys(sw)):
                bits, ok, iters = _decode(A, H, y, snr, it, 0.75, blk + ["kernel=bp_block_kernel ", w])
            assert (bits == rb).all() and (ok == rok).all() and (iters == rit).all(), (snr, sw)
        bits, ok, iters = _decode(A, H, y[:33], snr, it, 0.75, ["kernel=bp_fused_kernel ", dict(lanes_per_frame=64)], lanes_per_frame=64)
        assert (bits == rb[:33]).all() and (ok == rok[:33]).all() and (iters == rit[:33]).all(), snr
    # float symbols and scale 1.0 at the threshold
    y32 = ys[-1.6].astype(np.float32)
    for y, scale in ((y32, 0.75), (ys[-1.6], 1.0)):
        rb, rok, rit = refs("big", Hm, y, -1.6, 50, scale, np.float32)
        bits, ok, iters = _decode(A, H, y, -1.6, 50, scale, blk)
        assert (bits == rb).all() and (ok == rok).all() and (iters == rit).all(), (y.dtype, scale)
    # the spread of exit iterations is really there: a few sweeps at +2 dB ... 20 and more at the threshold ... never
    (k2, i2), (k16, i16), (k175, i175) = spread[2.0], spread[-1.6], spread[-1.75]
    assert k2.all() and i2.max() <= 10 and i16[k16 == 1].min() > 10 and i16[k16 == 1].max() > 30
    assert 0 < k175.sum() < len(k175) and len(set(i175[k175 == 1].tolist())) > 3


# ------------------------------------------------------------------------------------------ fp32, streamed engine
@pytest.mark.parametrize("ring", [True, False])
def test_streamed_fp32_exact(A, oracle, matrices, big, refs, ring):
    """messages in HBM, one lane per frame: the LDS-DMA ring instance (default) and the register-staged one; H05 with a batch that
    is not a multiple of 64 and the configs[4] code"""
    want = ["engine=streamed ", "kernel=bp_streamed_ring_kernel<" if ring else "kernel=bp_streamed_kernel ", dict(lanes_per_frame=1)]
    sw = {} if ring else {"ACG_STREAM_NO_RING": None}
    Hm = matrices["H05"]
    H = A.ParityCheckMatrix(Hm)
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 41, 515)
    for snr in (-2.0, -1.0):
        y64 = oracle.transmit_frames(cws, snr, first_seed=9000)
        for y in (y64, y64.astype(np.float32)):
            for scale in (0.75, 1.0):
                rb, rok, rit = refs("H05", Hm, y, snr, 50, scale, np.float32)
                for ee in (True, False):
                    with _env(**sw):
                        bits, ok, iters = _decode(A, H, y, snr, 50, scale, want, engine=A.ENGINE_STREAMED, early_exit=ee)
                    assert (bits == rb).all() and (ok == rok).all() and (iters == rit).all(), (snr, y.dtype, scale, ee)
    Hm, H, ys = big
    for snr in (2.0, -1.6):
        rb, rok, rit = (a[:61] for a in refs("big", Hm, ys[snr], snr, 50, 0.75, np.float32))
        for ee in (True, False):
            with _env(**sw):
                bits, ok, iters = _decode(A, H, ys[snr][:61], snr, 50, 0.75, want, engine=A.ENGINE_STREAMED, early_exit=ee)
            assert (bits == rb).all() and (ok == rok).all() and (iters == rit).all(), (snr, ee)


# ------------------------------------------------------------------------------------------ fp16, frame pairs
def _pair_exact(A, refs, key, Hm, H, y, snr, iters, scale, L, counts):
    want = ["kernel=bp_pair_kernel ", dict(lanes_per_frame=L, frames_per_block=2)]
    ref = refs(key, Hm, y, snr, iters, scale, np.float16)
    for n in counts:
        rb, rok, rit = (a[:n] for a in ref)
        for ee in (True, False):
            bits, ok, it = _decode(A, H, y[:n], snr, iters, scale, want, precision=A.PREC_F16, early_exit=ee)
            assert (bits == rb).all() and (ok == rok).all() and (it == rit).all(), (key, snr, y.dtype, scale, n, ee)
    return ref


def test_pair_f16_exact_on_the_configs4_code(A, big, refs):
    """bp_pair_kernel<1024, regular>: +2 dB and the threshold; 63 frames (the last pair is half empty), 64, 1"""
    Hm, H, ys = big
    for snr in (2.0, -1.6):
        _, rok, rit = _pair_exact(A, refs, "big", Hm, H, ys[snr], snr, 50, 0.75, 1024, (63, 64, 1))
    assert 0 < rok.sum() and rit[rok == 1].max() > 30
    _pair_exact(A, refs, "big", Hm, H, ys[-1.6].astype(np.float32), -1.6, 50, 0.75, 1024, (64,))


def test_pair_f16_exact_256_lanes_regular_and_irregular(A, mid, refs):
    """bp_pair_kernel<256, regular> on the 1500 x 3000 code and <256, irregular> on a code with variable degree 1..4 and check
    degree 1..8 (one-variable checks: inf * scale and the sums it enters)"""
    Hm, H = mid
    for snr in (-1.2, 1.0):
        y = _noisy(3000, 131, snr, 17)
        for yy in (y, y.astype(np.float32)):
            _, rok, rit = _pair_exact(A, refs, "mid", Hm, H, yy, snr, 50, 0.75, 256, (131, 64, 1))
        assert rok.sum() > 0
    _pair_exact(A, refs, "mid", Hm, H, y, 1.0, 50, 1.0, 256, (131,))
    Hi = _irregular()
    Hc = A.ParityCheckMatrix(Hi)
    for snr in (1.0, 4.0):
        y = _noisy(Hi.shape[1], 257, snr, 19)
        for scale in (0.75, 1.0):
            for yy in (y, y.astype(np.float32)):
                _, rok, rit = _pair_exact(A, refs, "irr", Hi, Hc, yy, snr, 30, scale, 256, (257, 2, 1))
    assert 0 < rok.sum()


# ------------------------------------------------------------------------------------------ ragged graphs
def test_ragged_graph_through_every_instance(A, refs):
    """one-/two-variable checks, an empty row, isolated and degree-1 variables through every flooding min-sum instance: the
    wave-group kernel at each group size, the workgroup-per-frame kernel, both streamed instances and the half-precision pairs.
    Scale 1.0 makes sums cancel to exactly zero (sign rule x <= 0 -> -1)."""
    Hm = _ragged()
    H = A.ParityCheckMatrix(Hm)
    y64 = 1.0 + 0.9 * np.random.default_rng(3).standard_normal((601, 9))
    inst = [(dict(lanes_per_frame=L), {}, ["kernel=bp_fused_kernel ", dict(lanes_per_frame=L)], np.float32) for L in (16, 32, 64)]
    inst.append((dict(lanes_per_frame=256), {}, ["kernel=bp_block_kernel ", dict(lanes_per_frame=256)], np.float32))
    inst.append((dict(engine=A.ENGINE_STREAMED), {}, ["kernel=bp_streamed_ring_kernel<"], np.float32))
    inst.append((dict(engine=A.ENGINE_STREAMED), {"ACG_STREAM_NO_RING": None}, ["kernel=bp_streamed_kernel "], np.float32))
    inst.append((dict(precision=A.PREC_F16), {}, ["kernel=bp_pair_kernel ", dict(lanes_per_frame=256, frames_per_block=2)], np.float16))
    for kw, sw, want, dt in inst:
        for y in (y64, y64.astype(np.float32)):
            for scale in (1.0, 0.75):
                rb, rok, rit = refs("ragged", Hm, y, 0.0, 12, scale, dt)
                for ee in (True, False):
                    with _env(**sw):
                        bits, ok, iters = _decode(A, H, y, 0.0, 12, scale, want, early_exit=ee, **kw)
                    assert (bits == rb).all() and (ok == rok).all() and (iters == rit).all(), (kw, sw, y.dtype, scale, ee)
                assert 0 < rok.sum() < len(rok)
    Hi = _irregular()
    Hc = A.ParityCheckMatrix(Hi)
    y = _noisy(Hi.shape[1], 257, 1.0, 19)
    for kw, sw, want, dt in inst:
        rb, rok, rit = refs("irr", Hi, y, 1.0, 30, 0.75, dt)
        with _env(**sw):
            bits, ok, iters = _decode(A, Hc, y, 1.0, 30, 0.75, want, **kw)
        assert (bits == rb).all() and (ok == rok).all() and (iters == rit).all(), (kw, sw)


# ------------------------------------------------------------------------------------------ Monte-Carlo path
def _mc_exact(A, dec, H, Hm, cws, F, snr, dt):
    """the symbols the Monte-Carlo run decodes (acg_ldpc_awgn_dev: same Philox keys), decoded by the restatement through the
    float-symbol LLR path and classified on the host as experiment.h does -> the counters run_experiment must return"""
    import ctypes as C
    import torch
    from acg_alp_ldpc_amd._lib import McCfg, check, lib
    first, seed = 1000, 99
    h, _ = dec.handle(H)
    cfg = McCfg()
    cfg.frames, cfg.first_frame, cfg.snr, cfg.seed, cfg.noise = F, first, snr, seed, 0
    cfg.codewords, cfg.n_codewords = cws.ctypes.data, cws.shape[0]
    yd = torch.empty((F, H.n), dtype=torch.float32, device="cuda")
    check(lib().acg_ldpc_awgn_dev(h, C.byref(cfg), yd.data_ptr(), None))
    dec.sync(H)
    y = yd.cpu().numpy()
    r = A.run_experiment(dec, cws, H, snr, frames=F, first_frame=first, noise="device", seed=seed)
    rb, rok, rit = flooding_minsum(Hm, y, snr, dec.max_iter, dec.scale, dt)
    want = classify(y, rb, rok, rit, sent_words(first, F, H.n, cws))
    got = {k: getattr(r, k) for k in want}
    assert got == want, (got, want)
    return want


def test_monte_carlo_counters_equal_the_restatement(A, matrices, mid):
    Hm = matrices["H05"]
    H = A.ParityCheckMatrix(Hm)
    G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 512, 1)
    for ee in (True, False):
        dec = A.MinSumDecoder(50, 0.75, early_exit=ee)
        assert "kernel=bp_fused_kernel " in dec.describe(H)
        w = _mc_exact(A, dec, H, Hm, cws, 4099, -1.5, np.float32)
        dec.close()
        assert 0 < w["correct"] < 4099
    Hm, H = mid
    cws = np.zeros((1, 3000), np.uint8)
    dec = A.MinSumDecoder(50, 0.75, precision=A.PREC_F16)
    assert "kernel=bp_pair_kernel " in dec.describe(H)
    w = _mc_exact(A, dec, H, Hm, cws, 2049, -1.2, np.float16)
    dec.close()
    assert 0 < w["correct"] <= 2049
