"""GPU: the device AWGN generator (Philox4x32-10 + Box-Muller) against its numpy restatement (tests/awgn_ref.py), sample by sample.

1. acg_ldpc_awgn_dev (awgn_kernel): z_gpu = (y - s) / sigma against the float64 restatement within TOL, over code lengths with
   n % 4 = 3, 0 and 1, launches inside and beyond the grid cap, frame indices and seeds on both sides of 2^32, cycling codewords
   and three SNRs; finite, capped at 6.7637 sigma, high words of frame index and seed alive, shard invariance bit for bit.
2. the distribution battery of tests/test_awgn_ref.py on 2^26 GPU samples, bounds of 5 standard errors under i.i.d. N(0, 1).
3. the in-kernel copies of the generator (wave-group, workgroup-per-frame, layered, QP-ADMM kernels): run_experiment(...,
   noise="device") must return, field for field, the seven counters obtained from awgn_kernel's symbols decoded by the same
   decoder and classified on the host — every Monte-Carlo route, on H05 and on an n = 75 code whose last quad is ragged.

Everything up to the transcendental instructions is exact in both, so a structural error (round count, constants, counter or key
words, word pairing) shows as differences of order 1 on almost every sample; TOL only has to cover v_log_f32 / v_sin_f32 /
v_cos_f32 and four fp32 roundings."""
import contextlib
import ctypes as C
import math
import os

import numpy as np
import pytest

import awgn_ref as R

pytestmark = pytest.mark.gpu

# max |z_gpu - z_ref| measured on the MI355X against the float64 restatement: 1.086e-6 over the sample-level cases (8.5e-7 on
# n = 75, 1.09e-6 on H05, 8.3e-7 on n = 65) and 9.3e-7 over the battery's 2^26 samples.  TOL = 4 x the maximum (the instructions
# are deterministic; the margin is for inputs the cases do not visit) and must stay below 1e-3: a structural error gives order 1.
MEASURED_MAX_DZ = 1.086e-6
TOL = 4 * MEASURED_MAX_DZ
assert TOL < 1e-3

GRID_CAP = 256 * 16 * 256      # awgn_kernel's launch: at most 4096 workgroups of 256 threads, one quad per thread and trip


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


@contextlib.contextmanager
def _env(**kw):
    """developer switches read when a decoder handle is created / a Monte-Carlo run starts"""
    for k in kw:
        os.environ[k] = "1"
    try:
        yield
    finally:
        for k in kw:
            del os.environ[k]


def _awgn_dev(dec, H, first, frames, seed, snr, cws):
    """acg_ldpc_awgn_dev -> device tensor y[frames, n] (float32)"""
    import torch
    from acg_alp_ldpc_amd._lib import McCfg, check, lib
    h, _ = dec.handle(H)
    cfg = McCfg()
    cfg.frames, cfg.first_frame, cfg.snr, cfg.seed, cfg.noise = frames, first, snr, seed, 0
    if cws is not None:
        assert cws.dtype == np.uint8 and cws.flags.c_contiguous
        cfg.codewords, cfg.n_codewords = cws.ctypes.data, cws.shape[0]
    yd = torch.empty((frames, H.n), dtype=torch.float32, device="cuda")
    check(lib().acg_ldpc_awgn_dev(h, C.byref(cfg), yd.data_ptr(), None))
    dec.sync(H)
    return yd


def _awgn(dec, H, first, frames, seed, snr, cws=None):
    return _awgn_dev(dec, H, first, frames, seed, snr, cws).cpu().numpy()


class _Tally:
    """largest |z_gpu - z_ref| and the sign guard's excluded share, per SNR, over the cases of one test"""

    def __init__(self):
        self.dz, self.out, self.n = 0.0, {}, {}

    def compare(self, y, first, seed, snr, cws, what):
        frames, n = y.shape
        yr, zr, s, sg = R.symbols(first, frames, n, seed, snr, cws)
        assert np.isfinite(y).all(), what
        zg = (y.astype(np.float64) - s) / sg
        dz = float(np.abs(zg - zr).max())
        self.dz = max(self.dz, dz)
        assert float(np.abs(zg).max()) <= R.ZMAX + TOL, (what, float(np.abs(zg).max()))
        assert dz <= TOL, (what, dz)
        guard = np.abs(yr) > sg * TOL
        assert np.array_equal(np.sign(y)[guard], np.sign(yr)[guard]), what
        self.out[snr] = self.out.get(snr, 0) + int((~guard).sum())
        self.n[snr] = self.n.get(snr, 0) + guard.size
        return zg

    def finish(self, name):
        print("%s: max |z_gpu - z_ref| = %.4g (TOL %.3g)" % (name, self.dz, TOL))
        for snr in self.n:
            share, bound = self.out[snr] / self.n[snr], 4 * TOL / (float(R.sigma32(snr)) * math.sqrt(2 * math.pi))
            print("%s: %+.0f dB: sign guard leaves out %d of %d (share %.3g, bound %.3g)" % (name, snr, self.out[snr], self.n[snr], share, bound))
            assert share <= bound, (snr, share, bound)


FIRSTS = (0, 1000, 2 ** 32 - 3, 2 ** 40 + 5)
SEEDS = (1, 2 ** 32 + 1, 2 ** 63 + 12345)
SNRS = (-3.0, 2.0, 8.0)


def _codes(A, matrices):
    return {"n75": A.regular_ldpc(45, 75, 3, 5, seed=1), "H05": matrices["H05"], "n65": A.regular_ldpc(39, 65, 3, 5, seed=1)}


# ------------------------------------------------------------------------------------------ 1. awgn_kernel, sample level
@pytest.mark.parametrize("name", ["n75", "H05", "n65"])
def test_awgn_dev_samples_equal_the_restatement(A, matrices, name):
    """n = 75: the last quad has 3 live symbols; H05: n = 280; n = 65: one live symbol.  Frame counts 1 and 63 over the whole product
    first_frame x seed x SNR x (all-zero word | 11 cycling codewords: 11 divides neither the counts nor the first frames but 0); a
    count whose frames * quads exceeds the grid cap (the grid-stride loop takes a second trip) over every first_frame, the other
    parameters rotating."""
    H = A.ParityCheckMatrix(_codes(A, matrices)[name])
    n, nq = H.n, (H.n + 3) // 4
    cws = np.ascontiguousarray(np.random.default_rng(n).integers(0, 2, size=(11, n), dtype=np.uint8))   # any words: the channel does not care
    big = GRID_CAP // nq + 211
    big += big % 11 == 0
    assert big * nq > GRID_CAP and all(f % 11 for f in FIRSTS[1:]) and all(c % 11 for c in (1, 63, big))
    dec = A.MinSumDecoder(5, 0.75)
    t = _Tally()
    for frames in (1, 63):
        for first in FIRSTS:
            for seed in SEEDS:
                for snr in SNRS:
                    for cw in (None, cws):
                        y = _awgn(dec, H, first, frames, seed, snr, cw)
                        t.compare(y, first, seed, snr, cw, (name, frames, first, seed, snr, cw is not None))
    for i, first in enumerate(FIRSTS):
        seed, snr, cw = SEEDS[i % 3], SNRS[(i + 1) % 3], (cws if i % 2 else None)
        y = _awgn(dec, H, first, big, seed, snr, cw)
        t.compare(y, first, seed, snr, cw, (name, big, first, seed, snr, cw is not None))
        # shard invariance at sample level, GPU against GPU: frames [lo, lo + c) of the long run == a run started at lo
        for lo, c in ((0, 1), (1, 100), (GRID_CAP // nq - 3, 64), (big - 5, 5)):
            part = _awgn(dec, H, first + lo, c, seed, snr, cw)
            assert np.array_equal(part, y[lo:lo + c]), (name, first, lo, c)
    dec.close()
    t.finish(name)


def test_high_words_of_frame_index_and_seed_reach_the_generator(A, matrices):
    """frames g and g + 2^32, seeds s and s + 2^32: different noise (a dropped high word would repeat it exactly)"""
    H = A.ParityCheckMatrix(matrices["H05"])
    dec = A.MinSumDecoder(5, 0.75)
    for g, s in ((0, 1), (1000, 2 ** 32 + 1), (2 ** 32 - 3, 2 ** 63 + 12345)):
        sg = float(R.sigma32(2.0))
        z = (_awgn(dec, H, g, 63, s, 2.0).astype(np.float64) - 1) / sg
        zg = (_awgn(dec, H, g + 2 ** 32, 63, s, 2.0).astype(np.float64) - 1) / sg
        zs = (_awgn(dec, H, g, 63, (s + 2 ** 32) % 2 ** 64, 2.0).astype(np.float64) - 1) / sg
        assert np.array_equal(z, (_awgn(dec, H, g, 63, s, 2.0).astype(np.float64) - 1) / sg)
        for other in (zg, zs):
            assert (other != z).mean() > 0.999 and abs(R.cross(other, z)) <= 5, (g, s)
    dec.close()


# ------------------------------------------------------------------------------------------ 2. distribution battery
def test_distribution_battery_on_gpu_samples(A):
    """N = 2^26 samples (65536 frames of a 1024-symbol code, all-zero word, +2 dB), compared with the restatement over the full set
    and held to N(0, 1): every bound is 5 standard errors of the statistic under i.i.d. N(0, 1) — derived, not measured — and the
    seeds are fixed, so the test is deterministic.  The count beyond 5 sigma (38 expected) is what catches truncated tails."""
    F, n, seed, first, snr = 65536, 1024, 2024, 0, 2.0
    assert F * n == 1 << 26
    H = A.ParityCheckMatrix(A.regular_ldpc(512, 1024, 3, 6, seed=1))
    dec = A.MinSumDecoder(5, 0.75)
    sg = float(R.sigma32(snr))
    y = _awgn(dec, H, first, F, seed, snr)
    z = (y.astype(np.float64) - 1.0) / sg
    z_seed = (_awgn(dec, H, first, F, seed + 1, snr).astype(np.float64) - 1.0) / sg
    z_hi = (_awgn(dec, H, first + 2 ** 32, F, seed, snr).astype(np.float64) - 1.0) / sg
    dec.close()
    assert np.isfinite(y).all() and np.abs(z).max() <= R.ZMAX + TOL
    dz, out = 0.0, 0
    for lo in range(0, F, 4096):
        yr, zr, _, _ = R.symbols(first + lo, 4096, n, seed, snr)
        dz = max(dz, float(np.abs(z[lo:lo + 4096] - zr).max()))
        guard = np.abs(yr) > sg * TOL
        assert np.array_equal(np.sign(y[lo:lo + 4096])[guard], np.sign(yr)[guard])
        out += int((~guard).sum())
    print("battery: max |z_gpu - z_ref| over 2^26 samples = %.4g (TOL %.3g); sign guard leaves out %d" % (dz, TOL, out))
    assert dz <= TOL
    assert out / (F * n) <= 4 * TOL / (sg * math.sqrt(2 * math.pi))
    for k, (v, e, se) in R.battery(z).items():
        print("battery: %-20s %.8g (expected %.8g): %.2f standard errors" % (k, v, e, abs(v - e) / se))
        assert abs(v - e) <= 5 * se, (k, v, e, se)
    cm = R.pair_correlations(z)
    cm["seed s / s + 1"] = R.cross(z, z_seed)
    cm["frame g / g + 2^32"] = R.cross(z, z_hi)
    for k, v in cm.items():
        print("battery: cross-moment %-20s %+.2f" % (k, v))
        assert abs(v) <= 5, (k, v)


# ------------------------------------------------------------------------------------------ 3. the in-kernel copies
def _unpack(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")[:, :n]


def _mc_route_exact(A, dec, H, Hm, cws, F, snr, first, seed, syndrome):
    """awgn_kernel's symbols -> the decoder's own decode_batch_dev (float symbols) -> awgn_ref.classify on the host; the
    Monte-Carlo run of the same decoder over the same global frames must return the same seven counters"""
    import torch
    yd = _awgn_dev(dec, H, first, F, seed, snr, cws)
    nw = (H.n + 31) // 32
    bits = torch.zeros((F, nw), dtype=torch.int32, device="cuda")
    ok = torch.zeros(F, dtype=torch.uint8, device="cuda")
    it = torch.zeros(F, dtype=torch.int32, device="cuda")
    dec.decode_batch_dev(H, yd.data_ptr(), False, F, snr, bits.data_ptr(), ok.data_ptr(), it.data_ptr())
    dec.sync(H)
    y = yd.cpu().numpy()
    sent = R.sent_words(first, F, H.n, cws)
    want = R.classify(y, _unpack(bits.cpu().numpy(), H.n), ok.cpu().numpy(), it.cpu().numpy(), sent, Hm if syndrome else None)
    r = A.run_experiment(dec, cws, H, snr, frames=F, first_frame=first, noise="device", seed=seed)
    got = {k: getattr(r, k) for k in want}
    assert got == want, (got, want)
    return want


def _routes(A):
    """name -> (factory, switches, what describe() / layout() must show on H05, QP-ADMM?)"""
    BP, MS, QP = A.BeliefPropagationDecoder, A.MinSumDecoder, A.QPADMMDecoder
    lay = A.SCHEDULE_LAYERED
    r = {}
    for L in (16, 32, 64):
        r["fused-%d" % L] = (lambda L=L: BP(50, lanes_per_frame=L), {}, ["kernel=bp_fused_kernel ", dict(lanes_per_frame=L)], False)
    for L in (256, 1024):
        r["block-%d" % L] = (lambda L=L: BP(50, lanes_per_frame=L), {}, ["kernel=bp_block_kernel ", dict(lanes_per_frame=L)], False)
    for nm, pr, msg in (("f32", A.PREC_DEFAULT, "messages=fp32"), ("f16", A.PREC_F16, "messages=fp16")):
        for sw in ({}, {"ACG_LAY_UNFUSED_MC": None}):
            r["layered-%s-%s" % (nm, "unfused" if sw else "fused")] = (lambda pr=pr: MS(20, 0.75, schedule=lay, precision=pr), sw,
                                                                       ["kernel=bp_layered_kernel ", msg], False)
    r["streamed-bp"] = (lambda: BP(50, engine=A.ENGINE_STREAMED), {}, ["engine=streamed ", "kernel=bp_streamed", dict(lanes_per_frame=1)], False)
    r["admm-wave"] = (lambda: QP(1.95, 0.5, 100, 1e-5, lanes_per_frame=64), {}, ["qpadmm engine=lds ", dict(lanes_per_frame=64)], True)
    r["admm-block"] = (lambda: QP(1.95, 0.5, 100, 1e-5), {}, ["qpadmm engine=lds "], True)
    r["admm-streamed"] = (lambda: QP(1.95, 0.5, 100, 1e-5, engine=A.ENGINE_STREAMED), {}, ["kernel=admm_streamed_kernel<"], True)
    return r


ROUTES = ["fused-16", "fused-32", "fused-64", "block-256", "block-1024", "layered-f32-fused", "layered-f32-unfused",
          "layered-f16-fused", "layered-f16-unfused", "streamed-bp", "admm-wave", "admm-block", "admm-streamed"]


@pytest.mark.parametrize("code", ["H05", "n75"])
@pytest.mark.parametrize("route", ROUTES)
def test_in_kernel_generators_equal_awgn_kernel(A, matrices, route, code):
    """every Monte-Carlo route; 37 cycling codewords (coprime to every tile size), first_frame = 2^32 - 100 (the run crosses the
    low-word carry), 1003 frames (ragged for every group size), at an SNR where frames both decode and fail"""
    make, sw, want, admm = _routes(A)[route]
    Hm = _codes(A, matrices)[code]
    H = A.ParityCheckMatrix(Hm)
    G, _ = H.get_orthogonal()
    cws = np.ascontiguousarray(A.gen_random_codewords(G, 37, 11), dtype=np.uint8)
    assert cws.any() and not ((cws.astype(np.int64) @ Hm.T.astype(np.int64)) % 2).any()
    F, first, seed = 1003, 2 ** 32 - 100, 2 ** 32 + 77
    snr = -1.5 if code == "H05" else 1.0
    with _env(**sw):
        dec = make()
        d, lay = dec.describe(H), dec.layout(H)
        print("%s on %s: %s" % (route, code, d))
        if code == "H05":
            for w in want:
                if isinstance(w, str):
                    assert w in d + " ", (w, d)
                else:
                    assert lay == dict(lay, **w), (w, lay)
            assert route != "admm-block" or lay["lanes_per_frame"] > 64, lay          # one workgroup per frame
        w = _mc_route_exact(A, dec, H, Hm, cws, F, snr, first, seed, admm)
        dec.close()
    print("%s on %s: %s" % (route, code, w))
    assert w["total"] == F and 0 < w["correct"] < F and w["sum_hamming"] == w["sum_hamming_ok"] + w["sum_hamming_wrong"]


def test_chunked_monte_carlo_equals_its_shards(A):
    """the AWGN -> decode -> classify loop in bounded chunks: the streamed engine on the (3,6) 5000 x 10000 code with
    frames = chunk + 7, chunk = 2^31 / (4 n) = 53687; the whole run must equal the merged counters of two shard runs split away
    from the chunk boundary"""
    n = 10000
    chunk = (1 << 31) // (4 * n)
    assert chunk == 53687
    F = chunk + 7
    H = A.ParityCheckMatrix(A.regular_ldpc(5000, 10000, 3, 6, seed=1))
    dec = A.MinSumDecoder(8, 0.75, engine=A.ENGINE_STREAMED)
    assert "engine=streamed " in dec.describe(H)
    first, seed, snr = 2 ** 32 - 20000, 5, -1.0
    whole = A.run_experiment(dec, None, H, snr, frames=F, first_frame=first, noise="device", seed=seed)
    split = 30011
    a = A.run_experiment(dec, None, H, snr, frames=split, first_frame=first, noise="device", seed=seed)
    b = A.run_experiment(dec, None, H, snr, frames=F - split, first_frame=first + split, noise="device", seed=seed)
    dec.close()
    A.merge_exp_results(a, b)
    print("chunked: %r" % whole)
    assert (whole.as_vector() == a.as_vector()).all(), (whole, a)
    assert whole.total == F and whole.sum_hamming > 0 and whole.sum_iters >= F
