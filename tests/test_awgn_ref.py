"""CPU: the numpy restatement of the device AWGN generator (tests/awgn_ref.py) against what is known independently of the
kernels — the Random123 known answers of Philox4x32-10, the analytic extremes of this Box-Muller, and N(0, 1) itself.  Every
statistic test_awgn_exact_gpu.py asks of the GPU's samples is asked of the restatement's first, with the same 5-standard-error
bounds, so the battery cannot demand what a correct generator does not deliver."""
import math

import numpy as np

import awgn_ref as R


def test_philox_random123_known_answers():
    """kat_vectors of Random123 (philox4x32 10): zero counter and key; the digits of pi"""
    assert [int(x) for x in R.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    got = R.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
    assert [int(x) for x in got] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    # vectorised: the same words from arrays, whatever the broadcast
    c0 = np.array([0, 0x243F6A88], dtype=np.uint64)
    out = R.philox4x32_10(c0, [0, 0x85A308D3], [0, 0x13198A2E], [0, 0x03707344], [0, 0xA4093822], [0, 0x299F31D0])
    assert [int(x[0]) for x in out] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(x[1]) for x in out] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_uniforms_are_the_fp32_values_of_the_kernel():
    """(float) a rounds to nearest even at 24 bits (2^24 + 1 -> 2^24, 2^25 + 6 -> 2^25 + 8, 2^32 - 128 -> 2^32), + 0.5f rounds again,
    * 2^-32 is exact; u2 keeps the top 24 bits of b"""
    a = np.array([0, 1, 2 ** 24 + 1, 2 ** 25 + 6, 2 ** 32 - 1, 2 ** 32 - 129, 2 ** 32 - 128], dtype=np.uint64)
    u1, u2 = R.uniforms(a, a)
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    assert u1.tolist() == [2.0 ** -33, 1.5 * 2.0 ** -32, 2.0 ** -8, (2 ** 25 + 8) * 2.0 ** -32, 1.0, 1.0 - 2.0 ** -24, 1.0]
    assert u2.tolist() == [0.0, 0.0, 2.0 ** -8, 2.0 ** -7, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24]
    assert (u1 > 0).all() and (u2 < 1).all()


def test_box_muller_is_finite_and_capped():
    """a = 0: u1 = 2^-33, the longest radius, sqrt(2 * 33 * ln 2) = 6.7637; a = 2^32 - 1: u1 rounds to 1.0f and z = +-0, not NaN"""
    assert abs(R.ZMAX - 6.7637) < 5e-5
    b = (np.arange(4096, dtype=np.uint64) << np.uint64(20))
    z0, z1 = R.box_muller(np.zeros(4096, dtype=np.uint64), b)
    assert np.isfinite(z0).all() and np.isfinite(z1).all()
    assert np.abs(np.hypot(z0, z1) - R.ZMAX).max() < 1e-12 and max(np.abs(z0).max(), np.abs(z1).max()) <= R.ZMAX + 1e-12
    assert abs(z0[0] - R.ZMAX) < 1e-12 and abs(z1[1024] - R.ZMAX) < 1e-12           # u2 = 0 and a quarter turn
    z0, z1 = R.box_muller(np.full(4096, 2 ** 32 - 1, dtype=np.uint64), b)
    assert (z0 == 0).all() and (z1 == 0).all()
    rng = np.random.default_rng(1)
    a, b = (rng.integers(0, 2 ** 32, size=1 << 20, dtype=np.uint64) for _ in range(2))
    z0, z1 = R.box_muller(a, b)
    assert np.isfinite(z0).all() and np.isfinite(z1).all() and max(np.abs(z0).max(), np.abs(z1).max()) <= R.ZMAX + 1e-12


def test_normals_layout_counter_and_key():
    """symbol 4q + e of frame g comes from counter (g_lo, g_hi, q, 0) and key (seed_lo, seed_hi); a row does not depend on where the
    run started; both high words count"""
    g, seed, n = 2 ** 32 - 3, 2 ** 32 + 1, 75
    z = R.normals(g, 9, n, seed)
    assert z.shape == (9, 75)
    for f, q in ((0, 0), (2, 18), (3, 7), (8, 18)):            # frame 3 is g = 2^32: (0, 1, q, 0)
        gf = g + f
        w = R.philox4x32_10(gf & 0xFFFFFFFF, gf >> 32, q, 0, seed & 0xFFFFFFFF, seed >> 32)
        quad = np.concatenate([R.box_muller(w[0], w[1]), R.box_muller(w[2], w[3])]).ravel()
        live = min(4, n - 4 * q)
        assert live == (3 if q == 18 else 4)
        assert np.array_equal(z[f, 4 * q:4 * q + live], quad[:live])
    assert np.array_equal(R.normals(g + 2, 5, n, seed), z[2:7])
    assert np.array_equal(R.normals(g, 9, 65, seed), z[:, :65])        # n changes the live symbols of the last quad only
    assert np.abs(R.normals(g + 2 ** 32, 9, n, seed) - z).min() > 0     # frame_hi is in the counter
    assert np.abs(R.normals(g, 9, n, seed + 2 ** 32) - z).min() > 0     # seed_hi is in the key
    assert np.abs(R.normals(g, 9, n, seed + 1) - z).min() > 0
    assert np.array_equal(R.normals(5, 3, n, 2 ** 63 + 12345), R.normals(5, 3, n, 2 ** 63 + 12345 - 2 ** 64))   # seed as int64


def test_symbols_and_classify():
    cws = np.random.default_rng(2).integers(0, 2, size=(7, 75), dtype=np.uint8)
    y, z, s, sg = R.symbols(12, 20, 75, 3, 2.0, cws)
    assert sg == float(np.float32(math.sqrt(10 ** -0.2 / 2))) and np.array_equal(y, s + sg * z)
    sent = R.sent_words(12, 20, 75, cws)
    assert np.array_equal(sent[0], cws[5]) and np.array_equal(sent[2], cws[0]) and np.array_equal(s, 1.0 - 2.0 * sent)
    assert not R.sent_words(0, 3, 5, None).any()
    # five frames by hand: correct, pseudo-codeword, not ok, ok but wrong with H given (syndrome), correct
    H = np.array([[1, 1, 0, 0], [0, 0, 1, 1]], dtype=np.uint8)
    sent = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0], [0, 0, 1, 1], [1, 1, 1, 1]], dtype=np.uint8)
    bits = np.array([[0, 0, 0, 0], [1, 1, 0, 0], [1, 1, 0, 0], [0, 1, 1, 1], [1, 1, 1, 1]], dtype=np.uint8)
    y = np.array([[1, 0.0, -1, 2], [1, 1, 1, 1], [-1, 1, 1, 1], [1, 1, 1, -1], [-1, -1, -1, 0.0]])
    ham = [2, 0, 1, 1, 0]                                        # y = 0 reads as a 1
    ok = np.array([1, 1, 0, 1, 1], dtype=np.uint8)
    it = np.array([3, 4, 50, 50, 1])
    assert R.classify(y, bits, ok, it, sent) == dict(correct=2, pseudo=2, total=5, sum_iters=108, sum_hamming=sum(ham),
                                                     sum_hamming_ok=2, sum_hamming_wrong=2)
    assert R.classify(y, bits, ok, it, sent, H) == dict(correct=2, pseudo=1, total=5, sum_iters=108, sum_hamming=sum(ham),
                                                        sum_hamming_ok=2, sum_hamming_wrong=2)


def test_battery_passes_on_the_restatement():
    """16384 x 1057 samples (n % 4 == 1), seed 12345, from frame 1000.  Measured |deviation| in standard errors: mean 0.23,
    variance 1.26, third moment 0.68, fourth moment 1.68, |z| > 1..5: 0.66 0.28 0.39 2.36 0.97, chi-square 0.11, cross-moments
    <= 1.4.  Asserted at the GPU test's 5."""
    z = R.normals(1000, 16384, 1057, 12345)
    for k, (v, e, se) in R.battery(z).items():
        print("%-20s %.6g (expected %.6g): %.2f standard errors" % (k, v, e, abs(v - e) / se))
        assert abs(v - e) <= 5 * se, (k, v, e, se)
    cm = R.pair_correlations(z[:, :1056])
    cm["seed s / s + 1"] = R.cross(z, R.normals(1000, 16384, 1057, 12346))
    cm["frame g / g + 2^32"] = R.cross(z, R.normals(1000 + 2 ** 32, 16384, 1057, 12345))
    for k, v in cm.items():
        print("%-20s %+.2f" % (k, v))
        assert abs(v) <= 5, (k, v)


def test_battery_detects_the_defects_it_is_there_for():
    """the statistics have the power the issue counts on, at the GPU test's N = 2^26 scaled down to what runs here in a second
    (bounds scale with sqrt N, so what shows here shows there): a 1 % variance error, tails cut at 4.9 sigma (u1 floor 2^-17),
    z2 / z3 made from the words of z0 / z1"""
    z = R.normals(0, 8192, 1024, 7)                                       # 2^23 samples
    b = R.battery(z * math.sqrt(1.01))
    assert abs(b["variance"][0] - 1) > 5 * b["variance"][2]
    # tails: at N = 2^26 the expected count beyond 5 sigma is 38 and the bound 5 * sqrt(38) = 31: zero samples there fails
    N = 1 << 26
    p5 = math.erfc(5 / math.sqrt(2))
    assert 37 < N * p5 < 40 and N * p5 - 0 > 5 * math.sqrt(N * p5)
    assert math.sqrt(2 * 17 * math.log(2)) < 5
    q = z.reshape(8192, 256, 4).copy()
    q[:, :, 2:] = q[:, :, :2]
    assert abs(R.pair_correlations(q.reshape(8192, 1024))["quad e0.e2"]) > 1000


def test_sign_guard_share_is_what_the_density_allows():
    """the GPU test compares signs only where |y_ref| > sigma * tol; the share it leaves out depends on the restatement alone and
    must stay under 4 * tol * pdf_max with pdf_max = 1 / (sigma sqrt(2 pi)) — checked here for the largest tol the issue admits and
    for one a hundred times smaller, at the three SNRs, on 2^22 samples of the GPU battery's stream"""
    for snr in (-3.0, 2.0, 8.0):
        y, _, _, sg = R.symbols(0, 4096, 1024, 2024, snr, None)
        for tol in (1e-3, 1e-5):
            share = float((np.abs(y) <= sg * tol).mean())
            bound = 4 * tol / (sg * math.sqrt(2 * math.pi))
            print("snr %+.0f tol %g: share %.3g bound %.3g" % (snr, tol, share, bound))
            assert share <= bound
