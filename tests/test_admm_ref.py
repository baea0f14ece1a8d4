"""tests/admm_ref.py qualified on the CPU: in float64 it IS the reference (word, flag and sweep count of
oracle.qpadmm_decode, and of the reference itself where it is built); in float32 it tells the true sweep from one with a
single operation changed, on the very frame sets tests/test_admm_f32_exact_gpu.py holds the kernels to; and those sets keep
clear of the band in which the order of the residual sum could move a frame's last sweep."""
import numpy as np
import pytest

import admm_f32_sets as S
import admm_ref


@pytest.fixture(scope="module")
def sets(oracle, matrices):
    return S.FrameSets(oracle, matrices)


def same(a, b):
    return all((np.asarray(x) == np.asarray(y)).all() for x, y in zip(a[:3], b[:3]))


def test_problem_and_variance_equal_the_oracle(oracle, sets):
    from test_admm_stream_tables import ragged_graph
    for name, H in list(sets.H.items()) + [("ragged", ragged_graph())]:
        want = oracle.admm_matrix(H)
        got = admm_ref.admm_problem(H)
        for w, g in zip(want, got):
            assert w.dtype == g.dtype and w.shape == g.shape and (w == g).all(), name
    for snr in (-3.0, -2.0, -1.5, 0.0, 1.0, 2.0, 0.3):
        assert admm_ref.llr_variance(snr) == oracle.llr_variance(snr)


@pytest.mark.parametrize("s", S.EARLY_EXIT_SETS, ids=lambda s: "%s%+g_a%g" % (s.code, s.snr, s.alpha))
def test_float64_is_the_oracle_on_the_gpu_sets(oracle, sets, s):
    y = sets.frames(s.code, s.snr)[1]
    for eps in (s.eps, 0.0):
        want = oracle.qpadmm_decode(sets.H[s.code], y, s.snr, s.alpha, s.mu, s.budget, eps, threads=4)
        got = admm_ref.qpadmm_ref(sets.H[s.code], y, s.snr, s.alpha, s.mu, s.budget, eps, np.float64, problem=sets.problem(s.code))
        assert same(got, want), (s, eps)
        assert got[0].dtype == np.uint8 and got[1].dtype == np.uint8 and got[2].dtype == np.int32
        if eps == 0.0:
            assert (got[2] == s.budget).all() and np.isinf(got[3]).all()
    if s.code in ("H", "small"):
        fixed = admm_ref.qpadmm_ref(sets.H[s.code], y, s.snr, s.alpha, s.mu, s.budget, s.eps, np.float64, early_exit=False,
                                    problem=sets.problem(s.code))
        assert same(fixed, got)        # early_exit=False and eps = 0 are the same run


def test_float64_is_the_oracle_on_the_synthetic_codes(oracle, sets):
    """the frames and parameters of test_qpadmm_mixed_check_degrees_and_long_lists and test_qpadmm_guard_and_small_checks:
    one- and two-variable checks, an empty row, long lists; the guard; sweep budgets 0 and 1 with zero, -0, NaN and denormal
    symbols"""
    H = S.mixed_code()
    rng = np.random.default_rng(12)
    y = 1.0 + 0.7 * rng.standard_normal((120, H.shape[1]))
    want = oracle.qpadmm_decode(H, y, 1.0, 0.6, 1.0, 60, 1e-6, threads=4)
    assert same(admm_ref.qpadmm_ref(H, y, 1.0, 0.6, 1.0, 60, 1e-6, np.float64), want)
    assert 1 < want[2].mean() < 60
    H = S.small_code()
    rng = np.random.default_rng(5)
    y = 1.0 + 0.8 * rng.standard_normal((200, 8))
    want = oracle.qpadmm_decode(H, y, 1.0, 0.6, 1.0, 80, 1e-6, threads=2)
    assert same(admm_ref.qpadmm_ref(H, y, 1.0, 0.6, 1.0, 80, 1e-6, np.float64), want)
    y0 = y.copy()
    y0[0, :4] = [0.0, -0.0, np.nan, 1e-320]
    for budget in (0, 1):
        want = oracle.qpadmm_decode(H, y0, 1.0, 0.6, 1.0, budget, 1e-6, threads=2)
        got = admm_ref.qpadmm_ref(H, y0, 1.0, 0.6, 1.0, budget, 1e-6, np.float64)
        assert same(got, want) and (got[2] == budget).all() and got[1].all(), budget
    got32 = admm_ref.qpadmm_ref(H, y0, 1.0, 0.6, 1.0, 0, 1e-6, np.float32)
    want0 = oracle.qpadmm_decode(H, y0, 1.0, 0.6, 1.0, 0, 1e-6, threads=2)
    assert want0[0][0, 3] == 1
    want0[0][0, 3] = 0                 # the denormal symbol underflows to q = 0 in float32
    assert same(got32, want0)
    # the guard e_min * mu <= alpha: (zeros, false), no sweeps — on H05 (e_min = 4) and on the small code (e_min = 1)
    for Hg, a, mu in ((sets.H["H05"], 2.0, 0.5), (H, 1.0, 1.0), (H, 1.5, 1.0)):
        yg = np.ones((5, Hg.shape[1]))
        want = oracle.qpadmm_decode(Hg, yg, 0.0, a, mu, 10, 1e-5)
        for T in (np.float64, np.float32):
            got = admm_ref.qpadmm_ref(Hg, yg, 0.0, a, mu, 10, 1e-5, T)
            assert same(got, want) and not got[1].any() and not got[0].any() and not got[2].any()


def test_float64_is_the_reference_itself(ref, sets):
    for s in (S.make("H05", -2.0), S.make("optimalH", -2.0, *S.HIGH_GAIN), S.make("H", 1.0), S.make("mixed", -2.0)):
        y = sets.frames(s.code, s.snr)[1][:6]
        rb, rok, _ = ref.qpadmm_decode(sets.H[s.code], y, s.snr, s.alpha, s.mu, s.budget, s.eps)
        got = admm_ref.qpadmm_ref(sets.H[s.code], y, s.snr, s.alpha, s.mu, s.budget, s.eps, np.float64)
        assert (got[0] == rb).all() and (got[1] == rok).all(), s


@pytest.mark.parametrize("s", S.EARLY_EXIT_SETS, ids=lambda s: "%s%+g_a%g" % (s.code, s.snr, s.alpha))
def test_sets_stop_early_and_late_and_keep_clear_of_the_band(sets, s):
    """Band census.  A kernel adds the float32 terms (z - r)^2 in a tree; any-order float32 summation of n_con non-negative
    terms is within (n_con - 1) * 2^-24 of the exact sum, relatively, to first order.  Twice that — 2 * n_con * 2^-24 — is
    the band around eps inside which a kernel's sum may fall on the other side: at most 2 % of a set may come that close on
    any sweep (measured: none, at twice the width too)."""
    bits, ok, iters, band = sets.ref(s)
    assert bits.shape == (S.FRAMES, sets.H[s.code].shape[1]) and ok.all()
    early, late = int((iters < s.budget).sum()), int((iters == s.budget).sum())
    width = sets.band(s.code)
    banded, banded2 = int((band < width).sum()), int((band < 2 * width).sum())
    print("band census %s: n_con %d, width %.3g, %d frames early, %d at the limit, banded %d (at twice the width %d), closest %.3g"
          % (s, len(sets.problem(s.code)[3]), width, early, late, banded, banded2, band.min()))
    assert early > 0 and late > 0, (early, late)
    assert banded <= 0.02 * S.FRAMES
    assert sets.clear(s, band).sum() == S.FRAMES - banded


# what each mutant changes, and whether a frame can show it
VISIBLE = ("reversed_terms", "inv_from_f32", "divide", "q_in_f32")


@pytest.mark.parametrize("mutant", VISIBLE)
def test_mutants_are_visible_on_the_sensitive_sets(sets, mutant):
    """one operation of the float32 sweep changed — the v-update's terms in reverse order, inv rounded from a float32
    computation, B / (1 / inv) for B * inv, q formed in float32 — changes a word or a sweep count on EACH sensitive set, so
    a kernel with that difference fails every GPU case that runs on one of them"""
    for s in S.SENSITIVE:
        true = sets.ref(s)
        wrong = sets.ref(s, mutant=mutant)
        words = int((true[0] != wrong[0]).any(axis=1).sum())
        sweeps = int((true[2] != wrong[2]).sum())
        print("mutant %s on %s: %d words, %d sweep counts differ" % (mutant, s, words, sweeps))
        assert words + sweeps > 0, (mutant, s)


def test_fused_term_is_the_same_number():
    """A fused mu * (z - b) + yl (one rounding) cannot be seen on any frame because it is no change at all: z and
    yl are the positive and the negative part of one number, so one of them is zero, and b is 0 or 2.  With yl = 0 the fused
    and the separate form both round mu * (z - b) once; with z = 0 the product mu * (0 - b) is 0 or -2 * mu, exact in any
    binary format, and both forms round yl - 2 * mu once.  Shown here on random states and end to end; it is why removing
    -ffp-contract=off can move nothing but the residual sum, which stays inside the band."""
    rng = np.random.default_rng(1)
    w = (rng.standard_normal(200000) * np.exp(rng.uniform(-20, 3, 200000))).astype(np.float32)
    z, yl = np.maximum(w, np.float32(0)), np.maximum(-w, np.float32(0))
    for mu in (0.5, 0.55, 1.0, 0.3, 0.95):
        m = np.float32(mu)
        for b in (np.float32(0), np.float32(2)):
            plain = yl + m * (z - b)
            fused = (np.float64(m) * (z - b).astype(np.float64) + yl.astype(np.float64)).astype(np.float32)
            assert plain.dtype == np.float32 and (plain == fused).all(), (mu, b)


def test_fused_term_end_to_end(sets):
    for s in S.SENSITIVE:
        assert same(sets.ref(s), sets.ref(s, mutant="fused_term")), s


def test_a_wrong_sign_is_visible_on_every_set(sets):
    """a structural error — the coefficient of one entry of one variable's list negated — shows on every set, the ones
    that forget rounding differences included"""
    for s in S.EARLY_EXIT_SETS:
        col_ptr, con, coef, b = sets.problem(s.code)
        bad = coef.copy()
        bad[col_ptr[len(col_ptr) // 2]] *= -1
        y = sets.frames(s.code, s.snr)[1]
        wrong = admm_ref.qpadmm_ref(sets.H[s.code], y, s.snr, s.alpha, s.mu, s.budget, s.eps, np.float32,
                                    problem=(col_ptr, con, bad, b))
        true = sets.ref(s)
        assert not same(true, wrong), s


def test_distance_between_float32_and_float64(oracle, sets):
    """information for DESIGN.md section 2, no assertion on the counts: how far the float32 sweep is from the float64 one"""
    for s in S.EARLY_EXIT_SETS:
        y = sets.frames(s.code, s.snr)[1]
        ob, ook, oit = oracle.qpadmm_decode(sets.H[s.code], y, s.snr, s.alpha, s.mu, s.budget, s.eps, threads=4)
        bits, ok, iters, _ = sets.ref(s)
        print("fp32 vs fp64 %s: %d of %d frames another word, %d another sweep count"
              % (s, int((bits != ob).any(axis=1).sum()), S.FRAMES, int((iters != oit).sum())))
        assert (ok == ook).all()
