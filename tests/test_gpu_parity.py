"""GPU parity tests proper: the HIP path (through the C ABI) against the oracle and the golden fixtures
captured from the real reference.  Run with `-m gpu` on an MI355X."""
import os

import numpy as np
import pytest

from golden_util import ADMM_ITERS, BP_ITERS, MATS, SNRS, known, load, unpack

pytestmark = pytest.mark.gpu
DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data")


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


@pytest.fixture(scope="module")
def pcm(A, matrices):
    return {k: A.ParityCheckMatrix(v) for k, v in matrices.items()}


# ---------------------------------------------------------------------------------------- phi
def test_phi_device_vs_long_double(A):
    import ctypes as C
    x = np.concatenate([np.logspace(-30, np.log10(45.7), 4000), np.array([0.0, 45.8, 60.0, np.inf, np.nan, 0.25, 2.0])])
    x32 = x.astype(np.float32)
    out = np.zeros_like(x32)
    assert A.lib().acg_ldpc_debug_phi(x32.ctypes.data, out.ctypes.data, len(x32), 0) == 0
    def phi_true(xl):
        # mathematically exact phi in long double.  (The reference's own -logl(tanhl(x/2)) is quantised to
        # multiples of 2^-64 above x ~ 38 because tanhl rounds towards 1; 2*atanh(e^-x) is used there.)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            t = np.exp(-xl)
            return np.where(xl < 1, -np.log(np.tanh(xl / 2)), np.log1p(2 * t / (1 - t)))
    xl = x32.astype(np.longdouble)
    ref = phi_true(xl)
    fin = np.isfinite(ref) & (x32 < 45.7) & (x32 > 0)
    rel = np.abs(out[fin].astype(np.longdouble) - ref[fin]) / np.abs(ref[fin])
    # fp32 tolerance on the soft function; x*|d phi/dx| amplification of the exp argument for large x
    assert rel.max() < 2e-5, rel.max()
    assert np.median(rel) < 2e-7
    assert out[x32 == 0][0] == np.inf          # phi(0) = +inf   (bp.h:34)
    assert (out[x32 >= 45.7477] == 0).all()   # long-double saturation point of the reference
    assert np.isnan(out[np.isnan(x32)]).all()
    # fp64 variant
    o64 = np.zeros_like(x)
    assert A.lib().acg_ldpc_debug_phi(x.ctypes.data, o64.ctypes.data, len(x), 1) == 0
    fin = np.isfinite(ref) & (x < 45.7) & (x > 0)
    ref64 = phi_true(x.astype(np.longdouble))
    rel = np.abs(o64[fin] - ref64[fin]) / np.abs(ref64[fin])
    assert rel.max() < 1e-12


# ---------------------------------------------------------------------------------------- BP
@pytest.mark.parametrize("name", MATS)
@pytest.mark.parametrize("snr", SNRS)
def test_bp_golden_hard_decisions(A, pcm, name, snr):
    """bit-exact bits + flag vs the real reference at every fixture iteration count"""
    g = load(name, snr)
    H = pcm[name]
    for it in BP_ITERS:
        dec = A.BeliefPropagationDecoder(it)
        bits, ok, iters = dec.decode_batch(H, g["y"], snr)
        assert (ok == g["bp%d_ok" % it]).all(), (name, snr, it)
        assert (bits == unpack(g["bp%d_bits" % it], H.n)).all(), (name, snr, it)
        dec.close()


@pytest.mark.parametrize("lpf", [16, 32, 64])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_bp_vs_oracle_2000_frames(A, oracle, matrices, pcm, lpf, prec):
    from acg_alp_ldpc_amd import _lib
    Hm, H = matrices["H05"], pcm["H05"]
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 4242, 2000)
    for snr in (-2.5, -1.0, 3.0):
        y = oracle.transmit_frames(cws, snr, first_seed=100000)
        ob, ook, oit = oracle.bp_decode(Hm, y, snr, 50, threads=8)
        dec = A.BeliefPropagationDecoder(50, lanes_per_frame=lpf,
                                         precision=_lib.PREC_F64 if prec == "f64" else _lib.PREC_DEFAULT)
        bits, ok, iters = dec.decode_batch(H, y, snr)
        dec.close()
        assert (ok == ook).all(), (snr, int((ok != ook).sum()))
        assert (bits == ob).all()
        assert (iters == oit).all()


def test_bp_fixed_work_equals_early_exit(A, oracle, matrices, pcm):
    Hm, H = matrices["optimalH"], pcm["optimalH"]
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 1, 700)
    y = oracle.transmit_frames(cws, -2.0, first_seed=1)
    a = A.BeliefPropagationDecoder(50, early_exit=True)
    b = A.BeliefPropagationDecoder(50, early_exit=False)
    ra, rb = a.decode_batch(H, y, -2.0), b.decode_batch(H, y, -2.0)
    for x, z in zip(ra, rb):
        assert (x == z).all()


def test_bp_edge_cases(A, oracle):
    # ragged degrees incl. degree-1 check (phi(0)=inf message), degree-0 variable, empty check row
    H = np.zeros((5, 9), np.uint8)
    H[0, [0, 1, 2, 3]] = 1
    H[1, [2, 3, 4]] = 1
    H[2, [5]] = 1          # degree-1 check pins variable 5 to 0
    H[3, [0, 6]] = 1       # degree-2 check
    # row 4 empty; column 7, 8 isolated
    rng = np.random.default_rng(3)
    y = 1.0 + 0.9 * rng.standard_normal((300, 9))
    ob, ook, oit = oracle.bp_decode(H, y, 0.0, 12, threads=2)
    dec = A.BeliefPropagationDecoder(12)
    bits, ok, iters = dec.decode_batch(H, y, 0.0)
    assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all()
    # empty batch
    b0, o0, i0 = dec.decode_batch(H, np.zeros((0, 9)), 0.0)
    assert b0.shape == (0, 9) and o0.shape == (0,)
    # single-frame reference signature: failure returns an empty word (bp.h:198)
    ybad = -np.ones(9)
    ybad[5] = 3.0
    word, flag = dec.decode(H, y[0], 0.0)
    assert flag == bool(ook[0]) and (not flag or (word == ob[0]).all())
    assert dec.name() == "BP"


def test_bp_infinite_messages_high_snr(A, oracle, matrices, pcm):
    # +4..+8 dB: LLR magnitudes saturate phi; flags/bits must still agree
    Hm, H = matrices["H05"], pcm["H05"]
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 9, 1500)
    for snr in (4.0, 8.0):
        y = oracle.transmit_frames(cws, snr, first_seed=777)
        ob, ook, oit = oracle.bp_decode(Hm, y, snr, 50, threads=8)
        dec = A.BeliefPropagationDecoder(50)
        bits, ok, iters = dec.decode_batch(H, y, snr)
        assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all()


# ---------------------------------------------------------------------------------------- QP-ADMM
@pytest.mark.parametrize("name", MATS)
@pytest.mark.parametrize("snr", SNRS)
def test_qpadmm_golden_hard_decisions(A, pcm, name, snr):
    g = load(name, snr)
    H = pcm[name]
    alpha, mu = g["admm_alpha_mu"]
    for it in ADMM_ITERS:
        for tag, eps in (("e0", 0.0), ("e5", 1e-5)):
            dec = A.QPADMMDecoder(alpha, mu, it, eps)
            bits, ok, iters = dec.decode_batch(H, g["y"], snr)
            dec.close()
            assert (ok == g["admm%d_%s_ok" % (it, tag)]).all()
            assert (bits == unpack(g["admm%d_%s_bits" % (it, tag)], H.n)).all(), (name, snr, it, tag)


@pytest.mark.parametrize("lpf", [0, 16, 32, 64])   # 0 = auto = one 256-thread workgroup per frame
def test_qpadmm_vs_oracle_iters(A, oracle, matrices, pcm, lpf):
    Hm, H = matrices["H05"], pcm["H05"]
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 11, 1000)
    y = oracle.transmit_frames(cws, -2.0, first_seed=31337)
    ob, ook, oit = oracle.qpadmm_decode(Hm, y, -2.0, 1.95, 0.5, 100, 1e-5, threads=8)
    dec = A.QPADMMDecoder(1.95, 0.5, 100, 1e-5, lanes_per_frame=lpf)
    bits, ok, iters = dec.decode_batch(H, y, -2.0)
    assert (ok == ook).all() and (bits == ob).all()
    assert (iters == oit).all()   # same sweep count: the residual test fires on the same sweep
    assert dec.name() == "QP-ADMM"


@pytest.mark.parametrize("name,alpha,mu", [("H05", 1.95, 0.5), ("optimalH", 1.2, 0.55)])
def test_qpadmm_100k_frames_bits_and_sweep_counts(A, oracle, matrices, pcm, name, alpha, mu):
    """the workgroup-per-frame kernel at volume: 100 000 frames over two SNRs, up to 200 sweeps, the reference's
    parameters for each matrix (main.cpp:31,33) — fp64 hard decisions and the sweep at which the residual rule fires
    (qp_admm.h:158-163) equal to the restatement on every frame"""
    Hm, H = matrices[name], pcm[name]
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 23, 50000)
    for snr, seed0 in ((-2.0, 500000), (1.0, 900000)):
        y = oracle.transmit_frames(cws, snr, first_seed=seed0)
        ob, ook, oit = oracle.qpadmm_decode(Hm, y, snr, alpha, mu, 200, 1e-5, threads=16)
        dec = A.QPADMMDecoder(alpha, mu, 200, 1e-5)
        bits, ok, iters = dec.decode_batch(H, y, snr)
        dec.close()
        assert (ok == ook).all() and (bits == ob).all(), (name, snr, int((bits != ob).any(axis=1).sum()))
        assert (iters == oit).all(), (name, snr, int((iters != oit).sum()))


@pytest.mark.parametrize("force_l", [128, 192, 256])
def test_qpadmm_workgroup_sizes_and_pass_instances(A, oracle, matrices, pcm, force_l):
    """the three workgroup sizes of the workgroup-per-frame QP-ADMM kernel (and with them its 2-, 3- and 4-pass
    instances: H.txt needs 2-4 passes, H05 3-4) give the reference's bits and sweep counts"""
    os.environ["ACG_ADMM_BLOCK_L"] = str(force_l)
    try:
        for name, alpha, mu in (("H", 1.9, 0.5), ("H05", 1.95, 0.5)):
            Hm, H = matrices[name], pcm[name]
            G, _ = oracle.get_orthogonal(Hm)
            cws = oracle.gen_codewords(G, 77, 1500)
            y = oracle.transmit_frames(cws, -1.5, first_seed=4242)
            ob, ook, oit = oracle.qpadmm_decode(Hm, y, -1.5, alpha, mu, 150, 1e-5, threads=8)
            dec = A.QPADMMDecoder(alpha, mu, 150, 1e-5)
            bits, ok, iters = dec.decode_batch(H, y, -1.5)
            lay = dec.layout(H)
            dec.close()
            assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all(), (name, lay)
            if name == "H05" and force_l != 128:     # 541 group slots need 5 passes of 128: that size is skipped
                assert lay["lanes_per_frame"] == force_l, lay
    finally:
        del os.environ["ACG_ADMM_BLOCK_L"]


def test_qpadmm_guard_and_small_checks(A, oracle, matrices, pcm):
    dec = A.QPADMMDecoder(2.0, 0.5, 10)          # e_min*mu = 2 <= alpha -> (zeros,false), qp_admm.h:112-114
    y = np.ones((5, pcm["H05"].n))
    bits, ok, iters = dec.decode_batch(pcm["H05"], y, 0.0)
    assert not ok.any() and not bits.any()
    # degree-1 / degree-2 checks (qp_admm.h:70-83) and an empty row
    H = np.zeros((5, 8), np.uint8)
    H[0, [0, 1, 2, 3, 4]] = 1
    H[1, [2, 5]] = 1
    H[2, [6]] = 1
    H[3, [1, 3, 7]] = 1
    H[4, [0, 7]] = 1
    rng = np.random.default_rng(5)
    y = 1.0 + 0.8 * rng.standard_normal((200, 8))
    ob, ook, oit = oracle.qpadmm_decode(H, y, 1.0, 0.6, 1.0, 80, 1e-6, threads=2)
    dec = A.QPADMMDecoder(0.6, 1.0, 80, 1e-6)
    bits, ok, iters = dec.decode_batch(H, y, 1.0)
    assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all()
    # sweep budgets 0 and 1.  Budget 0: the reference returns its initial guess v = (q > 0), qp_admm.h:116-119,166-175
    # (the complement of the channel hard decision), ok = true; zero / -0 / NaN symbols give q > 0 false -> bit 0
    y0 = y.copy()
    y0[0, :4] = [0.0, -0.0, np.nan, 1e-320]
    for budget in (0, 1):
        ob, ook, oit = oracle.qpadmm_decode(H, y0, 1.0, 0.6, 1.0, budget, 1e-6, threads=2)
        if budget == 0:
            assert ook.all() and (ob == (2 * y0 / A.llr_variance(1.0) > 0)).all() and not oit.any()
        for lpf in (0, 64):
            for prec in (A.PREC_DEFAULT, A.PREC_F32) if budget == 0 else (A.PREC_DEFAULT,):
                dec = A.QPADMMDecoder(0.6, 1.0, budget, 1e-6, lanes_per_frame=lpf, precision=prec)
                bits, ok, iters = dec.decode_batch(H, y0, 1.0)
                dec.close()
                if prec == A.PREC_F32:   # fp32 q: the denormal symbol underflows to q = 0 -> bit 0; everything else as fp64
                    ob32 = ob.copy()
                    ob32[0, 3] = 0
                    assert (ok == ook).all() and (bits == ob32).all() and (iters == oit).all(), (budget, lpf, "f32")
                else:
                    assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all(), (budget, lpf)
    # budget 0 on H05 through the Monte-Carlo loop: every frame "decodes" to the complement of its hard decision
    H5, Hb = pcm["H05"], matrices["H05"]
    yb = 1.0 + 0.9 * rng.standard_normal((64, H5.n))
    ob, ook, oit = oracle.qpadmm_decode(Hb, yb, -1.0, 1.95, 0.5, 0, 1e-5, threads=2)
    dec = A.QPADMMDecoder(1.95, 0.5, 0, 1e-5)
    bits, ok, iters = dec.decode_batch(H5, yb, -1.0)
    assert (ok == ook).all() and (bits == ob).all() and not iters.any()
    r = A.run_experiment(dec, None, H5, 3.0, frames=2000, noise="device", seed=3)
    dec.close()
    assert r.total == 2000 and r.correct == 0 and r.sum_iters == 0   # all-zero word sent, (q > 0) is almost all ones


def test_qpadmm_mixed_check_degrees_and_long_lists(A, oracle):
    """workgroup-per-frame QP-ADMM beyond H05's shape: several passes and wavefronts, one- and two-variable checks
    mixed with long ones (the GENERIC group instance next to the common one), variables in more checks than the
    register-resident list holds (tail read from the table).  fp64: bits, flag and
    sweep counts identical to the reference restatement (qp_admm.h:13-178)."""
    rng = np.random.default_rng(11)
    m, n = 230, 400
    H = np.zeros((m, n), np.uint8)
    degs = rng.choice([1, 2, 3, 4, 5, 6, 8], size=m, p=[0.08, 0.12, 0.2, 0.2, 0.2, 0.1, 0.1])
    for i, d in enumerate(degs):
        H[i, rng.choice(n, size=d, replace=False)] = 1
    H[:9, 3] = 1                                                  # a variable in >= 9 checks (list longer than 6)
    H[20:32, 5] = 1
    for v in np.nonzero(H.sum(0) == 0)[0]:                        # an isolated variable has e = 0 and trips the guard
        H[rng.integers(40, m), v] = 1                             # (qp_admm.h:108-114), tested elsewhere
    cw = np.zeros((300, n), np.uint8)
    y = (1.0 - 2.0 * cw) + 0.7 * rng.standard_normal((300, n))
    ob, ook, oit = oracle.qpadmm_decode(H, y, 1.0, 0.6, 1.0, 60, 1e-6, threads=4)
    for lpf in (0, 64):
        dec = A.QPADMMDecoder(0.6, 1.0, 60, 1e-6, lanes_per_frame=lpf)
        bits, ok, iters = dec.decode_batch(H, y, 1.0)
        lay = dec.layout(H)
        dec.close()
        assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all(), (lpf, lay)
        if lpf == 0:
            assert lay["lanes_per_frame"] in (128, 192, 256), lay   # the workgroup-per-frame kernel took it
    assert 1 < oit.mean() < 60                                      # the stopping rule was exercised both ways


def test_qpadmm_fp32_fer_only(A, oracle, matrices, pcm):
    """fp32 QP-ADMM: FER-level agreement only (the 1/(mu*e-alpha)=20x gain amplifies rounding)
    (against the fp64 oracle; tests/test_admm_f32_exact_gpu.py holds the fp32 kernels to their float32 restatement, frame by frame)"""
    from acg_alp_ldpc_amd import _lib
    Hm, H = matrices["optimalH"], pcm["optimalH"]
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 3, 1000)
    y = oracle.transmit_frames(cws, -2.0, first_seed=1)
    ob, _, _ = oracle.qpadmm_decode(Hm, y, -2.0, 1.2, 0.55, 100, 1e-5, threads=8)
    dec = A.QPADMMDecoder(1.2, 0.55, 100, 1e-5, precision=_lib.PREC_F32)
    bits, ok, _ = dec.decode_batch(H, y, -2.0)
    good_o = (ob == cws).all(axis=1).mean()
    good_g = (bits == cws).all(axis=1).mean()
    assert abs(good_o - good_g) < 0.03


# ---------------------------------------------------------------------------------------- min-sum (unpinned)
def test_minsum_against_own_restatement(A, oracle, matrices, pcm):
    """parity unpinned (no min-sum in the reference): checked against the repo's own fp64
    restatement; fp32 vs fp64 may differ on knife-edge frames, so agreement is asked at 99.5%."""
    Hm, H = matrices["H05"], pcm["H05"]
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 5, 2000)
    for scale in (1.0, 0.75):
        y = oracle.transmit_frames(cws, -1.0, first_seed=99)
        ob, ook, oit = oracle.minsum_decode(Hm, y, -1.0, 50, scale, threads=8)
        dec = A.MinSumDecoder(50, scale)
        bits, ok, iters = dec.decode_batch(H, y, -1.0)
        agree = ((ok == ook) & (bits == ob).all(axis=1)).mean()
        assert agree >= 0.995, agree
        from acg_alp_ldpc_amd import _lib
        dec64 = A.MinSumDecoder(50, scale, precision=_lib.PREC_F64)
        bits, ok, iters = dec64.decode_batch(H, y, -1.0)
        assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all()


# ---------------------------------------------------------------------------------------- Monte-Carlo
@pytest.mark.parametrize("idx", [0, 2, 3, 6, 7, 10, 12])
def test_mc_host_noise_known_answers(A, matrices, pcm, idx):
    """experiment.h loop with the reference's exact frames (mt19937(i+1)): counts identical to the
    single-threaded reference run recorded in tests/golden/known_answers.json"""
    e = known()["experiments"][idx]
    H = pcm[e["matrix"]]
    if e["codewords"].startswith("G05"):
        from oracle.pyoracle import Oracle
        G = Oracle().read_pcm(os.path.join(DATA, "G05.txt"))
    else:
        G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 1000, 239239239)
    if e["kind"] == "bp":
        dec = A.BeliefPropagationDecoder(e["max_iter"])
    else:
        dec = A.QPADMMDecoder(e["alpha"], e["mu"], e["max_iter"], 1e-5)
    r = A.run_experiment(dec, cws, H, e["snr"], noise="host")
    for k in ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong"):
        assert getattr(r, k) == e[k], (k, r, e)


def test_mc_device_noise_statistics(A, matrices, pcm):
    """Philox AWGN through the Monte-Carlo loop (the generator itself is pinned sample for sample in test_awgn_exact_gpu.py):
    raw BER = Q(1/sigma), FER inside the 99% binomial interval around the reference's 1000-frame estimate, shard-count
    invariance."""
    from math import erfc, sqrt
    H = pcm["H05"]
    G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 4096, 239239239)
    dec = A.BeliefPropagationDecoder(50)
    F = 200000
    snr = -2.0
    r = A.run_experiment(dec, cws, H, snr, frames=F, noise="device", seed=12345)
    assert r.total == F
    sigma = sqrt(A.llr_variance(snr))
    ber = 0.5 * erfc(1 / sigma / sqrt(2))
    assert abs(r.mean_hamming() / H.n - ber) < 4 * sqrt(ber * (1 - ber) / (F * H.n))
    p_ref = 1 - 915 / 1000.0   # known_answers: H05 BP-50 @ -2 dB
    half = 2.576 * sqrt(p_ref * (1 - p_ref) / 1000) + 2.576 * sqrt(p_ref * (1 - p_ref) / F)
    assert abs(r.FER() - p_ref) < half, (r.FER(), p_ref)
    # same global frames in 1 shard or 3 shards
    parts = [A.run_experiment(dec, cws, H, snr, frames=c, first_frame=lo, noise="device", seed=12345)
             for lo, c in (A.shard_range(F, k, 3) for k in range(3))]
    tot = parts[0]
    for p in parts[1:]:
        A.merge_exp_results(tot, p)
    assert (tot.as_vector() == r.as_vector()).all()
    # QP-ADMM through the same loop
    adm = A.QPADMMDecoder(1.95, 0.5, 100, 1e-5)
    ra = A.run_experiment(adm, cws, H, snr, frames=20000, noise="device", seed=5)
    p_ref = 1 - 660 / 1000.0
    assert abs(ra.FER() - p_ref) < 2.576 * sqrt(p_ref * (1 - p_ref) / 1000) + 0.01, ra.FER()


def test_awgn_dev_matches_mc_frames(A, pcm):
    """the standalone AWGN generator and the in-kernel one produce the same frames (same Philox keys):
    decoding the generated y through decode_batch_dev gives the same counters as the MC kernel."""
    import ctypes as C
    import torch
    from acg_alp_ldpc_amd._lib import McCfg, check, lib
    H = pcm["H05"]
    G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 512, 1)
    dec = A.BeliefPropagationDecoder(50)
    F, snr = 8192, -1.5
    h, _ = dec.handle(H)
    cfg = McCfg()
    cfg.frames, cfg.first_frame, cfg.snr, cfg.seed, cfg.noise = F, 1000, snr, 99, 0
    cfg.codewords, cfg.n_codewords = cws.ctypes.data, cws.shape[0]
    y = torch.empty((F, H.n), dtype=torch.float32, device="cuda")
    check(lib().acg_ldpc_awgn_dev(h, C.byref(cfg), y.data_ptr(), None))
    dec.sync(H)
    nw = (H.n + 31) // 32
    bits = torch.zeros((F, nw), dtype=torch.int32, device="cuda")
    ok = torch.zeros(F, dtype=torch.uint8, device="cuda")
    it = torch.zeros(F, dtype=torch.int32, device="cuda")
    dec.decode_batch_dev(H, y.data_ptr(), False, F, snr, bits.data_ptr(), ok.data_ptr(), it.data_ptr())
    dec.sync(H)
    r = A.run_experiment(dec, cws, H, snr, frames=F, first_frame=1000, noise="device", seed=99)
    okh = ok.cpu().numpy()
    assert int(it.sum().item()) == r.sum_iters
    assert int(okh.sum()) == r.correct + r.pseudo
    ysum = float(y.double().mean().item())
    assert abs(ysum - float((1 - 2 * cws.astype(np.float64)).mean())) < 0.02


# ---------------------------------------------------------------------------------------- full-size properties
def test_full_size_round_trip_properties(A, pcm):
    """BASELINE config-2 size (1M frames) through size-independent properties: encode -> AWGN -> decode
    returns the sent word whenever ok, every returned word has zero syndrome, totals add up."""
    H = pcm["H05"]
    G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 8192, 2024)
    dec = A.BeliefPropagationDecoder(50)
    F = 1 << 20
    r = A.run_experiment(dec, cws, H, 2.0, frames=F, noise="device", seed=1)
    assert r.total == F and r.correct + r.pseudo <= F
    assert r.sum_hamming == r.sum_hamming_ok + r.sum_hamming_wrong
    assert r.FER() < 1e-3               # +2 dB: reference FER is 0/1000
    assert r.pseudo <= 5
    r0 = A.run_experiment(dec, None, H, 2.0, frames=F, noise="device", seed=1)  # all-zero codeword
    assert r0.total == F and abs(r0.FER() - r.FER()) < 1e-3  # decoder symmetry


# ---------------------------------------------------------------------------------------- streamed (HBM) engine
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_streamed_engine_equals_oracle(A, oracle, matrices, pcm, prec):
    """the one-lane-per-frame HBM engine must give the same bits / flags / exit iterations as the oracle"""
    Hm, H = matrices["H05"], pcm["H05"]
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 21, 1500)
    for snr in (-2.0, 1.0):
        y = oracle.transmit_frames(cws, snr, first_seed=4000)
        ob, ook, oit = oracle.bp_decode(Hm, y, snr, 50, threads=8)
        for ee in (True, False):
            dec = A.BeliefPropagationDecoder(50, engine=A.ENGINE_STREAMED, early_exit=ee,
                                             precision=A.PREC_F64 if prec == "f64" else A.PREC_DEFAULT)
            bits, ok, iters = dec.decode_batch(H, y, snr)
            assert dec.layout(H)["lanes_per_frame"] == 1
            dec.close()
            assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all(), (snr, ee)
    # ragged batch (not a multiple of 64) and min-sum
    y = oracle.transmit_frames(cws[:77], 0.0, first_seed=9)
    ob, ook, oit = oracle.minsum_decode(Hm, y, 0.0, 30, 0.75, threads=4)
    dec = A.MinSumDecoder(30, 0.75, engine=A.ENGINE_STREAMED, precision=A.PREC_F64)
    bits, ok, iters = dec.decode_batch(H, y, 0.0)
    assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all()


def test_streamed_mc_matches_fused_mc(A, pcm):
    """same Philox frames through both engines -> identical Monte-Carlo counters"""
    H = pcm["optimalH"]
    G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 777, 5)
    a = A.BeliefPropagationDecoder(50, engine=A.ENGINE_FUSED)
    b = A.BeliefPropagationDecoder(50, engine=A.ENGINE_STREAMED)
    ra = A.run_experiment(a, cws, H, -1.5, frames=30000, first_frame=123, noise="device", seed=4)
    rb = A.run_experiment(b, cws, H, -1.5, frames=30000, first_frame=123, noise="device", seed=4)
    assert (ra.as_vector() == rb.as_vector()).all(), (ra, rb)


def test_config5_synthetic_regular_code(A, oracle):
    """BASELINE configs[4]: synthetic (3,6)-regular 5000 x 10000, min-sum 50 iterations.  fp64 does not fit in LDS
    (auto -> streamed engine); fp32 does, with one 1024-thread workgroup per frame.
    Oracle comparison on a few frames, size-independent properties on a larger batch."""
    Hm = A.regular_ldpc(5000, 10000, 3, 6, seed=1)
    H = A.ParityCheckMatrix(Hm)
    assert (H.m, H.n, H.E) == (5000, 10000, 30000)
    rng = np.random.default_rng(0)
    snr = 2.0
    sigma = np.sqrt(A.llr_variance(snr))
    y = 1.0 + sigma * rng.standard_normal((12, 10000))      # all-zero codeword
    ob, ook, oit = oracle.minsum_decode(Hm, y, snr, 50, 0.75, threads=8)
    ob1, ook1, oit1 = ob, ook, oit
    dec64 = A.MinSumDecoder(50, 0.75, precision=A.PREC_F64)
    bits, ok, iters = dec64.decode_batch(H, y, snr)
    assert dec64.layout(H)["lanes_per_frame"] == 1            # streamed engine chosen automatically
    assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all()
    dec64.close()
    # sum-product on the big code too
    ob, ook, oit = oracle.bp_decode(Hm, y[:6], snr, 50, threads=6)
    spa = A.BeliefPropagationDecoder(50)
    bits, ok, iters = spa.decode_batch(H, y[:6], snr)
    assert spa.layout(H)["lanes_per_frame"] == 1024       # fused, one workgroup per frame (120 KB of messages in LDS)
    assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all()
    spa.close()
    sps = A.BeliefPropagationDecoder(50, engine=A.ENGINE_STREAMED)
    bits, ok, iters = sps.decode_batch(H, y[:6], snr)
    assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all()
    sps.close()
    # the configs[4] HEADLINE kernel — fp32 min-sum, one 1024-thread workgroup per frame (bp_block_kernel, index table in
    # registers) — against the oracle's min-sum restatement.  Min-sum is parity-unpinned and fp32 may part
    # from the fp64 restatement on knife-edge frames, so the bar is an agreement RATE: word and flag equal on at least
    # 23 of 24 frames, exit iteration equal too on at least 20; 12 frames at +2 dB and 12 at the threshold (-1.6 dB:
    # exits after 21-42 sweeps, two frames never).
    sig2 = np.sqrt(A.llr_variance(-1.6))
    y2 = 1.0 + sig2 * np.random.default_rng(1).standard_normal((12, 10000))
    ob2, ook2, oit2 = oracle.minsum_decode(Hm, y2, -1.6, 50, 0.75, threads=8)
    for ee in (True, False):
        ms = A.MinSumDecoder(50, 0.75, early_exit=ee)
        assert ms.layout(H)["lanes_per_frame"] == 1024
        b1, k1, i1 = ms.decode_batch(H, y, snr)
        b2, k2, i2 = ms.decode_batch(H, y2, -1.6)
        ms.close()
        same = np.concatenate([(k1 == ook1) & (b1 == ob1).all(axis=1), (k2 == ook2) & (b2 == ob2).all(axis=1)])
        same_it = np.concatenate([i1 == oit1, i2 == oit2])
        assert same.sum() >= 23 and (same & same_it).sum() >= 20, (ee, int(same.sum()), int((same & same_it).sum()))
    assert ook1.all() and not ook2.all() and oit2[ook2 == 1].max() > 30     # the second set really sits at the threshold
    dec = A.MinSumDecoder(50, 0.75, early_exit=False)
    r = A.run_experiment(dec, None, H, snr, frames=4096, noise="device", seed=3)
    assert r.total == 4096 and r.pseudo == 0 and r.correct >= 4090, r
    assert r.sum_hamming == r.sum_hamming_ok + r.sum_hamming_wrong


def test_pair_f16_minsum_kernels(A, oracle):
    """precision = PREC_F16: two frames per workgroup, packed half-precision min-sum messages (bp_pair.hip).  Min-sum is
    not in the reference (parity unpinned) and half precision moves knife-edge frames, so the bar is the one of
    the fp32 min-sum kernels, loosened to what 10-bit magnitudes allow: at a comfortable SNR every frame decodes to the
    oracle's word (exit iteration within 2 sweeps); near the threshold the FER stays within 0.06 of the fp32 kernel's;
    ragged batches (odd frame counts), both workgroup sizes, regular and irregular codes; sum-product / QP-ADMM refuse
    the precision."""
    # (a) BASELINE configs[4] code: regular instance, 1024 threads per frame pair
    Hm = A.regular_ldpc(5000, 10000, 3, 6, seed=1)
    H = A.ParityCheckMatrix(Hm)
    rng = np.random.default_rng(3)
    snr = 2.0
    y = 1.0 + np.sqrt(A.llr_variance(snr)) * rng.standard_normal((13, 10000))      # odd count: the last pair is half empty
    ob, ook, oit = oracle.minsum_decode(Hm, y, snr, 50, 0.75, threads=8)
    for ee in (True, False):
        dec = A.MinSumDecoder(50, 0.75, precision=A.PREC_F16, early_exit=ee)
        assert dec.layout(H) == dict(dec.layout(H), lanes_per_frame=1024, frames_per_block=2)
        bits, ok, it = dec.decode_batch(H, y, snr)
        assert (ok == ook).all() and (bits == ob).all() and np.abs(it - oit).max() <= 2, (ee, it, oit)
        r = A.run_experiment(dec, None, H, snr, frames=2049, noise="device", seed=3)     # AWGN kernel -> decode -> classify
        dec.close()
        assert r.total == 2049 and r.pseudo == 0 and r.correct >= 2046, r
    y2 = 1.0 + np.sqrt(A.llr_variance(-1.6)) * rng.standard_normal((256, 10000))
    fers = []
    for prec in (A.PREC_DEFAULT, A.PREC_F16):
        dec = A.MinSumDecoder(50, 0.75, precision=prec)
        b2, k2, i2 = dec.decode_batch(H, y2, -1.6)
        dec.close()
        assert not b2[k2 == 1].any()                     # whatever converges, converges to the sent (all-zero) word
        fers.append(1 - k2.mean())
    assert 0.02 < fers[0] < 0.9 and abs(fers[0] - fers[1]) < 0.06, fers
    # (b) 256 threads per pair: a regular (3,6) 1500 x 3000 code and an irregular code (variable degree 2..4, check degree 4..8)
    Hr = A.regular_ldpc(1500, 3000, 3, 6, seed=5)
    Hi = np.zeros((300, 600), np.uint8)
    r2 = np.random.default_rng(8)
    for v in range(600):
        Hi[r2.choice(300, size=2 + (v % 3), replace=False), v] = 1
    Hi = Hi[(Hi.sum(1) >= 2)]
    for Hx in (Hr, Hi):
        if Hx.sum(1).max() > 8:
            Hx = Hx.copy()
            for i in np.nonzero(Hx.sum(1) > 8)[0]:
                Hx[i, np.nonzero(Hx[i])[0][8:]] = 0
        Hc = A.ParityCheckMatrix(Hx)
        yy = 1.0 + np.sqrt(A.llr_variance(4.0)) * rng.standard_normal((41, Hc.n))
        ob, ook, oit = oracle.minsum_decode(Hx, yy, 4.0, 30, 0.75, threads=4)
        dec = A.MinSumDecoder(30, 0.75, precision=A.PREC_F16)
        assert dec.layout(Hc)["lanes_per_frame"] == 256
        bits, ok, it = dec.decode_batch(Hc, yy, 4.0)
        dec.close()
        same = (ok == ook) & (bits == ob).all(axis=1)
        assert same.mean() >= 0.95 and np.abs(it - oit)[same].max() <= 2, (same.mean(), Hc.m, Hc.n)
    # (c) only min-sum has the half-precision variant
    with pytest.raises(A.LdpcError):
        A.BeliefPropagationDecoder(10, precision=A.PREC_F16).decode_batch(H, y[:1], snr)
    with pytest.raises(A.LdpcError):
        A.QPADMMDecoder(0.6, 1.0, 10, precision=A.PREC_F16).decode_batch(H, y[:1], snr)


def test_config5_block_kernel_variants_agree_near_threshold(A, oracle):
    """The workgroup-per-frame instance used for the (3,6) 5000 x 10000 code (index table in registers, syndrome taken
    from the check sweep, bank-conflict placement) against the plain instance (ACG_BP_NO_IDXREG / ACG_BP_NO_PLACEMENT)
    and the HBM-streamed engine, at an SNR where frames exit anywhere between 10 sweeps and never: the three share the
    arithmetic, so bits, flags and exit iterations must be identical; a few frames also against the oracle."""
    Hm = A.regular_ldpc(5000, 10000, 3, 6, seed=1)
    H = A.ParityCheckMatrix(Hm)
    rng = np.random.default_rng(7)
    snr = -1.75        # Es/N0; the (3,6) threshold is about -1.9 dB
    sigma = np.sqrt(A.llr_variance(snr))
    y = 1.0 + sigma * rng.standard_normal((192, 10000))
    for make in (lambda **kw: A.BeliefPropagationDecoder(60, **kw), lambda **kw: A.MinSumDecoder(60, 0.75, **kw)):
        dec = make()
        assert dec.layout(H)["lanes_per_frame"] == 1024
        b0, k0, i0 = dec.decode_batch(H, y, snr)
        dec.close()
        assert 0 < k0.sum() and len(set(i0[k0 == 1].tolist())) > 3      # a spread of exit iterations
        os.environ["ACG_BP_NO_IDXREG"] = "1"
        os.environ["ACG_BP_NO_PLACEMENT"] = "1"
        try:
            dec = make()
            b1, k1, i1 = dec.decode_batch(H, y, snr)
            dec.close()
        finally:
            del os.environ["ACG_BP_NO_IDXREG"], os.environ["ACG_BP_NO_PLACEMENT"]
        assert (k0 == k1).all() and (b0 == b1).all() and (i0 == i1).all()
        dec = make(engine=A.ENGINE_STREAMED)
        b2, k2, i2 = dec.decode_batch(H, y, snr)
        dec.close()
        assert (k0 == k2).all() and (b0 == b2).all() and (i0 == i2).all()
        # the wave-group kernel forced onto this code (one frame per wavefront, 160 KB of LDS): its message array is past the
        # 64 KiB the byte-offset index copy addresses, so this is the instance that reads the index table from memory
        dec = make(lanes_per_frame=64)
        assert dec.layout(H)["lanes_per_frame"] == 64
        b3, k3, i3 = dec.decode_batch(H, y[:48], snr)
        dec.close()
        assert (k0[:48] == k3).all() and (b0[:48] == b3).all() and (i0[:48] == i3).all()
    ob, ook, oit = oracle.bp_decode(Hm, y[:8], snr, 60, threads=8)
    dec = A.BeliefPropagationDecoder(60)
    bits, ok, iters = dec.decode_batch(H, y[:8], snr)
    dec.close()
    assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all()


def test_bp_fp32_knife_edge_frames(A, oracle, matrices, pcm):
    """The three frames of 4 * 10^6 (tools/soak_oracle.py, H05, BP-50, -2 / -1 dB; fixture tests/golden/bp_knife_edges.npz: symbols,
    the restatement's outputs, the fp32 kernels' exit iterations) on which the fp32 kernels reach the zero syndrome at another
    sweep than the 80-bit restatement — 6 vs 8, 18 vs 15, 3 vs 4: a posterior that hovers at zero for a few sweeps has another sign
    in fp32.  The word and the flag are the oracle's on all three; both fp32 engines agree with each other; fp64 messages
    reproduce the oracle's iteration.  (The bar of the parity tests is word + flag exact; the exit iteration of the fp32 engines
    may differ on ~1e-6 of the frames, by up to three sweeps here.)"""
    k = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bp_knife_edges.npz"))
    Hm, H = matrices["H05"], pcm["H05"]
    assert len(k["snr"]) == 3
    for i in range(len(k["snr"])):
        snr, y = float(k["snr"][i]), np.ascontiguousarray(k["y"][i:i + 1])
        want = np.unpackbits(k["oracle_bits"][i])[:H.n]
        ob, ook, oit = oracle.bp_decode(Hm, y, snr, 50)           # the fixture is what the oracle says today
        assert (ob[0] == want).all() and ook[0] == k["oracle_ok"][i] and oit[0] == k["oracle_iters"][i]
        for eng in (A.ENGINE_FUSED, A.ENGINE_STREAMED):
            dec = A.BeliefPropagationDecoder(50, engine=eng)
            bits, ok, iters = dec.decode_batch(H, y, snr)
            dec.close()
            assert (bits[0] == want).all() and ok[0] == ook[0] == 1
            assert iters[0] == k["gpu_fp32_iters"][i] and 1 <= abs(int(iters[0]) - int(oit[0])) <= 3, (i, eng, iters[0], oit[0])
        d64 = A.BeliefPropagationDecoder(50, precision=A.PREC_F64)
        bits, ok, iters = d64.decode_batch(H, y, snr)
        d64.close()
        assert (bits[0] == want).all() and ok[0] == 1 and iters[0] == oit[0]


@pytest.mark.parametrize("engine", ["streamed_ring", "streamed_regs", "fused", "fused_block256"])
@pytest.mark.parametrize("name", MATS)
@pytest.mark.parametrize("snr", [-2.0, 2.0])
def test_bp_soft_messages_vs_reference_trace(A, pcm, name, snr, engine, monkeypatch):
    """SURVEY §8(c) stated tolerance: soft LLR-domain values after iterations 1 and 2 within
    1e-4 * max(1, |x|) of the real reference (fp32) for finite, unsaturated (|x| < 15) values; fp64: 1e-9.
    Every engine has its own sweep code, so each is traced by a debug instance of the kernel that ships:
      streamed_ring   bp_streamed_ring_kernel (RingPass + the counted vmcnt waits; what the fp32 streamed engine runs) — the slab
                      of the first tile copied out of memory
      streamed_regs   bp_streamed_kernel (StreamPass; fp64, and fp32 for node degrees 13-16 that do not fit a ring slot; forced
                      here with ACG_STREAM_NO_RING)
      fused / fused_block256   BpPass wave groups / workgroup-per-frame with the syndrome merged into the check sweep — the
                      message words copied out of LDS."""
    g = load(name, snr)
    H = pcm[name]
    E = H.E
    nf = g["trace1_c2v"].shape[0]
    y = np.ascontiguousarray(g["y"][:nf])
    eng, lpf = {"streamed_ring": (A.ENGINE_STREAMED, 0), "streamed_regs": (A.ENGINE_STREAMED, 0), "fused": (A.ENGINE_FUSED, 0),
                "fused_block256": (A.ENGINE_FUSED, 256)}[engine]
    if engine == "streamed_regs":
        monkeypatch.setenv("ACG_STREAM_NO_RING", "1")
    for f64, tol in (((0, 1e-4),) if engine == "streamed_ring" else ((0, 1e-4), (1, 1e-9))):
        for it in (1, 2):
            c2v, mag, sgn = (np.zeros((nf, E)) for _ in range(3))
            post = np.zeros((nf, H.n))
            rc = A.lib().acg_ldpc_debug_bp_trace(H._h, y.ctypes.data, nf, float(snr), it, f64, eng, lpf, c2v.ctypes.data,
                                                 mag.ctypes.data, sgn.ctypes.data, post.ctypes.data)
            assert rc == 0, A.lib().acg_ldpc_last_error()
            for got, key in ((c2v, "c2v"), (post, "post")):
                ref = g["trace%d_%s" % (it, key)]
                m = np.isfinite(ref) & (np.abs(ref) < 15)
                assert (np.abs(got[m] - ref[m]) <= tol * np.maximum(1.0, np.abs(ref[m]))).all(), (name, snr, it, key, f64)
                # beyond |x| = 15 (outside the SURVEY tolerance band) the values must still agree to 1e-3 relative
                big = np.isfinite(ref) & ~m
                assert (np.abs(got[big] - ref[big]) <= 1e-3 * np.abs(ref[big])).all()
                assert (np.isfinite(got) == np.isfinite(ref)).all()
            refm, refs = g["trace%d_v2c_mag" % it], g["trace%d_v2c_sgn" % it]
            assert (sgn == refs).all()
            m = np.isfinite(refm) & (refm < 15) & (refm > 1e-6)
            assert (np.abs(mag[m] - refm[m]) <= tol * np.maximum(1.0, refm[m])).all()


# ---------------------------------------------------------------------------------------- BASELINE configs 3 and 4 at size
def test_config3_qpadmm_1m_frames_properties(A, pcm):
    """configs[2]: H05 QP-ADMM (1.95, 0.5) 100 sweeps, eps 1e-5, 1M frames on one GPU — size-independent properties
    (counter sums, decoder symmetry, FER inside the 99% interval of the reference's 1000-frame estimate 0.340)."""
    from math import sqrt
    H = pcm["H05"]
    G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 4096, 239239239)
    dec = A.QPADMMDecoder(1.95, 0.5, 100, 1e-5)
    F = 1 << 20
    r = A.run_experiment(dec, cws, H, -2.0, frames=F, noise="device", seed=1)
    assert r.total == F and r.sum_hamming == r.sum_hamming_ok + r.sum_hamming_wrong
    p_ref = 1 - 660 / 1000.0
    assert abs(r.FER() - p_ref) < 2.576 * sqrt(p_ref * (1 - p_ref) / 1000) + 0.005, r.FER()
    assert 60 < r.mean_iters() <= 100
    r0 = A.run_experiment(dec, None, H, -2.0, frames=1 << 17, noise="device", seed=1)   # all-zero word
    assert abs(r0.FER() - r.FER()) < 0.01


def test_config4_optimalh_qpadmm_snr_sweep_sharded(A, pcm):
    """configs[3]: optimalH QP-ADMM (1.2, 0.55), SNR 1..4 dB, sharded exactly as 8 ranks would run it
    (8 contiguous global ranges, counters merged on the host).  Scaled to 8 x 32k frames per point here;
    the reference shows FER 0 at >= 1 dB with 1e4 frames, so FER must stay below 1e-3."""
    H = pcm["optimalH"]
    G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 2048, 239239239)
    dec = A.QPADMMDecoder(1.2, 0.55, 100, 1e-5)
    F = 8 * 32768
    prev = 1.0
    for snr in (1.0, 2.0, 3.0, 4.0):
        tot = None
        for rank in range(8):
            lo, cnt = A.shard_range(F, rank, 8)
            part = A.run_experiment(dec, cws, H, snr, frames=cnt, first_frame=lo, noise="device", seed=77)
            tot = part if tot is None else A.merge_exp_results(tot, part)
        assert tot.total == F
        assert tot.FER() < 1e-3 and tot.FER() <= prev + 1e-4
        prev = tot.FER()
    whole = A.run_experiment(dec, cws, H, 4.0, frames=F, noise="device", seed=77)
    assert (whole.as_vector() == tot.as_vector()).all()     # same frames for 1 or 8 shards


# ---------------------------------------------------------------------------------------- large parity sub-run, threads
def test_bp_100k_frames_identical_to_oracle(A, oracle, matrices, pcm):
    """SURVEY §8(d) config-2 parity sub-run: 10^5 frames with the reference's host noise (frame i <- mt19937(i+1))
    over SNR in {-3,-2,-1,0}: bits and flags identical to the oracle on every frame; exit iterations identical except for the
    stated fp32-vs-80-bit knife edge below (a few sweeps apart, same word, on at most 1 frame in 10^4 — exact exit-iteration
    parity of the fp32 kernel was given up in round 2 for the one-instruction branch selection in phi, bp_core.inc; the three such
    frames of a 4 * 10^6 soak are pinned in test_bp_fp32_knife_edge_frames)."""
    Hm, H = matrices["H05"], pcm["H05"]
    G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 10000, 239239239)
    dec = A.BeliefPropagationDecoder(50)
    threads = min(16, os.cpu_count() or 1)
    for snr, lo, cnt in ((-3.0, 0, 10000), (-2.0, 10000, 30000), (-1.0, 40000, 30000), (0.0, 70000, 30000)):
        y = A.transmit_frames(cws, snr, first_frame=lo, frames=cnt)      # global frames lo..lo+cnt-1, codewords cycle
        ob, ook, oit = oracle.bp_decode(Hm, y, snr, 50, threads=threads)
        bits, ok, iters = dec.decode_batch(H, y, snr)
        assert (ok == ook).all(), (snr, int((ok != ook).sum()))
        assert (bits == ob).all(), snr
        # Stated tolerance on the exit iteration of the fp32 kernel against the 80-bit oracle: the word and the flag
        # are exact (above); the sweep at which the syndrome first vanishes may differ by up to 3 on at most 1 frame in
        # 10^4 (an fp32 / long-double knife edge: 3 of 4 * 10^6 frames in tools/soak_oracle.py — by 1, 2 and 3 sweeps —, none here).
        dit = np.abs(iters.astype(np.int64) - oit.astype(np.int64))
        assert dit.max() <= 3 and (dit != 0).mean() <= 1e-4, (snr, int(dit.max()), int((dit != 0).sum()))
        sent = cws[(np.arange(lo, lo + cnt)) % len(cws)]
        fer = 1 - ((ok == 1) & (bits == sent).all(axis=1)).mean()
        assert {-3.0: 0.45 < fer < 0.6, -2.0: 0.07 < fer < 0.11, -1.0: fer < 0.012, 0.0: fer < 0.002}[snr], (snr, fer)


def test_one_decoder_called_from_many_threads(A, oracle, matrices, pcm):
    """the reference calls ONE decoder object from THREADS_NUM pthreads (experiment.h:101,127-130): concurrent
    calls on one handle must stay correct (they are serialised inside the library)."""
    import threading
    Hm, H = matrices["optimalH"], pcm["optimalH"]
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 5, 64)
    dec = A.BeliefPropagationDecoder(30)
    adm = A.QPADMMDecoder(1.2, 0.55, 60, 1e-5)
    ys = [oracle.transmit_frames(cws, -1.0, first_seed=1000 * t) for t in range(8)]
    exp_bp = [oracle.bp_decode(Hm, y, -1.0, 30, threads=2) for y in ys]
    exp_ad = [oracle.qpadmm_decode(Hm, y, -1.0, 1.2, 0.55, 60, 1e-5, threads=2) for y in ys]
    dec.handle(H), adm.handle(H)     # handle creation itself is done once, as in main.cpp:28-40
    errs = []

    def work(t):
        try:
            for _ in range(3):
                b, o, i = dec.decode_batch(H, ys[t], -1.0)
                assert (b == exp_bp[t][0]).all() and (o == exp_bp[t][1]).all() and (i == exp_bp[t][2]).all()
                b, o, i = adm.decode_batch(H, ys[t], -1.0)
                assert (b == exp_ad[t][0]).all() and (o == exp_ad[t][1]).all()
        except Exception as e:  # noqa: BLE001
            errs.append((t, repr(e)))

    th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    [x.start() for x in th]
    [x.join() for x in th]
    assert not errs, errs


@pytest.mark.parametrize("kind", ["bp", "bp_streamed", "qpadmm"])
def test_one_handle_two_streams_overlapping_launches(A, oracle, matrices, pcm, kind):
    """acg_ldpc_decode_batch_dev is asynchronous on the caller's stream: two launches of ONE handle on two streams,
    issued back to back with no sync in between, must each decode every frame of its batch exactly once (every launch
    owns a work counter; the streamed engine's slabs are ordered on the device).  Both outputs equal the oracle."""
    import torch
    Hm, H = matrices["H05"], pcm["H05"]
    G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 512, 7)
    snr = -1.0
    F = {"bp": 200000, "bp_streamed": 60000, "qpadmm": 60000}[kind]
    nchk = 1500
    if kind == "qpadmm":
        dec = A.QPADMMDecoder(1.95, 0.5, 100, 1e-5)
    else:
        dec = A.BeliefPropagationDecoder(50, engine=A.ENGINE_STREAMED if kind == "bp_streamed" else A.ENGINE_AUTO)
    nw = (H.n + 31) // 32
    ys, outs, exps = [], [], []
    for b in range(2):
        yh = A.transmit_frames(cws, snr, first_frame=b * F, frames=F)
        ys.append(torch.from_numpy(yh).cuda())                  # doubles on the device (the exact-LLR input path)
        outs.append((torch.full((F, nw), -1, dtype=torch.int32, device="cuda"),
                     torch.full((F,), 7, dtype=torch.uint8, device="cuda"),
                     torch.full((F,), -1, dtype=torch.int32, device="cuda")))
        pick = np.r_[0:nchk // 2, F - nchk // 2:F]             # the head and the tail of the batch against the oracle
        if kind == "qpadmm":
            exps.append((pick,) + tuple(oracle.qpadmm_decode(Hm, yh[pick], snr, 1.95, 0.5, 100, 1e-5, threads=8)))
        else:
            exps.append((pick,) + tuple(oracle.bp_decode(Hm, yh[pick], snr, 50, threads=8)))
    dec.handle(H)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for rep in range(3):                                        # repeated so the launches really queue up behind each other
        for b in range(2):
            bits, ok, it = outs[b]
            dec.decode_batch_dev(H, ys[b].data_ptr(), True, F, snr, bits.data_ptr(), ok.data_ptr(), it.data_ptr(),
                                 streams[b].cuda_stream)
    torch.cuda.synchronize()
    serial = []
    for b in range(2):
        bits, ok, it = outs[b]
        okh, ith = ok.cpu().numpy(), it.cpu().numpy()
        assert set(np.unique(okh).tolist()) <= {0, 1} and ith.min() >= 0, "a frame was skipped"   # sentinels overwritten
        bh = np.unpackbits(bits.cpu().numpy().view(np.uint8), axis=1, bitorder="little")[:, :H.n]
        pick, ob, ook, oit = exps[b]
        assert (okh[pick] == ook).all() and (bh[pick] == ob).all() and (ith[pick] == oit).all(), (kind, b)
        serial.append((bh, okh, ith))
    # and the whole batches against a serial run on the handle's own stream
    for b in range(2):
        bits, ok, it = (torch.zeros_like(t) for t in outs[b])
        dec.decode_batch_dev(H, ys[b].data_ptr(), True, F, snr, bits.data_ptr(), ok.data_ptr(), it.data_ptr())
        dec.sync(H)
        bh = np.unpackbits(bits.cpu().numpy().view(np.uint8), axis=1, bitorder="little")[:, :H.n]
        assert (bh == serial[b][0]).all() and (ok.cpu().numpy() == serial[b][1]).all() and (it.cpu().numpy() == serial[b][2]).all(), (kind, b)
    dec.close()


def test_host_api_pipelined_chunks_double_and_float(A, oracle, matrices, pcm):
    """acg_ldpc_decode_batch / _f32 stream large host batches through two pinned staging sets in chunks of 65536 frames
    (host threads pack / unpack while the GPU decodes): a batch of three chunks with a ragged tail must come back frame
    for frame equal to the device-buffer entry point on the same symbols, and equal to the oracle on a sample from every
    chunk.  float32 symbols: the oracle is fed the same rounded symbols."""
    import torch
    Hm, H = matrices["H05"], pcm["H05"]
    G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 1024, 11)
    snr, F = -1.5, 2 * 65536 + 9001
    y64 = A.transmit_frames(cws, snr, first_frame=5, frames=F)
    pick = np.r_[0:300, 65536 - 150:65536 + 150, 2 * 65536 - 150:2 * 65536 + 150, F - 300:F]
    nw = (H.n + 31) // 32
    for dec, ofn in ((A.BeliefPropagationDecoder(50), lambda yy: oracle.bp_decode(Hm, yy, snr, 50, threads=8)),
                     (A.QPADMMDecoder(1.95, 0.5, 60, 1e-5), lambda yy: oracle.qpadmm_decode(Hm, yy, snr, 1.95, 0.5, 60, 1e-5, threads=8))):
        for y in (y64, y64.astype(np.float32)):
            bits, ok, it = dec.decode_batch(H, y, snr)
            yd = torch.from_numpy(y).cuda()
            db = torch.zeros((F, nw), dtype=torch.int32, device="cuda")
            dk = torch.zeros(F, dtype=torch.uint8, device="cuda")
            di = torch.zeros(F, dtype=torch.int32, device="cuda")
            dec.decode_batch_dev(H, yd.data_ptr(), y.dtype == np.float64, F, snr, db.data_ptr(), dk.data_ptr(), di.data_ptr())
            dec.sync(H)
            ref_bits = np.unpackbits(db.cpu().numpy().view(np.uint8), axis=1, bitorder="little")[:, :H.n]
            assert (bits == ref_bits).all() and (ok == dk.cpu().numpy()).all() and (it == di.cpu().numpy()).all(), (dec.name(), y.dtype)
            ob, ook, oit = ofn(y[pick].astype(np.float64))
            assert (bits[pick] == ob).all() and (ok[pick] == ook).all() and (it[pick] == oit).all(), (dec.name(), y.dtype)
        dec.close()


# ---------------------------------------------------------------------------------------- workgroup-per-frame fused BP
@pytest.mark.parametrize("lpf", [256, 1024])
def test_block_mode_equals_oracle_on_h05(A, oracle, matrices, pcm, lpf):
    """one workgroup (256 / 1024 threads) per frame: same sweeps, same results"""
    Hm, H = matrices["H05"], pcm["H05"]
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 33, 600)
    for snr in (-2.0, 3.0):
        y = oracle.transmit_frames(cws, snr, first_seed=8000)
        ob, ook, oit = oracle.bp_decode(Hm, y, snr, 50, threads=8)
        for ee in (True, False):
            dec = A.BeliefPropagationDecoder(50, lanes_per_frame=lpf, early_exit=ee)
            bits, ok, iters = dec.decode_batch(H, y, snr)
            assert dec.layout(H)["lanes_per_frame"] == lpf
            dec.close()
            assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all(), (lpf, snr, ee)
    # Monte-Carlo path: same Philox frames as the wavefront kernels -> identical counters
    a = A.BeliefPropagationDecoder(50, lanes_per_frame=64)
    b = A.BeliefPropagationDecoder(50, lanes_per_frame=lpf)
    ra = A.run_experiment(a, cws, H, -1.5, frames=20000, first_frame=7, noise="device", seed=9)
    rb = A.run_experiment(b, cws, H, -1.5, frames=20000, first_frame=7, noise="device", seed=9)
    assert (ra.as_vector() == rb.as_vector()).all()


def test_block_mode_auto_for_mid_size_code(A, oracle):
    """a 1500 x 3000 (3,6) code (E = 9000: 36 KB of messages per frame) is decoded by the workgroup-per-frame kernel"""
    Hm = A.regular_ldpc(1500, 3000, 3, 6, seed=5)
    H = A.ParityCheckMatrix(Hm)
    rng = np.random.default_rng(1)
    snr = 1.0
    y = 1.0 + np.sqrt(A.llr_variance(snr)) * rng.standard_normal((96, 3000))
    ob, ook, oit = oracle.bp_decode(Hm, y, snr, 40, threads=8)
    dec = A.BeliefPropagationDecoder(40)
    bits, ok, iters = dec.decode_batch(H, y, snr)
    assert dec.layout(H)["lanes_per_frame"] == 256
    assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all()
    ms = A.MinSumDecoder(40, 0.75, precision=A.PREC_F64, lanes_per_frame=256)
    ob, ook, oit = oracle.minsum_decode(Hm, y, snr, 40, 0.75, threads=8)
    bits, ok, iters = ms.decode_batch(H, y, snr)
    assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all()


# ---------------------------------------------------------------------------------------- wide nodes, odd sizes
@pytest.mark.parametrize("dv,dc,m,n", [(4, 16, 100, 400), (4, 32, 50, 400), (3, 12, 75, 300)])
def test_high_degree_codes_all_engines(A, oracle, dv, dc, m, n):
    """check degree 12 / 16 / 32: the rolled (degree > 8) sweeps of the fused kernels and the streamed engine"""
    Hm = A.regular_ldpc(m, n, dv, dc, seed=11)
    H = A.ParityCheckMatrix(Hm)
    rng = np.random.default_rng(dc)
    snr = 4.0
    y = 1.0 + np.sqrt(A.llr_variance(snr)) * rng.standard_normal((300, n))
    ob, ook, oit = oracle.bp_decode(Hm, y, snr, 25, threads=8)
    mb, mok, mit = oracle.minsum_decode(Hm, y, snr, 25, 0.8, threads=8)
    engines = [A.ENGINE_FUSED] + ([A.ENGINE_STREAMED] if dc <= 16 else [])
    for eng in engines:
        for lpf in ((0, 16, 32) if eng == A.ENGINE_FUSED else (0,)):
            dec = A.BeliefPropagationDecoder(25, engine=eng, lanes_per_frame=lpf)
            bits, ok, iters = dec.decode_batch(H, y, snr)
            dec.close()
            assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all(), (eng, lpf)
        ms = A.MinSumDecoder(25, 0.8, engine=eng, precision=A.PREC_F64)
        bits, ok, iters = ms.decode_batch(H, y, snr)
        ms.close()
        assert (ok == mok).all() and (bits == mb).all() and (iters == mit).all(), eng
    if dc > 16:
        with pytest.raises(A.LdpcError):
            A.BeliefPropagationDecoder(5, engine=A.ENGINE_STREAMED).decode_batch(H, y[:2], snr)
    assert ook.mean() > 0.5


def test_odd_sizes_and_iteration_limits(A, oracle, matrices, pcm):
    """n not a multiple of 32, one frame, fewer frames than lanes, max_iter 0 and 1"""
    Hm = A.regular_ldpc(45, 75, 3, 5, seed=2)        # n = 75
    H = A.ParityCheckMatrix(Hm)
    rng = np.random.default_rng(4)
    y = 1.0 + 0.7 * rng.standard_normal((5, 75))
    for it in (0, 1, 2, 30):
        ob, ook, oit = oracle.bp_decode(Hm, y, 1.0, it, threads=2)
        for eng in (A.ENGINE_FUSED, A.ENGINE_STREAMED):
            for frames in (1, 5):
                dec = A.BeliefPropagationDecoder(it, engine=eng)
                bits, ok, iters = dec.decode_batch(H, y[:frames], 1.0)
                dec.close()
                assert (ok == ook[:frames]).all() and (bits == ob[:frames]).all() and (iters == oit[:frames]).all(), (it, eng, frames)
    Hb, H5 = matrices["H05"], pcm["H05"]
    yy = 1.0 + 0.8 * rng.standard_normal((3, H5.n))
    ob, ook, oit = oracle.qpadmm_decode(Hb, yy, 0.0, 1.95, 0.5, 1, 1e-5)
    bits, ok, iters = A.QPADMMDecoder(1.95, 0.5, 1, 1e-5).decode_batch(H5, yy, 0.0)
    assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all()


def test_qpadmm_mc_block_and_wave_kernels_agree(A, pcm):
    """QP-ADMM Monte-Carlo: the workgroup-per-frame kernel (auto) and the wavefront kernels (L = 64, 32) see the same
    Philox frames and must return identical counters (decode is bit-exact in both)."""
    H = pcm["H05"]
    G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 100, 3)
    res = []
    for lpf in (0, 64, 32):
        dec = A.QPADMMDecoder(1.95, 0.5, 100, 1e-5, lanes_per_frame=lpf)
        res.append(A.run_experiment(dec, cws, H, -1.0, frames=6000, first_frame=11, noise="device", seed=21).as_vector())
        dec.close()
    assert (res[0] == res[1]).all() and (res[0] == res[2]).all(), res


def test_non_finite_and_extreme_symbols(A, oracle, matrices, pcm):
    """the reference has no clipping — zero, huge, infinite and NaN channel symbols flow through phi as
    IEEE says (phi(0) = inf, inf - inf = NaN, NaN <= 0 is false -> bit 0).  Same hard outputs on the device."""
    Hm, H = matrices["H05"], pcm["H05"]
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 8, 200)
    y = oracle.transmit_frames(cws, 1.0, first_seed=60000)
    rng = np.random.default_rng(9)
    for f in range(200):
        k = rng.integers(0, 6)
        idx = rng.choice(H.n, size=k, replace=False)
        kind = f % 5
        if kind == 0:
            y[f, idx] = 0.0
        elif kind == 1:
            y[f, idx] = 1e6 * np.sign(y[f, idx] + 1e-9)
        elif kind == 2:
            y[f, idx] = np.inf * np.sign(1 - 2.0 * cws[f, idx] + 0.0)
        elif kind == 3:
            y[f, idx] = np.nan
        else:
            y[f, idx] = -np.inf      # wrong-signed certainty on up to 5 positions
    ob, ook, oit = oracle.bp_decode(Hm, y, 1.0, 50, threads=8)
    for kw in (dict(), dict(lanes_per_frame=64), dict(engine=A.ENGINE_STREAMED), dict(precision=A.PREC_F64)):
        dec = A.BeliefPropagationDecoder(50, **kw)
        bits, ok, iters = dec.decode_batch(H, y, 1.0)
        dec.close()
        bad = np.nonzero((ok != ook) | (bits != ob).any(axis=1) | (iters != oit))[0]
        assert len(bad) == 0, (kw, bad[:10], [(int(f) % 5) for f in bad[:10]])


def test_edge_graphs_and_extreme_symbols_other_engines(A, oracle, matrices, pcm):
    """the ragged graph of test_bp_edge_cases (degree-1 / degree-2 checks, empty row, isolated variables) through the
    streamed and workgroup-per-frame engines and min-sum; QP-ADMM with non-finite symbols"""
    H = np.zeros((5, 9), np.uint8)
    H[0, [0, 1, 2, 3]] = 1
    H[1, [2, 3, 4]] = 1
    H[2, [5]] = 1
    H[3, [0, 6]] = 1
    rng = np.random.default_rng(3)
    y = 1.0 + 0.9 * rng.standard_normal((200, 9))
    y[::7, 2] = 0.0
    y[::11, 4] = np.inf
    ob, ook, oit = oracle.bp_decode(H, y, 0.0, 12, threads=2)
    mb, mok, mit = oracle.minsum_decode(H, y, 0.0, 12, 1.0, threads=2)
    for kw in (dict(engine=A.ENGINE_STREAMED), dict(lanes_per_frame=256), dict(lanes_per_frame=16)):
        dec = A.BeliefPropagationDecoder(12, **kw)
        bits, ok, iters = dec.decode_batch(H, y, 0.0)
        dec.close()
        assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all(), kw
        ms = A.MinSumDecoder(12, 1.0, precision=A.PREC_F64, **kw)
        bits, ok, iters = ms.decode_batch(H, y, 0.0)
        ms.close()
        assert (ok == mok).all() and (bits == mb).all() and (iters == mit).all(), kw
    Hm, H5 = matrices["H05"], pcm["H05"]
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 8, 60)
    yy = oracle.transmit_frames(cws, 0.0, first_seed=70000)
    yy[0, 3] = np.nan
    yy[1, 10] = np.inf
    yy[2, 17] = -np.inf
    yy[3, :5] = 0.0
    yy[4, 100] = 1e300
    ob, ook, oit = oracle.qpadmm_decode(Hm, yy, 0.0, 1.95, 0.5, 40, 1e-5, threads=4)
    for lpf in (0, 64):
        dec = A.QPADMMDecoder(1.95, 0.5, 40, 1e-5, lanes_per_frame=lpf)
        bits, ok, iters = dec.decode_batch(H5, yy, 0.0)
        dec.close()
        assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all(), lpf


# ---------------------------------------------------------------------------------------- the reference's published tables
@pytest.mark.parametrize("matrix,gfile,alpha,mu,rows", [
    # reports/report_H05.csv:17,19,21 (QP-ADMM rows) and :6,8 (BP rows below the race floor)
    ("H05", "G05.txt", 1.95, 0.5, {"qpadmm": {-3.0: 0.3380, -2.0: 0.0379, -1.0: 0.0016}, "bp": {-3.0: 0.5185, -2.0: 0.1038}}),
    # reports/report_opt.csv:17,19,21 and :6,8
    ("optimalH", None, 1.2, 0.55, {"qpadmm": {-3.0: 0.2751, -2.0: 0.0245, -1.0: 0.0001}, "bp": {-3.0: 0.4860, -2.0: 0.0851}}),
])
def test_published_fer_tables_statistically(A, pcm, oracle, matrix, gfile, alpha, mu, rows):
    """The only numbers the reference publishes for this path: FER per SNR over 10^4 frames with BP(100) and
    QP-ADMM(alpha, mu, 10000, 1e-5) (main.cpp:25-33).  Same pipeline here (codewords mt19937(239'239'239), frame i
    <- mt19937(i+1)); their run used 8 racy threads and another standard library, so the pin is
    statistical: inside the 99.9 % binomial interval of two independent 10^4-frame estimates."""
    from math import sqrt
    H = pcm[matrix]
    if gfile:
        G = oracle.read_pcm(os.path.join(DATA, gfile))      # main.cpp:59-60 (non-OPTIMAL build)
    else:
        G, _ = H.get_orthogonal()                             # main.cpp:56-57
    cws = A.gen_random_codewords(G, 10000, 239239239)
    decs = {"bp": A.BeliefPropagationDecoder(100), "qpadmm": A.QPADMMDecoder(alpha, mu, 10000, 1e-5)}
    for kind, tab in rows.items():
        for snr, p_ref in tab.items():
            r = A.run_experiment(decs[kind], cws, H, snr, noise="host")
            half = 3.29 * sqrt(2 * max(p_ref, 3e-4) * (1 - p_ref) / 10000) + 2e-4
            if kind == "bp" and snr > -2.5:
                # the published BP rows carry the Node::counter race of the 8-thread run (floor 0.034 at
                # >= -1 dB); it only ever ADDS failures, already ~ +0.017 at -2 dB (0.1038 published vs 0.0868 for the
                # race-free decoder, which is bit-identical to the single-threaded reference on 10^5 frames)
                assert p_ref - 0.03 < r.FER() < p_ref + half, (matrix, kind, snr, r.FER(), p_ref)
            else:
                assert abs(r.FER() - p_ref) < half, (matrix, kind, snr, r.FER(), p_ref, half)


def test_specialised_instances_equal_the_general_ones(A, pcm):
    """The instances with general paths compiled out (QP-ADMM LEAN for the tuple placement of H05, BP REG for regular codes)
    against the general instances of the same kernels (ACG_ADMM_NO_LEAN / ACG_BP_NO_REGULAR): bits, flags, sweep counts."""
    H = pcm["H05"]
    rng = np.random.default_rng(11)
    y = 1.0 + 0.8 * rng.standard_normal((3000, H.n))
    y[5, 7] = np.nan                      # the lean instance passes a NaN through its clamp (MODE.DX10_CLAMP cleared)
    y[6, :4] = [0.0, -0.0, np.inf, -np.inf]
    res = []
    for env in (None, "ACG_ADMM_NO_LEAN"):
        if env:
            os.environ[env] = "1"
        try:
            for eps in (0.0, 1e-5):
                dec = A.QPADMMDecoder(1.95, 0.5, 60, eps)
                res.append(dec.decode_batch(H, y, -1.0))
                dec.close()
        finally:
            if env:
                del os.environ[env]
    for a, b in ((res[0], res[2]), (res[1], res[3])):
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2] == b[2]).all()
    Hm = A.regular_ldpc(3000, 6000, 3, 6, seed=3)   # 36 KB of index table: the register-index instances, which have a REG twin
    Hr = A.ParityCheckMatrix(Hm)
    yr = 1.0 + 0.75 * rng.standard_normal((48, Hr.n))
    out = []
    for env in (None, "ACG_BP_NO_REGULAR"):
        if env:
            os.environ[env] = "1"
        try:
            for make in (lambda: A.MinSumDecoder(40, 0.75, lanes_per_frame=1024), lambda: A.BeliefPropagationDecoder(40, lanes_per_frame=1024)):
                dec = make()
                assert dec.layout(Hr)["lanes_per_frame"] == 1024
                out.append(dec.decode_batch(Hr, yr, 0.5))
                dec.close()
        finally:
            if env:
                del os.environ[env]
    for a, b in ((out[0], out[2]), (out[1], out[3])):
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2] == b[2]).all()
