"""GPU: the wide-check layered kernel (bp_layered_wide_kernel: SCHEDULE_LAYERED on a code whose largest check has 9 ... 32
variables) against the repo's own operation-exact restatements (tests/layered_ref.py), run over the sets of
ParityCheckMatrix.layers_wide(): word, flag and iteration count of EVERY frame identical, nothing tolerated.  The codes are those
of tests/layered_wide_cases.py; the FER test keeps the one-sided binomial band of test_block_layered_25_not_worse_than_flooding_50.

SNRs (Es/N0): the restatements decode some frames and fail others there — qc4x24z27 and qc6x32z64 at +2.5 dB, qc2x10z300 at
+3.0 dB, ragged at +3.0 dB (chosen from the restatements alone: tests/test_layered_wide.py); the tests assert it again."""
import ctypes as C

import numpy as np
import pytest

import layered_wide_cases as W
from layered_ref import layered_minsum, layered_sumproduct_exact
from test_layered_block_gpu import _assert_same, _dt, _prec

pytestmark = pytest.mark.gpu

KERNEL = "bp_layered_wide_kernel"
FRAMES = 200


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


@pytest.fixture(scope="module")
def device_phi(A):
    """float32 array -> Dom<float>::phi of every element, evaluated on the device (log2(e)-scaled domain), same shape"""
    def phi(x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.zeros(3 * x.size, dtype=np.uint32)
        assert A.lib().acg_ldpc_debug_phi_sat(x.ctypes.data, out.ctypes.data, x.size) == 0
        return out[0::3].copy().view(np.float32).reshape(x.shape)
    return phi


class Case:
    """matrix, sets, noisy all-zero codewords (symbol +1) and the restatements computed on them (once each, shared by the tests)"""

    def __init__(self, A, oracle, name):
        self.name = name
        self.snr = W.CASES[name][2]
        self.Hm = np.array(W.matrix(name))
        self.H = A.ParityCheckMatrix(self.Hm)
        self.Z, self.layers = self.H.layers_wide()
        self.sizes = [int((l >= 0).sum()) for l in self.layers]
        self.y = oracle.transmit_frames(np.zeros((FRAMES, self.Hm.shape[1]), dtype=np.uint8), self.snr, first_seed=1)
        self._ref = {}

    def minsum(self, it, msg):
        k = ("ms", it, msg)
        if k not in self._ref:
            self._ref[k] = layered_minsum(self.Hm, self.layers, self.y, self.snr, it, 0.75, _dt(msg))
        return self._ref[k]

    def sumproduct(self, it, msg, phi):
        k = ("spa", it, msg)
        if k not in self._ref:
            self._ref[k] = layered_sumproduct_exact(self.Hm, self.layers, self.y, self.snr, it, phi, _dt(msg))
        return self._ref[k]


@pytest.fixture(scope="module")
def cases(A, oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(A, oracle, name)
        return made[name]
    return get


def _decode(A, algo, H, y, snr, it, msg, L, ee=True):
    kw = dict(schedule=A.SCHEDULE_LAYERED, early_exit=ee, precision=_prec(A, msg), lanes_per_frame=L)
    dec = A.MinSumDecoder(it, 0.75, **kw) if algo == "minsum" else A.BeliefPropagationDecoder(it, **kw)
    try:
        out = dec.decode_batch(H, y, snr)
        d = dec.describe(H)
        assert "kernel=%s " % KERNEL in d and "schedule=layered messages=%s" % ("fp16" if msg == "f16" else "fp32") in d, d
        assert d.startswith("minsum" if algo == "minsum" else "sum-product"), d
        if L:
            assert "lanes_per_frame=%d " % L in d, d
        return out
    finally:
        dec.close()


# ----------------------------------------------------------------------------------------------------------------- min-sum
@pytest.mark.parametrize("msg", ["f32", "f16"])
@pytest.mark.parametrize("name,L", [("qc4x24z27", 256), ("qc6x32z64", 256), ("qc6x32z64", 1024), ("qc2x10z300", 256),
                                    ("qc2x10z300", 512), ("ragged", 256)])
def test_wide_minsum_equals_restatement(A, cases, name, L, msg):
    """25 / 3 / 0 iterations, early exit and fixed work, fp32 and fp16 messages, 200 frames: identical to layered_minsum over the
    sets of layers_wide().  The shapes: degree 22-23 in sets of 27 checks (three chunks, the last partly filled), degree 32 in
    sets of 64 (four full chunks; one wavefront of 4 or of 16 has work), degree 10 in sets of 300 (two passes at L = 256, the
    second partly filled; one partly filled pass at L = 512), and narrow and wide checks in one code (ragged: 3 ... 19)."""
    c = cases(name)
    for it in (25, 3, 0):
        want = c.minsum(it, msg)
        for ee in (True, False):
            _assert_same(_decode(A, "minsum", c.H, c.y, c.snr, it, msg, L, ee), want, (name, L, msg, it, "early exit" if ee else "fixed work"))
        rok = want[1]
        if it == 25:
            assert 0 < rok.sum() < len(rok), (name, int(rok.sum()))      # decoded and failed frames, both exits covered
        if it == 0:
            assert not rok.any() and not want[0].any() and (want[2] == 0).all()


# ------------------------------------------------------------------------------------------------------------- sum-product
@pytest.mark.parametrize("msg", ["f32", "f16"])
@pytest.mark.parametrize("name", ["qc4x24z27", "qc6x32z64", "ragged"])
def test_wide_sumproduct_equals_exact_restatement(A, cases, device_phi, name, msg):
    """layered_sumproduct_exact with the device's own phi, L = 256: 25 and 3 iterations, both modes"""
    c = cases(name)
    for it in (25, 3):
        want = c.sumproduct(it, msg, device_phi)
        for ee in (True, False):
            _assert_same(_decode(A, "bp", c.H, c.y, c.snr, it, msg, 256, ee), want, (name, "sum-product", msg, it, "early exit" if ee else "fixed work"))
        if it == 25:
            assert 0 < want[1].sum() < len(want[1]), (name, int(want[1].sum()))


@pytest.mark.parametrize("msg", ["f32", "f16"])
def test_wide_sumproduct_knife_edges(A, device_phi, msg):
    """eight checks of degree 9, 12, 16, 17, 24, 25, 31, 32 on disjoint variables (one check per set), max_iter = 1: one message
    of the first iteration decides each frame's flag to the last bit — a prefix or suffix sum taken in another order across a
    chunk boundary, a padding edge that contributes anything but +0, a missing or doubled rounding shows here"""
    Hm, y, knife, high = W.knife_edge_case_wide(device_phi, 1.0, 320, 3, _dt(msg))
    H = A.ParityCheckMatrix(Hm)
    Z, layers = H.layers_wide()
    assert Hm.shape == (8, 166) and Z == 0
    assert sorted(int(Hm[l[l >= 0]].sum(axis=1)[0]) for l in layers) == W.KNIFE_DEGREES and all((l >= 0).sum() == 1 for l in layers)
    post = []
    want = layered_sumproduct_exact(Hm, layers, y, 1.0, 1, device_phi, _dt(msg), posteriors=post)
    pk = post[0][np.arange(len(y)), knife]
    assert len(y) >= 200 and (pk[~high] == 0).all() and not np.signbit(pk[~high]).any() and (pk[high] < 0).all()
    assert 0 < want[1].sum() < len(y)
    for ee in (True, False):
        _assert_same(_decode(A, "bp", H, y, 1.0, 1, msg, 256, ee), want, ("knife edges", msg, "early exit" if ee else "fixed work"))


# --------------------------------------------------------------------------------------------------- lanes_per_frame = 0
def test_wide_lanes_per_frame_zero_picks_the_smallest_workgroup_that_holds_a_set(A, cases):
    """qc6x32z64 (sets of 64): 256, and the words of lanes_per_frame = 256; qc2x10z300 (sets of 300): 512"""
    c = cases("qc6x32z64")
    dec = A.MinSumDecoder(25, 0.75, schedule=A.SCHEDULE_LAYERED)
    try:
        _assert_same(dec.decode_batch(c.H, c.y, c.snr), c.minsum(25, "f32"), "qc6x32z64, lanes_per_frame = 0")
        d = dec.describe(c.H)
        assert "kernel=%s " % KERNEL in d and "lanes_per_frame=256 " in d and "largest_set=64 " in d, d
        c2 = cases("qc2x10z300")
        _assert_same(dec.decode_batch(c2.H, c2.y, c2.snr), c2.minsum(25, "f32"), "qc2x10z300, lanes_per_frame = 0")
        d = dec.describe(c2.H)
        assert "kernel=%s " % KERNEL in d and "lanes_per_frame=512 " in d and "largest_set=300 " in d, d
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------------------ batch shapes
def test_wide_batch_shapes_and_float_symbols(A, cases):
    """1 and 63 frames on one handle (fewer frames than workgroups), then float32 symbols — the (double) y * (2 / sigma^2) LLR
    path — and the layout report"""
    c = cases("qc4x24z27")
    want = c.minsum(25, "f32")
    dec = A.MinSumDecoder(25, 0.75, schedule=A.SCHEDULE_LAYERED, lanes_per_frame=256)
    try:
        for F in (1, 63):
            _assert_same(dec.decode_batch(c.H, c.y[:F], c.snr), tuple(a[:F] for a in want), ("frames", F))
        y32 = c.y.astype(np.float32)
        want32 = layered_minsum(c.Hm, c.layers, y32, c.snr, 25, 0.75, symbols_f32=True)
        _assert_same(dec.decode_batch(c.H, y32, c.snr), want32, "float32 symbols")
        assert dec.live_handles() == 1 and KERNEL in dec.describe(c.H)
        lay = dec.layout(c.H)
        n, E = c.Hm.shape[1], int(c.Hm.sum())
        lds = 4 * (((n + 1 + 3) & ~3) + E + (n + 31) // 32)
        assert (lay["lds_bytes_per_frame"], lay["lanes_per_frame"], lay["frames_per_block"]) == (lds, 256, 1) and lay["grid_blocks"] >= 1, lay
    finally:
        dec.close()
    assert 0 < want32[1].sum() < FRAMES


# ------------------------------------------------------------------------------------------------------------- Monte-Carlo
def test_wide_monte_carlo_host_noise_equals_decode_batch(A, cases):
    """run_experiment with the reference's host noise = the seven counters formed here from decode_batch of
    acg_ldpc_transmit_host's frames and the sent words (experiment.h:25-68,109-120)"""
    c = cases("qc4x24z27")
    F, n = 2000, c.Hm.shape[1]
    dec = A.MinSumDecoder(25, 0.75, schedule=A.SCHEDULE_LAYERED, lanes_per_frame=256)
    try:
        got = A.run_experiment(dec, None, c.H, c.snr, frames=F, noise="host").as_vector()
        y = A.transmit_frames(np.zeros((1, n), dtype=np.uint8), c.snr, 0, F)
        bits, ok, iters = dec.decode_batch(c.H, y, c.snr)
        assert "kernel=%s " % KERNEL in dec.describe(c.H)
    finally:
        dec.close()
    ham = (y <= 0).sum(axis=1)                                     # the all-zero word was sent
    cw = np.array([ok[f] == 1 and c.H.is_codeword(bits[f]) for f in range(F)])
    correct = cw & ~bits.any(axis=1)
    want = np.array([correct.sum(), (cw & ~correct).sum(), F, ham.sum(), ham[correct].sum(), ham[~correct].sum(), iters.sum()], dtype=np.int64)
    assert (got == want).all(), (got, want)
    assert 0 < want[0] < F


def test_wide_monte_carlo_device_noise_shards_and_detail(A, cases):
    """device noise (AWGN kernel -> decode -> classification kernel): a 50 000-frame run = the sum of the shards 12 345 + 1 +
    rest; and the detail run's base counters are those of acg_ldpc_mc_run on the same cfg"""
    c = cases("qc4x24z27")
    F = 50000
    dec = A.MinSumDecoder(25, 0.75, schedule=A.SCHEDULE_LAYERED, lanes_per_frame=256)
    try:
        whole = A.run_experiment(dec, None, c.H, c.snr, frames=F, noise="device", seed=9).as_vector()
        parts = sum(A.run_experiment(dec, None, c.H, c.snr, frames=k, first_frame=lo, noise="device", seed=9).as_vector()
                    for lo, k in ((0, 12345), (12345, 1), (12346, F - 12346)))
        det = A.run_experiment_detail(dec, None, c.H, c.snr, frames=F, noise="device", seed=9, cap=4)
        assert "kernel=%s " % KERNEL in dec.describe(c.H)
    finally:
        dec.close()
    assert (whole == parts).all(), (whole, parts)
    assert whole[2] == F and whole[3] == whole[4] + whole[5] and 0 < whole[0] < F
    assert (det.as_vector() == whole).all(), (det, whole)


# --------------------------------------------------------------------------------------------------------------------- FER
@pytest.mark.parametrize("algo", ["minsum", "bp"])
def test_wide_layered_25_not_worse_than_flooding_50(A, cases, algo):
    """qc6x32z64, device noise, 20 000 frames per point, at the first of +2.25, +2.5, +2.75, +3.0, +3.25 dB where flooding-50 of the
    same check rule (the project's fused flooding kernel) has 0.01 <= FER <= 0.3: FER(layered-25) <= FER(flooding-50) +
    3 sqrt(p (1 - p) / N) on the same frames.  And every ok = 1 word of a 2000-frame host-side sample is a codeword."""
    c = cases("qc6x32z64")
    F = 20000
    if algo == "minsum":
        lay = A.MinSumDecoder(25, 0.75, schedule=A.SCHEDULE_LAYERED)
        flo = A.MinSumDecoder(50, 0.75)
    else:
        lay = A.BeliefPropagationDecoder(25, schedule=A.SCHEDULE_LAYERED)
        flo = A.BeliefPropagationDecoder(50)
    try:
        assert "kernel=%s " % KERNEL in lay.describe(c.H) and "schedule=flooding" in flo.describe(c.H)
        seen = []
        for snr in (2.25, 2.5, 2.75, 3.0, 3.25):
            rf = A.run_experiment(flo, None, c.H, snr, frames=F, noise="device", seed=3)
            seen.append((snr, rf.FER()))
            if not 0.01 <= rf.FER() <= 0.3:
                continue
            rl = A.run_experiment(lay, None, c.H, snr, frames=F, noise="device", seed=3)
            assert rl.total == rf.total == F and rl.sum_hamming == rf.sum_hamming      # the same frames
            fl, ff = rl.FER(), rf.FER()
            print("qc6x32z64 %s %+.2f dB: FER layered-25 %.5f  flooding-50 %.5f; mean iterations %.2f / %.2f; pseudo %d / %d"
                  % (algo, snr, fl, ff, rl.mean_iters(), rf.mean_iters(), rl.pseudo, rf.pseudo))
            assert fl <= ff + 3.0 * np.sqrt(ff * (1 - ff) / F), (snr, fl, ff)
            y = A.transmit_frames(np.zeros((1, c.Hm.shape[1]), dtype=np.uint8), snr, 0, 2000)
            bits, ok, _ = lay.decode_batch(c.H, y, snr)
            assert ok.any() and all(c.H.is_codeword(b) for b in bits[ok == 1])
            break
        else:
            pytest.fail("no SNR of the list gave flooding-50 a FER in [0.01, 0.3]: %s" % seen)
    finally:
        lay.close()
        flo.close()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_wide_refusals_through_the_c_abi(A, cases):
    """each gives a non-zero code and a message, and no handle"""
    L = A.lib()
    wide = cases("qc6x32z64").H
    Hm33 = np.zeros((2, 40), dtype=np.uint8)
    Hm33[0, :33] = 1
    Hm33[1, 30:] = 1
    deg33 = A.ParityCheckMatrix(Hm33)
    big = A.ParityCheckMatrix(W.quasi_cyclic(6, 32, 256, 5))       # fp32: 32 KB of posteriors + 192 KB of messages

    def create(H, **kw):
        p = A._lib.Params()
        L.acg_ldpc_params_default(C.byref(p))
        p.algo, p.max_iter, p.ms_scale, p.schedule, p.lanes_per_frame = A._lib.ALGO_MINSUM, 10, 0.75, A.SCHEDULE_LAYERED, 256
        for k, v in kw.items():
            setattr(p, k, v)
        h = C.c_void_p()
        rc = L.acg_ldpc_decoder_create(H._h, C.byref(p), C.byref(h))
        msg = L.acg_ldpc_last_error().decode()
        if rc == 0:
            L.acg_ldpc_decoder_destroy(h)
        return rc, msg, h.value
    for Lw in (0, 256, 512, 1024):
        assert create(wide, lanes_per_frame=Lw)[0] == 0
    for what, H, kw, word in (("degree 33", deg33, dict(), "degree above 32"),
                              ("degree 33, auto", deg33, dict(lanes_per_frame=0), "degree above 32"),
                              ("fp64", wide, dict(precision=A.PREC_F64), "fp32 posteriors"),
                              ("streamed", wide, dict(engine=A.ENGINE_STREAMED), "LDS-resident"),
                              ("128 lanes", wide, dict(lanes_per_frame=128), "lanes_per_frame"),
                              ("frame beyond LDS", big, dict(lanes_per_frame=1024), "does not fit in LDS"),
                              ("frame beyond LDS, auto", big, dict(lanes_per_frame=0), "does not fit in LDS")):
        rc, msg, h = create(H, **kw)
        assert rc != 0 and word in msg and not h, (what, rc, msg)
