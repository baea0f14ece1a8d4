"""GPU: the workgroup-per-frame layered kernel (bp_layered_block_kernel, lanes_per_frame 256 / 512 / 1024 with SCHEDULE_LAYERED)
against the repo's own operation-exact restatements (tests/layered_ref.py), run over the sets of ParityCheckMatrix.layers_block():
word, flag and iteration count of EVERY frame identical.  The kernel calls the same per-check functions as bp_layered_kernel
(bp_layer_math.inc), so nothing is tolerated anywhere; the FER test at the end keeps the two-sided binomial band of
test_layered_25_not_worse_than_flooding_50.

SNRs: (3,6)-regular codes under normalised min-sum have their threshold near Es/N0 = -1.3 dB, so short ones are run a little
above it (n = 768: -1.0 dB, n = 4000: -1.2 dB) where a 25-iteration run decodes most frames and fails some; the tests assert
that the RESTATEMENT has both kinds."""
import ctypes as C

import numpy as np
import pytest

from layered_ref import knife_edge_case, layered_minsum, layered_sumproduct_exact
from test_layered_block import ragged_40x80

pytestmark = pytest.mark.gpu


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


# name -> (matrix, SNR in dB, frames)
CASES = {
    "384x768": (lambda A, M: A.regular_ldpc(384, 768, 3, 6, seed=1), -1.0, 600),      # every set partly filled at L = 256
    "ragged": (lambda A, M: ragged_40x80(A), 1.0, 600),                             # mostly idle threads, degrees 1, 3, 5, 6
    "H05": (lambda A, M: M["H05"], -2.0, 600),                                      # quasi-cyclic: the block rows
    "2000x4000": (lambda A, M: A.regular_ldpc(2000, 4000, 3, 6, seed=2), -1.2, 200),  # sets wider than 256, some below 512
}


class Case:
    """matrix, sets, noisy all-zero codewords and the restatements computed on them (once each, shared by the tests)"""

    def __init__(self, A, oracle, matrices, name):
        make, self.snr, frames = CASES[name]
        self.name = name
        self.Hm = np.asarray(make(A, matrices))
        self.H = A.ParityCheckMatrix(self.Hm)
        self.Z, self.layers = self.H.layers_block()
        self.sizes = [int((l >= 0).sum()) for l in self.layers]
        self.y = oracle.transmit_frames(np.zeros((frames, self.Hm.shape[1]), dtype=np.uint8), self.snr, first_seed=1)
        self._ref = {}

    def minsum(self, it, msg):
        k = ("ms", it, msg)
        if k not in self._ref:
            self._ref[k] = layered_minsum(self.Hm, self.layers, self.y, self.snr, it, 0.75, _dt(msg))
        return self._ref[k]


@pytest.fixture(scope="module")
def cases(A, oracle, matrices):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(A, oracle, matrices, name)
        return made[name]
    return get


def _dt(msg):
    return np.float16 if msg == "f16" else np.float32


def _prec(A, msg):
    return A.PREC_F16 if msg == "f16" else A.PREC_DEFAULT


def _assert_same(got, want, ctx):
    """equality of bits, ok and iters for every frame; the message names the first differing frame and what differs there"""
    (bits, ok, iters), (rb, rok, rit) = got, want
    assert bits.shape == rb.shape and ok.shape == rok.shape and iters.shape == rit.shape, ctx
    d_flag, d_word, d_count = ok != rok, (bits != rb).any(axis=1), iters != rit
    bad = d_flag | d_word | d_count
    if bad.any():
        f = int(np.nonzero(bad)[0][0])
        what = ", ".join(n for n, d in (("flag", d_flag), ("word", d_word), ("count", d_count)) if d[f])
        pytest.fail("%s: %d of %d frames differ; first: frame %d, differing in %s (kernel ok=%d iters=%d, restatement ok=%d iters=%d, "
                    "%d word bits apart)" % (ctx, int(bad.sum()), len(bad), f, what, ok[f], iters[f], rok[f], rit[f],
                                             int((bits[f] != rb[f]).sum())))


def _decode(A, algo, H, y, snr, it, msg, L, ee=True, expect_kernel="bp_layered_block_kernel"):
    kw = dict(schedule=A.SCHEDULE_LAYERED, early_exit=ee, precision=_prec(A, msg), lanes_per_frame=L)
    dec = A.MinSumDecoder(it, 0.75, **kw) if algo == "minsum" else A.BeliefPropagationDecoder(it, **kw)
    try:
        out = dec.decode_batch(H, y, snr)
        d = dec.describe(H)
        assert "kernel=%s " % expect_kernel in d and "schedule=layered messages=%s" % ("fp16" if msg == "f16" else "fp32") in d, d
        if expect_kernel == "bp_layered_block_kernel" and L:
            assert "lanes_per_frame=%d " % L in d and d.startswith("minsum" if algo == "minsum" else "sum-product"), d
        return out
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------- min-sum, four matrices
@pytest.mark.parametrize("msg", ["f32", "f16"])
@pytest.mark.parametrize("name,L", [("384x768", 256), ("ragged", 256), ("ragged", 1024), ("H05", 256), ("2000x4000", 256),
                                    ("2000x4000", 512)])
def test_block_minsum_equals_restatement(A, cases, name, L, msg):
    """25 / 3 / 0 iterations, early exit and fixed work, fp32 and fp16 messages: identical to layered_minsum over the sets of
    layers_block().  The shapes: sets that fill a fraction of the workgroup (384 x 768: 68 ... 2 checks), sets of a few checks
    under 1024 threads (ragged), sets of 353 ... checks under 256 threads (two passes, the second partly filled) and under 512
    (one partly filled pass)."""
    c = cases(name)
    if name == "384x768":
        assert c.sizes == [68, 68, 65, 61, 55, 45, 20, 2]
    if name == "2000x4000":
        assert max(c.sizes) > 256 and min(c.sizes) < 256 and max(c.sizes) < 512, c.sizes
    if name == "H05":
        assert c.Z == 20 and c.sizes == [20] * 8
    for it in (25, 3, 0):
        want = c.minsum(it, msg)
        for ee in (True, False):
            _assert_same(_decode(A, "minsum", c.H, c.y, c.snr, it, msg, L, ee), want, (name, L, msg, it, "early exit" if ee else "fixed work"))
        rok = want[1]
        if it == 25:
            assert 0 < rok.sum() < len(rok), (name, int(rok.sum()))      # decoded and failed frames, both exits covered
        if it == 0:
            assert not rok.any() and not want[0].any() and (want[2] == 0).all()


@pytest.mark.parametrize("msg", ["f32", "f16"])
@pytest.mark.parametrize("algo", ["minsum", "bp"])
def test_block_equals_the_wavefront_group_kernel_on_H05(A, cases, algo, msg):
    """H05: both engines walk the same eight block rows, so the new kernel must give what bp_layered_kernel (lanes_per_frame = 0,
    20 lanes per frame) gives on the same 600 frames, bit for bit — in both check rules and both modes"""
    c = cases("H05")
    assert (c.layers == c.H.layers()[2]).all()
    for it in (25, 3):
        for ee in (True, False):
            old = _decode(A, algo, c.H, c.y, c.snr, it, msg, 0, ee, expect_kernel="bp_layered_kernel")
            new = _decode(A, algo, c.H, c.y, c.snr, it, msg, 256, ee)
            _assert_same(new, old, ("H05 against bp_layered_kernel", algo, msg, it, ee))
    assert 0 < old[1].sum() < len(old[1])


# ------------------------------------------------------------------------------------------------------------ sum-product
@pytest.mark.parametrize("msg", ["f32", "f16"])
def test_block_sumproduct_equals_exact_restatement(A, cases, device_phi, msg):
    """layered_sumproduct_exact with the device's own phi on the 384 x 768 code at L = 256: 25 / 3 / 0 iterations, both modes"""
    c = cases("384x768")
    for it in (25, 3, 0):
        want = layered_sumproduct_exact(c.Hm, c.layers, c.y, c.snr, it, device_phi, _dt(msg))
        for ee in (True, False):
            _assert_same(_decode(A, "bp", c.H, c.y, c.snr, it, msg, 256, ee), want, ("sum-product", msg, it, "early exit" if ee else "fixed work"))
        if it == 25:
            assert 0 < want[1].sum() < len(want[1])


@pytest.mark.parametrize("msg", ["f32", "f16"])
def test_block_sumproduct_knife_edges(A, device_phi, msg):
    """the eight-check graph of layered_ref.knife_edge_case (degrees 1 ... 8, one check per set), max_iter = 1: one message of the
    first iteration decides each frame's flag to the last bit — the order of the prefix / suffix sums, the saturation constant,
    the single rounding to the storage type"""
    Hm, y, knife, high = knife_edge_case(device_phi, 1.0, 320, 3, _dt(msg))
    H = A.ParityCheckMatrix(Hm)
    Z, layers = H.layers_block()
    assert sorted(int(Hm[l[l >= 0]].sum(axis=1)[0]) for l in layers) == list(range(1, 9)) and all((l >= 0).sum() == 1 for l in layers)
    post = []
    want = layered_sumproduct_exact(Hm, layers, y, 1.0, 1, device_phi, _dt(msg), posteriors=post)
    pk = post[0][np.arange(len(y)), knife]
    assert len(y) >= 200 and (pk[~high] == 0).all() and not np.signbit(pk[~high]).any() and (pk[high] < 0).all()
    assert 0 < want[1].sum() < len(y)
    for ee in (True, False):
        _assert_same(_decode(A, "bp", H, y, 1.0, 1, msg, 256, ee), want, ("knife edges", msg, "early exit" if ee else "fixed work"))


# ----------------------------------------------------------------------------------------------------------- batch shapes
def test_block_batch_shapes_and_float_symbols(A, cases):
    """1, 2, 3 and 257 frames on ONE handle (frames are dealt one at a time: fewer frames than workgroups, and more), then the
    same frames as float32 symbols — the (double) y * (2 / sigma^2) LLR path"""
    c = cases("384x768")
    y = c.y[:257]
    want = tuple(a[:257] for a in c.minsum(25, "f32"))      # (frames are independent: a prefix is a prefix)
    dec = A.MinSumDecoder(25, 0.75, schedule=A.SCHEDULE_LAYERED, lanes_per_frame=256)
    try:
        for F in (1, 2, 3, 257):
            _assert_same(dec.decode_batch(c.H, y[:F], c.snr), tuple(a[:F] for a in want), ("frames", F))
        y32 = y.astype(np.float32)
        want32 = layered_minsum(c.Hm, c.layers, y32, c.snr, 25, 0.75, symbols_f32=True)
        _assert_same(dec.decode_batch(c.H, y32, c.snr), want32, "float32 symbols")
        assert dec.live_handles() == 1 and "bp_layered_block_kernel" in dec.describe(c.H)
        lay = dec.layout(c.H)
        lds = 4 * (((768 + 1 + 3) & ~3) + 384 * 6 + 768 // 32)
        assert (lay["lds_bytes_per_frame"], lay["lanes_per_frame"], lay["frames_per_block"]) == (lds, 256, 1) and lay["grid_blocks"] >= 1, lay
    finally:
        dec.close()
    assert 0 < want[1].sum() < 257


# ------------------------------------------------------------------------------------------- the size the engine exists for
def test_block_decodes_the_5000_x_10000_code(A, oracle):
    """(3,6)-regular 5000 x 10000, E = 30 000: 10 004 posterior + 30 000 message + 313 output words = 161 268 bytes of LDS with
    fp32 messages.  16 noisy all-zero codewords at +2 dB, 8 iterations, L = 1024, identical to layered_minsum; and with
    lanes_per_frame = 0 — refused before this engine existed ("a frame does not fit in LDS") — the same words through it."""
    Hm = A.regular_ldpc(5000, 10000, 3, 6, seed=1)
    H = A.ParityCheckMatrix(Hm)
    Z, layers = H.layers_block()
    assert Z == 0 and [int((l >= 0).sum()) for l in layers] == [883, 866, 840, 772, 687, 559, 304, 84, 5]
    y = oracle.transmit_frames(np.zeros((16, 10000), dtype=np.uint8), 2.0, first_seed=1)
    for msg, lds in (("f32", 161268), ("f16", 101268)):
        want = layered_minsum(Hm, layers, y, 2.0, 8, 0.75, _dt(msg))
        dec = A.MinSumDecoder(8, 0.75, schedule=A.SCHEDULE_LAYERED, lanes_per_frame=1024, precision=_prec(A, msg))
        try:
            _assert_same(dec.decode_batch(H, y, 2.0), want, ("5000 x 10000", msg))
            d = dec.describe(H)
            assert "kernel=bp_layered_block_kernel " in d and "lanes_per_frame=1024 " in d and "lds_block=%d " % lds in d and "sets=9 " in d, d
            assert dec.layout(H)["lds_bytes_per_frame"] == lds
        finally:
            dec.close()
        if msg == "f32":
            auto = A.MinSumDecoder(8, 0.75, schedule=A.SCHEDULE_LAYERED)
            try:
                _assert_same(auto.decode_batch(H, y, 2.0), want, "5000 x 10000, lanes_per_frame = 0")
                d = auto.describe(H)
                assert "kernel=bp_layered_block_kernel " in d and "lanes_per_frame=1024 " in d, d
            finally:
                auto.close()
        assert want[1].any()


# ------------------------------------------------------------------------------------------------------------ Monte-Carlo
def test_block_monte_carlo_host_noise_equals_decode_batch(A, cases):
    """run_experiment with the reference's host noise = the seven counters formed here from decode_batch of
    acg_ldpc_transmit_host's frames and the sent words (experiment.h:25-68,109-120)"""
    c = cases("384x768")
    F, n = 2000, 768
    dec = A.MinSumDecoder(25, 0.75, schedule=A.SCHEDULE_LAYERED, lanes_per_frame=256)
    try:
        got = A.run_experiment(dec, None, c.H, c.snr, frames=F, noise="host").as_vector()
        y = A.transmit_frames(np.zeros((1, n), dtype=np.uint8), c.snr, 0, F)
        bits, ok, iters = dec.decode_batch(c.H, y, c.snr)
    finally:
        dec.close()
    ham = (y <= 0).sum(axis=1)                                     # the all-zero word was sent
    cw = np.array([ok[f] == 1 and c.H.is_codeword(bits[f]) for f in range(F)])
    correct = cw & ~bits.any(axis=1)
    want = np.array([correct.sum(), (cw & ~correct).sum(), F, ham.sum(), ham[correct].sum(), ham[~correct].sum(), iters.sum()], dtype=np.int64)
    assert (got == want).all(), (got, want)
    assert 0 < want[0] < F


def test_block_monte_carlo_device_noise_shards(A, cases):
    """device noise (AWGN kernel -> decode -> classification kernel): a 50 000-frame run = the sum of the shards 12 345 + 1 + rest"""
    c = cases("384x768")
    F = 50000
    dec = A.MinSumDecoder(25, 0.75, schedule=A.SCHEDULE_LAYERED, lanes_per_frame=256)
    try:
        whole = A.run_experiment(dec, None, c.H, c.snr, frames=F, noise="device", seed=9).as_vector()
        parts = sum(A.run_experiment(dec, None, c.H, c.snr, frames=k, first_frame=lo, noise="device", seed=9).as_vector()
                    for lo, k in ((0, 12345), (12345, 1), (12346, F - 12346)))
    finally:
        dec.close()
    assert (whole == parts).all(), (whole, parts)
    assert whole[2] == F and whole[3] == whole[4] + whole[5] and 0 < whole[0] < F


# -------------------------------------------------------------------------------------------------------------------- FER
def test_block_layered_25_not_worse_than_flooding_50(A, cases):
    """2000 x 4000, L = 512, device noise, 20 000 frames per point, at the first of -1.5, -1.0, -0.5, 0.0 dB where flooding
    min-sum-50 has 0.01 <= FER <= 0.3: FER(layered-25) <= FER(flooding-50) + 3 sqrt(p (1 - p) / N).  And every ok = 1 word of a
    2000-frame host-side sample is a codeword."""
    c = cases("2000x4000")
    F = 20000
    lay = A.MinSumDecoder(25, 0.75, schedule=A.SCHEDULE_LAYERED, lanes_per_frame=512)
    flo = A.MinSumDecoder(50, 0.75)
    try:
        assert "kernel=bp_layered_block_kernel " in lay.describe(c.H) and "schedule=flooding" in flo.describe(c.H)
        seen = []
        for snr in (-1.5, -1.0, -0.5, 0.0):
            rf = A.run_experiment(flo, None, c.H, snr, frames=F, noise="device", seed=3)
            seen.append((snr, rf.FER()))
            if not 0.01 <= rf.FER() <= 0.3:
                continue
            rl = A.run_experiment(lay, None, c.H, snr, frames=F, noise="device", seed=3)
            assert rl.total == rf.total == F and rl.sum_hamming == rf.sum_hamming      # the same frames
            fl, ff = rl.FER(), rf.FER()
            print("2000 x 4000 %+.1f dB: FER layered-25 (L = 512) %.5f  flooding-50 %.5f; mean iterations %.2f / %.2f; pseudo %d / %d"
                  % (snr, fl, ff, rl.mean_iters(), rf.mean_iters(), rl.pseudo, rf.pseudo))
            assert fl <= ff + 3.0 * np.sqrt(ff * (1 - ff) / F), (snr, fl, ff)
            y = A.transmit_frames(np.zeros((1, 4000), dtype=np.uint8), snr, 0, 2000)
            bits, ok, _ = lay.decode_batch(c.H, y, snr)
            assert ok.any() and all(c.H.is_codeword(b) for b in bits[ok == 1])
            break
        else:
            pytest.fail("no SNR of the list gave flooding min-sum-50 a FER in [0.01, 0.3]: %s" % seen)
    finally:
        lay.close()
        flo.close()


# -------------------------------------------------------------------------------------------------------------- refusals
def test_block_refusals_through_the_c_abi(A, cases):
    """each gives a non-zero code and a message, and no handle"""
    L = A.lib()
    small = cases("384x768").H
    big = A.ParityCheckMatrix(A.regular_ldpc(8000, 16000, 3, 6, seed=1))      # fp32: 64 KB of posteriors + 192 KB of messages

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
    assert create(small)[0] == 0
    for what, H, kw, word in (("fp64", small, dict(precision=A.PREC_F64), "fp32 posteriors"),
                              ("streamed", small, dict(engine=A.ENGINE_STREAMED), "LDS-resident"),
                              ("128 lanes", small, dict(lanes_per_frame=128), "lanes_per_frame"),
                              ("frame beyond LDS", big, dict(lanes_per_frame=1024), "does not fit in LDS"),
                              ("frame beyond LDS, auto", big, dict(lanes_per_frame=0), "does not fit in LDS")):
        rc, msg, h = create(H, **kw)
        assert rc != 0 and word in msg and not h, (what, rc, msg)
