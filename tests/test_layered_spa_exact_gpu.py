"""GPU: the layered SUM-PRODUCT kernel (bp_layered_kernel<..., ALGO = 0>, layer_back_spa) against the operation-exact restatement
of tests/layered_ref.py, EXACTLY: word, flag and iteration count of every frame.

Everything in layer_back_spa except phi is plain IEEE fp32 that numpy reproduces (Q = P - R, XOR of sign bits, a prefix sum in
edge order, a suffix sum in reverse edge order, fminf(., 83.25f), one rounding to the storage type, P' = Q + R'), and phi is a
pure function of its input bits that the library exports: acg_ldpc_debug_phi_sat returns the bits of Dom<float>::phi.  The
restatement is handed that device function, so there is nothing left to tolerate.  phi's own accuracy is held to long double by
test_phi_device_vs_long_double, its special values by test_phi_fast_path_boundaries; tests/test_layered.py ties the
restatement (with a host phi) to the float64 sum-product on the CPU and keeps the rate / FER tests that tie the kernel to the
reference side.

Also here: the layered kernels of BOTH check rules on extreme channel symbols (zero, huge, infinite)."""
import numpy as np
import pytest

from layered_ref import knife_edge_case, layered_minsum, layered_sumproduct_exact

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


def _spa(A, H, y, snr, it, msg, ee=True):
    dec = A.BeliefPropagationDecoder(it, schedule=A.SCHEDULE_LAYERED, early_exit=ee,
                                     precision=A.PREC_F16 if msg == "f16" else A.PREC_DEFAULT)
    try:
        out = dec.decode_batch(H, y, snr)
        d = dec.describe(H)
        assert "bp_layered_kernel" in d and d.startswith("sum-product"), d
        return out
    finally:
        dec.close()


def _dt(msg):
    return np.float16 if msg == "f16" else np.float32


# ------------------------------------------------------------------------------------------ a. the reference's matrices
@pytest.mark.parametrize("msg", ["f32", "f16"])
@pytest.mark.parametrize("name,snr", [("H05", -2.0), ("H05", 0.5), ("optimalH", -2.0), ("H", 1.0)])
def test_layered_sumproduct_equals_restatement(A, oracle, matrices, device_phi, name, snr, msg):
    """600 frames per matrix and SNR, 25 / 3 / 0 iterations, early exit and fixed work, messages stored in fp32 or fp16.  At
    -2 dB some frames stop after a quiet round, some pass the final syndrome pass or fail: every exit is covered."""
    Hm = matrices[name]
    H = A.ParityCheckMatrix(Hm)
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 5, 600)
    y = oracle.transmit_frames(cws, snr, first_seed=1)
    _, _, layers = H.layers()
    for it in (25, 3, 0):
        want = layered_sumproduct_exact(Hm, layers, y, snr, it, device_phi, _dt(msg))
        for ee in (True, False):
            _assert_same(_spa(A, H, y, snr, it, msg, ee), want, (name, snr, msg, it, "early exit" if ee else "fixed work"))
        rok = want[1]
        if it == 25 and snr < 0:
            assert 0 < rok.sum() < len(rok), rok.sum()      # the restatement decodes some frames and fails some
        if it == 0:
            assert not rok.any() and not want[0].any() and (want[2] == 0).all()


# ------------------------------------------------------------------------------------------ b. ragged batches, float symbols
def test_layered_sumproduct_ragged_batches_and_float_symbols(A, oracle, matrices, device_phi):
    """batches that do not fill their wavefronts (three frames of 20 lanes per wavefront on optimalH), on one decoder object;
    then the same frames as float32 symbols: the (double) y * (2 / sigma^2) LLR path"""
    Hm = matrices["optimalH"]
    H = A.ParityCheckMatrix(Hm)
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 9, 257)
    y = oracle.transmit_frames(cws, -1.0, first_seed=50)
    _, _, layers = H.layers()
    want = layered_sumproduct_exact(Hm, layers, y, -1.0, 20, device_phi)      # (frames are independent: a prefix is a prefix)
    dec = A.BeliefPropagationDecoder(20, schedule=A.SCHEDULE_LAYERED)
    try:
        for F in (1, 2, 3, 59, 60, 61, 257):
            _assert_same(dec.decode_batch(H, y[:F], -1.0), tuple(a[:F] for a in want), ("optimalH", "frames", F))
        y32 = y.astype(np.float32)
        want32 = layered_sumproduct_exact(Hm, layers, y32, -1.0, 20, device_phi, symbols_f32=True)
        _assert_same(dec.decode_batch(H, y32, -1.0), want32, ("optimalH", "float32 symbols"))
        assert dec.describe(H).startswith("sum-product") and "bp_layered_kernel" in dec.describe(H)
    finally:
        dec.close()
    assert 0 < want[1].sum() < 257


# ------------------------------------------------------------------------------------------ c. ragged graph
def ragged_graph(A):
    """the graph of test_layered_ragged_graph (an empty check, a degree-3 and a degree-1 check among degree-6 ones, an isolated
    variable, whose checks drop to degree 5) + four rows of degree 2, 4, 7 and 8: every D-specific instance of the layer step"""
    Hm = A.regular_ldpc(40, 80, 3, 6, seed=5).copy()
    Hm[0, :] = 0
    Hm[1, np.nonzero(Hm[1])[0][:3]] = 0
    Hm[2, np.nonzero(Hm[2])[0][1:]] = 0          # degree 1
    Hm[:, 7] = 0                                  # an isolated variable
    extra = np.zeros((4, 80), dtype=Hm.dtype)
    extra[0, [10, 50]] = 1
    extra[1, [5, 26, 44, 63]] = 1
    extra[2, np.arange(3, 80, 11)] = 1            # 7 variables
    extra[3, np.arange(1, 80, 10)] = 1            # 8 variables
    return np.vstack([Hm, extra])


@pytest.mark.parametrize("msg", ["f32", "f16"])
def test_layered_sumproduct_ragged_graph(A, oracle, device_phi, msg):
    """layers of check degree 1 ... 8, partly filled (lanes beyond the layer's count must neither store nor count), an empty
    check and an isolated variable; 400 noisy all-zero codewords at +1 dB, 15 iterations, both modes"""
    Hm = ragged_graph(A)
    H = A.ParityCheckMatrix(Hm)
    G, Z, layers = H.layers()
    degs = [int(Hm[l[l >= 0]].sum(axis=1)[0]) for l in layers]
    assert Z == 0 and set(degs) == {1, 2, 3, 4, 5, 6, 7, 8}, degs
    assert any(0 < (l >= 0).sum() < G for l in layers)
    y = oracle.transmit_frames(np.zeros((400, 80), dtype=np.uint8), 1.0, first_seed=9)
    want = layered_sumproduct_exact(Hm, layers, y, 1.0, 15, device_phi, _dt(msg))
    for ee in (True, False):
        _assert_same(_spa(A, H, y, 1.0, 15, msg, ee), want, ("ragged graph", msg, "early exit" if ee else "fixed work"))
    assert want[1].any()


# ------------------------------------------------------------------------------------------ d. group widths
# The layering picks the group width G that needs the fewest wavefront-steps per frame, sum(ceil(set / G)) / (64 / G), the
# smallest G winning a tie.  ceil(s / 16) <= 2 ceil(s / 32) and <= 4 ceil(s / 64) for every set size s, so G = 16 never costs
# more than G = 32 or G = 64: NO matrix reaches the G = 32 and G = 64 instances through the API (lanes_per_frame must equal
# the layering's choice).  What can be reached: G = 16, and G = 20 with a matrix that is not quasi-cyclic — the position
# table read from memory where H05 / optimalH build it from their circulant shifts.
WIDTHS = {16: (48, 96, 3), 20: (96, 192, 1)}


@pytest.mark.parametrize("msg", ["f32", "f16"])
@pytest.mark.parametrize("width", sorted(WIDTHS))
def test_layered_sumproduct_group_widths(A, device_phi, width, msg):
    """(3,6)-regular codes whose greedy layering picks 16 and 20 lanes per frame, partly filled layers in both; 200 noisy
    all-zero codewords at +2 dB, 12 iterations"""
    m, n, seed = WIDTHS[width]
    Hm = A.regular_ldpc(m, n, 3, 6, seed=seed)
    H = A.ParityCheckMatrix(Hm)
    G, Z, layers = H.layers()
    assert (G, Z) == (width, 0) and any(0 < (l >= 0).sum() < G for l in layers)
    y = 1.0 + np.sqrt(10.0 ** (-2.0 / 10.0) / 2.0) * np.random.default_rng(21).standard_normal((200, n))
    want = layered_sumproduct_exact(Hm, layers, y, 2.0, 12, device_phi, _dt(msg))
    for ee in (True, False):
        _assert_same(_spa(A, H, y, 2.0, 12, msg, ee), want, ("G", width, msg, "early exit" if ee else "fixed work"))
    assert want[1].any()


# ------------------------------------------------------------------------------------------ one message, to the last bit
@pytest.mark.parametrize("msg", ["f32", "f16"])
def test_layered_sumproduct_knife_edges(A, device_phi, msg):
    """Random frames cannot see a message that is one ulp off: on the CPU neither another order of the suffix sums nor
    half-precision storage changes more than 3 words, flags or counts in 2000 frames (tests/test_layered.py).  These frames can:
    layered_ref.knife_edge_case builds them, with the device's phi, so that one message of the first iteration meets a posterior
    of exactly minus its value (or minus the next fp32 number) — the frame's flag after max_iter = 1 says whether the kernel's
    message has every bit of the restatement's.  Checks of degree 1 ... 8, one per layer: the order of the prefix / suffix sums
    (D >= 4), the saturation constant (D = 1), the single rounding to the storage type."""
    Hm, y, knife, high = knife_edge_case(device_phi, 1.0, 320, 3, _dt(msg))
    H = A.ParityCheckMatrix(Hm)
    G, Z, layers = H.layers()
    assert sorted(int(Hm[l[l >= 0]].sum(axis=1)[0]) for l in layers) == list(range(1, 9)) and all((l >= 0).sum() == 1 for l in layers)
    post = []
    want = layered_sumproduct_exact(Hm, layers, y, 1.0, 1, device_phi, _dt(msg), posteriors=post)
    pk = post[0][np.arange(len(y)), knife]
    assert len(y) >= 200 and (pk[~high] == 0).all() and not np.signbit(pk[~high]).any() and (pk[high] < 0).all()
    assert 0 < want[1].sum() < len(y)
    for ee in (True, False):
        _assert_same(_spa(A, H, y, 1.0, 1, msg, ee), want, ("knife edges", msg, "early exit" if ee else "fixed work"))


# ------------------------------------------------------------------------------------------ e. extreme symbols
def _extreme_frames(oracle, Hm, kinds):
    """H05 at +1 dB, 200 frames; up to five random positions per frame replaced, cycling through `kinds`:
    0 zero, 1 1e6 with the sent sign, 2 infinity with the sent sign, 3 -infinity whatever was sent"""
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 17, 200)
    y = oracle.transmit_frames(cws, 1.0, first_seed=300).copy()
    sent = 1.0 - 2.0 * cws.astype(np.float64)
    rng = np.random.default_rng(4)
    k = 0
    for f in range(len(y)):
        for v in rng.choice(y.shape[1], size=int(rng.integers(0, 6)), replace=False):
            kind = kinds[k % len(kinds)]
            k += 1
            y[f, v] = (0.0, 1e6 * sent[f, v], np.inf * sent[f, v], -np.inf)[kind]
    return cws, y


@pytest.mark.parametrize("msg", ["f32", "f16"])
def test_layered_sumproduct_extreme_symbols(A, oracle, matrices, device_phi, msg):
    """zero, huge, correctly signed infinite and wrongly infinite symbols, and one symbol of 1e300 whose LLR overflows fp32 to
    infinity.  All NaN-free in sum-product: phi(0) = inf, phi(inf) = 0, messages are bounded by 83.25 and no inf - inf can form
    (asserted on the restatement's final posteriors).  NaN symbols are out of scope: the sign of a generated NaN differs between
    x86 and the GPU, so their hard decisions have no host restatement."""
    Hm = matrices["H05"]
    H = A.ParityCheckMatrix(Hm)
    _, _, layers = H.layers()
    cws, y = _extreme_frames(oracle, Hm, (0, 1, 2, 3))
    last = oracle.transmit_frames(cws[:1], 1.0, first_seed=999).copy()
    last[0, 11] = 1e300 * (1.0 - 2.0 * cws[0, 11])
    y = np.vstack([y, last])
    assert np.isinf(y).any() and (y == 0).any() and not np.isnan(y).any()
    post = []
    want = layered_sumproduct_exact(Hm, layers, y, 1.0, 25, device_phi, _dt(msg), posteriors=post)
    assert not np.isnan(post[0]).any() and np.isinf(post[0][-1, 11])
    _assert_same(_spa(A, H, y, 1.0, 25, msg), want, ("extreme symbols", msg))
    assert 0 < want[1].sum() < len(y)      # (a symbol pinned to the wrong infinity cannot be corrected)


@pytest.mark.parametrize("msg", ["f32", "f16"])
def test_layered_minsum_extreme_symbols(A, oracle, matrices, msg):
    """layered MIN-SUM on the zero and +-1e6 frames above, exact against layered_minsum.  Infinite symbols are left out for
    min-sum: a scaled infinite minimum can meet an opposite infinite posterior and form a NaN.  (With at most five replaced symbols
    per frame no check of H05 has all its other edges huge, so no half-precision message overflows to infinity here either.)"""
    Hm = matrices["H05"]
    H = A.ParityCheckMatrix(Hm)
    _, _, layers = H.layers()
    cws, y = _extreme_frames(oracle, Hm, (0, 1))
    assert (y == 0).any() and (np.abs(y) == 1e6).any() and np.isfinite(y).all()
    want = layered_minsum(Hm, layers, y, 1.0, 25, 0.75, _dt(msg))
    dec = A.MinSumDecoder(25, 0.75, schedule=A.SCHEDULE_LAYERED, precision=A.PREC_F16 if msg == "f16" else A.PREC_DEFAULT)
    try:
        got = dec.decode_batch(H, y, 1.0)
        assert "bp_layered_kernel" in dec.describe(H) and "layered" in dec.describe(H)
    finally:
        dec.close()
    _assert_same(got, want, ("min-sum, extreme symbols", msg))
    assert want[1].any()
