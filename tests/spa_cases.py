"""graphs shared by the operation-exact GPU tests of the flooding kernels (tests/test_minsum_exact_gpu.py,
tests/test_spa_exact_gpu.py): the node degrees at which the kernels take another path"""
import numpy as np


def ragged():
    """degree-1 and degree-2 checks, an empty row, degree-0 and degree-1 variables (the graph of test_bp_edge_cases)"""
    H = np.zeros((5, 9), np.uint8)
    H[0, [0, 1, 2, 3]] = 1
    H[1, [2, 3, 4]] = 1
    H[2, [5]] = 1
    H[3, [0, 6]] = 1
    return H


def irregular():
    """variable degree 1..4, check degree 1..8 — one-variable checks included (their message is inf * scale in min-sum,
    phi(+0) = +inf in sum-product), which test_pair_f16_minsum_kernels removes"""
    Hi = np.zeros((300, 600), np.uint8)
    r = np.random.default_rng(8)
    for v in range(600):
        Hi[r.choice(300, size=1 + (v % 4), replace=False), v] = 1
    for i in np.nonzero(Hi.sum(1) > 8)[0]:
        Hi[i, np.nonzero(Hi[i])[0][8:]] = 0
    for i, d in ((3, 1), (57, 1), (120, 1), (200, 2), (201, 2)):      # a few checks cut down to one / two variables
        Hi[i, np.nonzero(Hi[i])[0][d:]] = 0
    Hi = Hi[:, Hi.sum(0) >= 1]
    assert set(Hi.sum(1)) >= {1, 2, 8} and set(Hi.sum(0)) == {1, 2, 3, 4}
    return Hi


# ------------------------------------------------------------------------------------------ flooding sum-product case sets
# One SNR (Es/N0, dB) per matrix at which 50 sweeps take BOTH exits within 192 frames and the exit iterations spread from a few
# sweeps to the budget (tests/test_spa_ref.py asserts it on the restatement), and +6 dB, where phi saturates.
SPA_SNR = {"H05": -2.0, "optimalH": -2.0, "H": -1.0}
SPA_SNR_SATURATED = 6.0
SPA_FRAMES = 192
SPA_TRACE_FRAMES = 64          # acg_ldpc_debug_bp_trace takes at most 64 frames
SPA_TRACE_SNRS = (-2.0, SPA_SNR_SATURATED)     # the traced sets of the three matrices


def spa_frames(oracle, Hm, snr, frames=SPA_FRAMES):
    """random codewords + the reference's host noise -> (codewords, symbols [frames, n] float64)"""
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 23, frames)
    return cws, oracle.transmit_frames(cws, snr, first_seed=7000)


def noisy_zero(n, frames, snr, seed):
    """all-zero codeword + AWGN at Es/N0 = snr dB, for graphs without a generator matrix at hand"""
    return 1.0 + np.sqrt(10.0 ** (-snr / 10.0) / 2.0) * np.random.default_rng(seed).standard_normal((frames, n))


def ragged_frames(frames=SPA_FRAMES):
    return 1.0 + 0.9 * np.random.default_rng(3).standard_normal((frames, 9)), 0.0      # symbols, snr


def irregular_frames(n, frames=SPA_FRAMES):
    return noisy_zero(n, frames, 1.0, 19), 1.0


def wide_code():
    """(4,16)-regular 100 x 400: check degree 16, the streamed engines' generic-degree path"""
    from acg_alp_ldpc_amd.codes import regular_ldpc
    return regular_ldpc(100, 400, 4, 16, seed=3)


def wide_frames(frames=SPA_TRACE_FRAMES):
    return noisy_zero(400, frames, 3.0, 29), 3.0
