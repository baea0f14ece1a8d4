"""numpy restatement of the device AWGN generator (Philox4x32-10 + Box-Muller; awgn_kernel in mc_kernels.hip and its in-kernel
copies in bp_core.inc, bp_block.hip, bp_layered.hip and admm_kernels.hip) and of the Monte-Carlo classification.

Every step up to the three transcendental instructions is an integer or IEEE fp32 operation and is reproduced bit for bit: the
Philox words, u1 = fl32(fl32(fl32(a) + 0.5f) * 2^-32) and u2 = fl32(fl32(b >> 8) * 2^-24).  From there on the restatement is
float64 (ln, sqrt, cos, sin), so what separates it from the device is the accuracy of v_log_f32 / v_sin_f32 / v_cos_f32 and the
fp32 rounding of r, r * cos, r * sin and the final fma — nothing structural.  tests/test_awgn_ref.py holds it to the Random123
known answers and to N(0, 1); tests/test_awgn_exact_gpu.py holds the device to it."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # Philox4x32 multipliers (Salmon et al. 2011), on c0 and c2
W0, W1 = 0x9E3779B9, 0xBB67AE85          # Weyl key increments
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
ZMAX = math.sqrt(2 * 33 * math.log(2))   # a = 0 -> u1 = 2^-33 -> r = 6.7637: the generator's largest |z|


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """ten rounds on uint64 arrays holding 32-bit words (broadcast against each other) -> the four output words"""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(x) for x in (c0, c1, c2, c3, k0, k1)))
    for _ in range(10):
        p0 = np.uint64(M0) * c0                      # 32 x 32 -> 64 bits, exact in uint64
        p1 = np.uint64(M1) * c2
        n0 = (p1 >> S32) ^ c1 ^ k0
        n2 = (p0 >> S32) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & MASK, n2, p0 & MASK
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def uniforms(a, b):
    """the two fp32 uniforms of box_muller, bit-equal to the device's: u1 in [2^-33, 1], u2 in [0, 1) (revolutions)"""
    a32 = _u64(a).astype(np.int64).astype(np.float32)                # v_cvt_f32_u32: round to nearest even
    u1 = (a32 + np.float32(0.5)) * np.float32(2.0 ** -32)
    u2 = (_u64(b) >> np.uint64(8)).astype(np.int64).astype(np.float32) * np.float32(2.0 ** -24)
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    return u1, u2


def box_muller(a, b):
    """two 32-bit words -> two N(0, 1) samples, float64 from the uniforms on"""
    u1, u2 = uniforms(a, b)
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    t = 2.0 * np.pi * u2.astype(np.float64)
    return r * np.cos(t), r * np.sin(t)


def normals(first_frame, frames, n, seed):
    """z[frames, n] of global frames first_frame ... : counter (frame_lo, frame_hi, quad, 0), key (seed_lo, seed_hi); symbol 4q + e
    is (z0, z1 | z0', z1')[e] of box_muller(r0, r1) and box_muller(r2, r3)"""
    nq = (n + 3) // 4
    gf = (int(first_frame) + np.arange(frames, dtype=np.int64)).astype(np.uint64)[:, None]
    q = np.arange(nq, dtype=np.uint64)[None, :]
    seed = int(seed) & (2 ** 64 - 1)
    r0, r1, r2, r3 = philox4x32_10(gf & MASK, gf >> S32, q, 0, seed & 0xFFFFFFFF, seed >> 32)
    z = np.empty((frames, nq, 4), dtype=np.float64)
    z[:, :, 0], z[:, :, 1] = box_muller(r0, r1)
    z[:, :, 2], z[:, :, 3] = box_muller(r2, r3)
    return z.reshape(frames, 4 * nq)[:, :n]


def sigma32(snr):
    """the noise amplitude the kernels are handed: sqrt in double, then cast to float (acg_ldpc_awgn_dev)"""
    return np.float32(math.sqrt(10.0 ** (-(snr / 10.0)) / 2))


def sent_words(first_frame, frames, n, codewords):
    """frame g transmits codewords[g % n_cw]; None: the all-zero word"""
    if codewords is None:
        return np.zeros((frames, n), dtype=np.uint8)
    cw = np.asarray(codewords, dtype=np.uint8)
    idx = np.array([(int(first_frame) + f) % cw.shape[0] for f in range(frames)], dtype=np.int64)
    return cw[idx]


def symbols(first_frame, frames, n, seed, snr, codewords=None):
    """-> (y, z, s, sigma): y = s + float32(sigma) * z in float64, s = 1 - 2 * bit"""
    z = normals(first_frame, frames, n, seed)
    s = 1.0 - 2.0 * sent_words(first_frame, frames, n, codewords).astype(np.float64)
    sg = float(sigma32(snr))
    return s + sg * z, z, s, sg


def classify(y, bits, ok, iters, sent, H=None):
    """the seven counters of the reference's experiment loop (experiment.h:109-120) for decoded frames: correct <=> flagged ok and
    equal to the sent word, pseudo <=> flagged ok and another word; the raw-channel Hamming count of every frame (symbol <= 0 reads
    as 1) goes to the ok or the wrong sum.  H: for decoders whose flag is always set (QP-ADMM) — ok additionally needs a zero
    syndrome, which is the loop's own IsCodeword."""
    okf = np.asarray(ok) == 1
    if H is not None:
        okf &= ((bits.astype(np.int64) @ np.asarray(H, dtype=np.int64).T) % 2 == 0).all(axis=1)
    correct = okf & (bits == sent).all(axis=1)
    ham = np.where(sent == 1, y > 0, y <= 0).sum(axis=1)
    return dict(correct=int(correct.sum()), pseudo=int((okf & ~correct).sum()), total=int(len(okf)), sum_iters=int(np.sum(iters)),
                sum_hamming=int(ham.sum()), sum_hamming_ok=int(ham[correct].sum()), sum_hamming_wrong=int(ham[~correct].sum()))


# ------------------------------------------------------------------------------------------ distribution battery
def _inv_norm_cdf(p):
    """quantiles of N(0, 1) by bisection on erfc (float64; used for 63 bin edges only)"""
    lo, hi = -10.0, 10.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if 0.5 * math.erfc(-mid / math.sqrt(2)) < p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


BIN_EDGES = np.array([_inv_norm_cdf(k / 64.0) for k in range(1, 64)])
TAILS = (1, 2, 3, 4, 5)


def battery(z):
    """{statistic: (value, expectation under i.i.d. N(0, 1), standard error)} for the samples z (any shape): the first four
    moments, the counts of |z| > t and the chi-square over 64 equiprobable bins"""
    z = np.asarray(z, dtype=np.float64).ravel()
    N = z.size
    z2 = z * z
    out = {"mean": (z.mean(), 0.0, 1 / math.sqrt(N)),
           "variance": (z2.mean(), 1.0, math.sqrt(2.0 / N)),                    # second moment about 0: var(z^2) = 2
           "third moment": ((z2 * z).mean(), 0.0, math.sqrt(15.0 / N)),         # var(z^3) = 15
           "fourth moment": ((z2 * z2).mean(), 3.0, math.sqrt(96.0 / N))}       # var(z^4) = 105 - 9
    az = np.abs(z)
    for t in TAILS:
        p = math.erfc(t / math.sqrt(2))
        out["|z| > %d" % t] = (float((az > t).sum()), N * p, math.sqrt(N * p))
    cnt = np.bincount(np.searchsorted(BIN_EDGES, z), minlength=64)
    out["chi-square 64 bins"] = (float(((cnt - N / 64.0) ** 2 / (N / 64.0)).sum()), 63.0, math.sqrt(126.0))
    return out


def cross(a, b):
    """normalised cross-moment mean(a * b) * sqrt(size): N(0, 1) for independent N(0, 1) samples"""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float((a * b).mean() * math.sqrt(a.size))


def pair_correlations(z):
    """z[frames, n], n a multiple of 4: the cross-moments inside one stream — quad-mates, neighbours in a frame, neighbours across
    frames"""
    q = z.reshape(z.shape[0], -1, 4)
    return {"quad e0.e1": cross(q[:, :, 0], q[:, :, 1]), "quad e0.e2": cross(q[:, :, 0], q[:, :, 2]),
            "quad e1.e3": cross(q[:, :, 1], q[:, :, 3]), "adjacent symbols": cross(z[:, :-1], z[:, 1:]),
            "adjacent frames": cross(z[:-1], z[1:])}
