"""Codes with checks of more than 8 variables for the wide-check layered engine (bp_layered_wide_kernel; tests/test_layered_wide.py
on the CPU, tests/test_layered_wide_gpu.py on the device): plain numpy generators with fixed seeds, nothing is read from disk.

  qc4x24z27    4 x 24 blocks of 27 x 27 circulants, each block absent with probability 0.08: 108 x 648, check degree 22-23 (the
               shape of 802.11n rate 5/6), sets of 27 checks — a fraction of one wavefront
  qc6x32z64    6 x 32 blocks of Z = 64: 384 x 2048, E = 12 288, (6,32)-regular — the 10GBASE-T shape, check degree AT the cap
  qc2x10z300   2 x 10 blocks of Z = 300: 600 x 3000, check degree 10, sets of 300 checks: two passes at L = 256, one partly filled
               pass at L = 512
  ragged       not quasi-cyclic, 60 x 400, every variable used: check degrees 3 ... 19 with 8, 9, 16, 17 among them (narrow and
               wide checks in one code, both sides of every chunk boundary), first-fit colouring

and the knife-edge construction of layered_ref.knife_edge_case for wide checks (degrees 9, 12, 16, 17, 24, 25, 31, 32)."""
import numpy as np

from layered_ref import LOG2E_F32, _variance, channel_llr_f32, spa_messages


def quasi_cyclic(mb, nb, Z, seed, p_absent=0.0):
    """mb x nb blocks, each a Z x Z cyclic shift of the identity or, with probability p_absent, zero: row k of block (R, C) has
    its one in column (k + shift) mod Z.  default_rng(seed), block by block in row-major order: one uniform for "absent" (only
    if p_absent > 0), then, for a block that is there, its shift, uniform in 0 ... Z-1."""
    rng = np.random.default_rng(seed)
    Hm = np.zeros((mb * Z, nb * Z), dtype=np.uint8)
    k = np.arange(Z)
    for R in range(mb):
        for Cc in range(nb):
            if p_absent > 0 and rng.random() < p_absent:
                continue
            Hm[R * Z + k, Cc * Z + (k + int(rng.integers(0, Z))) % Z] = 1
    return Hm


RAGGED_DEGREES = [3, 5, 8, 9, 10, 12, 15, 16, 17, 19]


def ragged_60x400(seed=4):
    """60 checks whose degrees cycle through RAGGED_DEGREES, on 400 variables.  Check r first takes the lowest-numbered variables
    no check has used yet (so every variable is used: the degrees sum to 684 > 400), then random others."""
    rng = np.random.default_rng(seed)
    m, n = 60, 400
    Hm = np.zeros((m, n), dtype=np.uint8)
    fresh = 0
    for r in range(m):
        D = RAGGED_DEGREES[r % len(RAGGED_DEGREES)]
        take = min(D, n - fresh, 8)                  # at most 8 fresh ones per check: the rest overlaps with other checks
        v = list(range(fresh, fresh + take))
        fresh += take
        pool = np.setdiff1d(np.arange(n), v)
        v += list(rng.choice(pool, D - take, replace=False))
        Hm[r, v] = 1
    assert fresh == n and (Hm.sum(axis=0) > 0).all()
    return Hm


# name -> (generator, circulant size the layering must report, SNR in dB at which 0 < decoded < frames, iterations of the
# CPU check of that statement)
CASES = {
    "qc4x24z27": (lambda: quasi_cyclic(4, 24, 27, 1, 0.08), 27, 2.5),
    "qc6x32z64": (lambda: quasi_cyclic(6, 32, 64, 2), 64, 2.5),
    "qc2x10z300": (lambda: quasi_cyclic(2, 10, 300, 3), 300, 3.0),
    # the SNR of `ragged` is chosen from the restatement alone (layered_minsum and layered_sumproduct_exact with host_phi on 200
    # frames, 25 iterations: both decode some frames and fail others there; test_layered_wide.py asserts it)
    "ragged": (ragged_60x400, 0, 3.0),
}

_made = {}


def matrix(name):
    if name not in _made:
        _made[name] = CASES[name][0]()
        _made[name].setflags(write=False)
    return _made[name]


KNIFE_DEGREES = [9, 12, 16, 17, 24, 25, 31, 32]


def knife_edge_case_wide(phi, snr, frames, seed, msg_dtype=np.float32):
    """layered_ref.knife_edge_case on checks of degree 9, 12, 16, 17, 24, 25, 31, 32 over disjoint variables (n = 166): frame f
    targets check f mod 8 and a random edge j of it; the other symbols are positive, and symbol j is set so that its scaled LLR is
    exactly -out_j (f // 8 even: P'_j = +0) or -nextafter(out_j, inf) (f // 8 odd: P'_j < 0), out_j being the message
    spa_messages sends to j.  With 9 to 32 terms the fp32 prefix / suffix sums round at almost every add, so an out_j formed
    in another order — across a chunk boundary, say — is off by an ulp in a good share of the frames.  max_iter = 1.
    The other LLRs are 2 ... 6 (scaled): 8 to 31 terms phi(x) of 0.02 ... 0.36 each sum to 1 ... 4, where phi is steep enough
    for the sum's last bits to show in out_j.
    -> Hm [8, 166], y [F', 166] float64, knife [F'] the variable on the edge, high [F'] bool: the second kind"""
    degs = KNIFE_DEGREES
    n = sum(degs)
    Hm = np.zeros((len(degs), n), dtype=np.uint8)
    first = np.concatenate([[0], np.cumsum(degs)])
    for c, D in enumerate(degs):
        Hm[c, first[c]:first[c] + D] = 1
    rng = np.random.default_rng(seed)
    var = _variance(snr)
    y = rng.uniform(2.0, 6.0, size=(frames, n)) * var / 2.0 / float(LOG2E_F32)
    kind = np.zeros(frames, dtype=bool)
    knife = np.zeros(frames, dtype=np.int64)
    keep = np.zeros(frames, dtype=bool)
    for f in range(frames):
        c = f % len(degs)
        D = degs[c]
        j = int(rng.integers(0, D))
        q = (channel_llr_f32(y[f, first[c]:first[c] + D], snr) * LOG2E_F32)[None, :]
        out = spa_messages(q, phi, msg_dtype)[0, j]                                     # (> 0: every q is positive)
        high = (f // len(degs)) % 2 == 1
        target = np.nextafter(out, np.float32(np.inf)) if high else out
        t0 = np.float32(np.float64(target) / np.float64(LOG2E_F32))
        for t in (t0, np.nextafter(t0, np.float32(0)), np.nextafter(t0, np.float32(np.inf))):
            ys = -(np.float64(t) * var / 2.0)
            if channel_llr_f32(np.array([ys]), snr)[0] * LOG2E_F32 == -target:
                y[f, first[c] + j] = ys
                keep[f], kind[f], knife[f] = True, high, first[c] + j
                break
    return Hm, y[keep], knife[keep], kind[keep]
