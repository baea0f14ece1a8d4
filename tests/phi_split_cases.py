"""Batches that put phi inputs of the fused fixed-work sum-product sweeps onto the thresholds of the one-series phi (bp_core.inc:
BpPass::word_c / word_v, SPLIT) to the bit, in units that are uniform but for one lane, used by tests/test_phi_split_gpu.py.
NumPy only; the check-side batch is handed the device's phi.  All symbols are positive (the all-zero codeword is received without
an error), so every frame latches at its first syndrome and its wavefront runs the split sweeps from the second sweep on.  Every
frame stands twice in a row: the two frames of a wavefront at 32 lanes are then the same kind.  The expectation is the
ACG_BP_NO_PHISPLIT=1 run of the same library.

A channel value becomes an LLR of known bits: llr = fl32(fl64(y) * (2 / sigma^2 * log2(e))) (one double multiply, bp_core.inc:
chan_llr); the symbol for a wanted fp32 value is found by dividing and checked by multiplying back.

Variable side (variable_batch).  The layout deals the variables to the passes in the stable order of falling degree
(code.cpp: bp_layout_build), L to a pass, so the lanes of pass 0 are the L variables of highest degree: the 32-lane units of its
edge rows hold them and nothing else.  They get LLR 8; every other variable gets 2^-40, whose phi is about 41.5, so that any two of
them in a check's exclude-self sum pass 66 and the check's message is a zero.  One variable s of pass 0 whose checks all hold two
such neighbours then receives zeros only: the phi input of each of its edge rows is |LLR_s| exactly, in every sweep.  Its unit
mates receive non-negative messages and stay at 8 or above.  So a unit is "every lane >= 2" but for the lane of s, which carries in
turn 2.0 (the unit takes phi_large, s on the threshold itself), its fp32 neighbour below (s alone makes the wavefront take the full
phi) and above, 1.0 and its neighbours, NaN (fails the compare: full phi), a finite value >= 66 and +inf (both off the
evaluating lanes: the unit stays uniform), 8 (the control), and +0 (an LLR of zero decides for a one, so these two frames never
latch: the wavefront that stays on the sweeps without the split).

Check side (check_batch; codes with a degree-1 variable: H05 and optimalH of the default codes).  Every variable of degree two or more gets
LLR 70: its messages are +0 in every sweep, because what it receives is non-negative.  A degree-1 variable's message never changes:
phi(|LLR|).  The other rows of its check therefore see the exclude-self sum phi(|LLR|) + 0 + ... exactly, a row "with one
non-saturated input".  Every degree-1 variable gets LLR 4 (sum about 0.18: at or below 1), but for one, a, whose LLR is chosen with
the device's phi so that phi(|LLR_a|) is, to the bit, 1.0 (the unit takes phi_small, a on the threshold itself), its neighbour above
(a alone makes the wavefront take the full phi) and below, 2.0, and — through LLR_a = NaN, 70, 0, 2^-70 — NaN, +0, +inf and a finite
value >= 66 (the full path's saturation select; with LLR_a = 0 the frame decides for a one and never latches).  Where no fp32 LLR gives the wanted sum exactly the nearest is taken (`hits` says
which).  The phi memo of the absorbed passes would answer these rows from its one entry, so the test runs this batch under
ACG_BP_NO_PHIMEMO=1 as well, where the rows evaluate phi."""
import numpy as np

END_SNR = -2.0
LOG2E = 1.44269504088896341


def channel_scale(snr):
    """the double the kernels multiply a symbol with: inv_var2 * Dom<float>::scale"""
    var = 10.0 ** (-snr / 10.0) / 2.0
    return (2.0 / var) * LOG2E


def symbol_for(llr32, k):
    """float64 symbol y with fl32(y * k) == llr32"""
    llr32 = np.float32(llr32)
    if not np.isfinite(llr32) or llr32 == 0:
        return float(llr32)
    y = float(np.float64(llr32) / k)
    for cand in (y, np.nextafter(y, np.inf), np.nextafter(y, -np.inf)):
        if np.float32(np.float64(cand) * k) == llr32:
            return float(cand)
    raise AssertionError("no symbol for %r" % llr32)


def _neighbours(x):
    x = np.float32(x)
    return [x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))]


def variable_batch(Hm, L):
    """-> (y [frames][n] float64, s, the values of s in frame order)"""
    Hm = np.asarray(Hm) != 0
    m, n = Hm.shape
    k = channel_scale(END_SNR)
    deg = Hm.sum(axis=0)
    order = np.argsort(-deg, kind="stable")
    pass0 = set(int(v) for v in order[:L])
    s = None
    for v in order[:L]:
        checks = np.nonzero(Hm[:, v])[0]
        if all(sum(1 for u in np.nonzero(Hm[c])[0] if int(u) not in pass0) >= 2 for c in checks):
            s = int(v)
            break
    assert s is not None, "no variable of pass 0 whose checks all hold two variables of other passes"
    values = _neighbours(2.0) + _neighbours(1.0) + [np.float32(np.nan), np.float32(0.0), np.float32(70.0), np.float32(np.inf), np.float32(8.0)]
    base = np.full(n, symbol_for(2.0 ** -40, k))
    base[sorted(pass0)] = symbol_for(8.0, k)
    y = np.repeat(base[None, :], 2 * len(values), axis=0)
    for i, val in enumerate(values):
        y[2 * i:2 * i + 2, s] = symbol_for(val, k)
    return np.ascontiguousarray(y), s, values


def check_batch(Hm, phi):
    """phi: float32 array -> float32 array, the device's Dom<float>::phi.  -> (y, a, [(wanted sum, LLR of a, exact?)]) or None
    for a code without a degree-1 variable"""
    Hm = np.asarray(Hm) != 0
    m, n = Hm.shape
    k = channel_scale(END_SNR)
    deg = Hm.sum(axis=0)
    d1 = np.nonzero(deg == 1)[0]
    if len(d1) == 0:
        return None
    a = int(d1[len(d1) // 2])
    hits = []
    for want in _neighbours(1.0) + [np.float32(2.0)]:
        x0 = phi(np.array([want], dtype=np.float32))[0]          # phi is its own inverse up to rounding
        cand = (x0.view(np.uint32).astype(np.int64) + np.arange(-4096, 4097)).astype(np.uint32).view(np.float32)
        got = phi(cand)
        best = int(np.argmin(np.abs(got.astype(np.float64) - np.float64(want))))
        hits.append((want, cand[best], bool(got[best] == want)))
    llrs = [h[1] for h in hits] + [np.float32(np.nan), np.float32(70.0), np.float32(0.0), np.float32(2.0 ** -70), np.float32(4.0)]
    base = np.full(n, symbol_for(70.0, k))
    base[d1] = symbol_for(4.0, k)
    y = np.repeat(base[None, :], 2 * len(llrs), axis=0)
    for i, val in enumerate(llrs):
        y[2 * i:2 * i + 2, a] = symbol_for(val, k)
    return np.ascontiguousarray(y), a, hits
