"""numpy restatement of ordered-statistics decoding as include/acg_ldpc.h states it ("OSD", algo = ACG_LDPC_OSD) and osd.hip
implements it: order 0 and 1 on int16 soft values.  Every value is an integer, so the device must return the same word, flag
and iters for every frame.

  z_v = (s_v < 0), r_v = min(|s_v|, 32767), key_v = (r_v << 16) | v ascending.  Scanning the variables in that order, v joins
  the pivot set B iff column v of H is independent over GF(2) of the columns already in B.  I = the complement of B.  x_T (T a
  subset of I) is the codeword with x_v = z_v ^ [v in T] on I; M(x) = sum_v r_v [x_v != z_v].  Order 0: x_{}.  Order 1: the
  minimiser over x_{} and x_{j}, j in I; ties: x_{} first, then the lowest j.  ok = 1, iters = |T| of the winner.

Written for clarity, on dense 0/1 arrays, one frame at a time: the elimination is plain row reduction."""
import numpy as np


def soft_values(y):
    """the symbol entrance's quantiser: y32 = the symbol as float (a double is rounded to nearest), s = clamp(truncf(y32 * 4096),
    -32767, 32767), NaN -> 0, +-inf -> +-32767.  float32 or float64 symbols of any shape -> int16"""
    with np.errstate(over="ignore", invalid="ignore"):
        y32 = np.asarray(y).astype(np.float32)
        t = y32 * np.float32(4096.0)
    t = np.where(np.isnan(t), np.float32(0), t)
    t = np.clip(t, np.float32(-32767.0), np.float32(32767.0))
    return np.trunc(t).astype(np.int16)


def reliabilities(s):
    s = np.asarray(s).astype(np.int64)
    return (s < 0).astype(np.uint8), np.minimum(np.abs(s), 32767)


def order_of(r):
    """the variables in ascending key (r_v << 16 | v): least reliable first, ties by the lower v"""
    n = len(r)
    return np.argsort((r.astype(np.int64) << 16) | np.arange(n), kind="stable")


def reduce_on(Hm, order):
    """row-reduce a copy of H scanning the columns in `order` -> (H_red, piv): piv[r] = the pivot column of row r, -1 for a row
    that stays without one; the pivot columns of H_red are unit vectors"""
    A = (np.asarray(Hm) != 0).astype(np.uint8)
    m = A.shape[0]
    piv = np.full(m, -1, dtype=np.int64)
    free = np.ones(m, dtype=bool)
    for v in order:
        rows = np.flatnonzero(A[:, v].astype(bool) & free)
        if not len(rows):
            continue          # dependent on the columns already in B
        p = rows[0]           # (which free row serves does not change the result)
        others = np.flatnonzero(A[:, v])
        others = others[others != p]
        A[others] ^= A[p]
        piv[p] = v
        free[p] = False
        if not free.any():
            break
    return A, piv


def _reduced(Hm, s):
    """what both orders share for one frame: z, r, the pivot column and the reduced row of every used row, sigma"""
    z, r = reliabilities(s)
    A, piv = reduce_on(Hm, order_of(r))
    used = piv >= 0
    pc = piv[used]                       # pivot column of every used row
    Ar = A[used].astype(np.int64)        # H_red restricted to the used rows (the others are all-zero)
    sigma = (Ar @ z.astype(np.int64)) & 1
    return z, r, pc, Ar, sigma


def _finish(parts, order):
    z, r, pc, Ar, sigma = parts
    rp = r[pc]
    in_B = np.zeros(len(z), dtype=bool)
    in_B[pc] = True
    best_M, best_j = int((sigma * rp).sum()), -1
    if order == 1:
        I = np.flatnonzero(~in_B)
        M = r[I] + ((sigma[:, None] ^ Ar[:, I]) * rp[:, None]).sum(axis=0)    # M(x_{j}) of every j in I, ascending j
        if len(I) and M.min() < best_M:  # strict: x_{} wins a tie; argmin: then the lowest j
            best_M, best_j = int(M.min()), int(I[np.argmin(M)])
    x = z.copy()
    flip = sigma.copy()
    if best_j >= 0:
        x[best_j] ^= 1
        flip ^= Ar[:, best_j]
    x[pc] = z[pc] ^ flip.astype(np.uint8)
    return x, (1 if best_j >= 0 else 0), best_M


def osd_frame(Hm, s, order):
    """one frame -> word [n] uint8, iters, metric"""
    if order not in (0, 1):
        raise ValueError("order above 1 is out of scope")
    return _finish(_reduced(Hm, s), order)


def osd(Hm, s, order):
    """s: frames x n integer soft values -> words [F, n] uint8, iters [F] int32, metric [F] int64  (ok = 1 for every frame)"""
    if order not in (0, 1):
        raise ValueError("order above 1 is out of scope")
    return osd_orders(Hm, s, (order,))[order]


def osd_orders(Hm, s, orders=(0, 1)):
    """osd() for several orders on one elimination per frame -> {order: (words, iters, metric)}"""
    s = np.atleast_2d(np.asarray(s))
    F, n = s.shape
    out = {o: (np.zeros((F, n), dtype=np.uint8), np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int64)) for o in orders}
    for f in range(F):
        parts = _reduced(Hm, s[f])
        for o in orders:
            out[o][0][f], out[o][1][f], out[o][2][f] = _finish(parts, o)
    return out


def metric_of(word, s):
    z, r = reliabilities(s)
    return int(r[np.asarray(word) != z].sum())


def information_set(Hm, s):
    """the boolean mask of I for one frame"""
    _, r = reliabilities(s)
    _, piv = reduce_on(Hm, order_of(r))
    mask = np.ones(len(r), dtype=bool)
    mask[piv[piv >= 0]] = False
    return mask


def cascade(first, Hm, order):
    """the by-hand composition of a two-stage decode with OSD behind a first stage that yields soft values: first = (bits, ok,
    iters, soft) of the first stage on every frame -> (bits, ok, iters, stage); a frame with ok = 0 gets OSD's answer on its soft
    values"""
    bits, ok, iters, soft = (np.array(x) for x in first)
    stage = np.ones(len(ok), dtype=np.uint8)
    fail = np.flatnonzero(ok == 0)
    if len(fail):
        w, it, _ = osd(Hm, soft[fail], order)
        bits[fail], ok[fail], iters[fail], stage[fail] = w, 1, it, 2
    return bits, ok, iters, stage
