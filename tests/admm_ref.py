"""numpy restatement of the QP-ADMM decoder (DecodeQPADMM, qp_admm.h:104-178) in a chosen storage type T, operation for
operation and vectorised over frames.  T = float64 is the reference itself (tests/test_admm_ref.py ties it to
`oracle.qpadmm_decode`: word, flag and sweep count); T = float32 is what the fp32 instances of the QP-ADMM kernels
(csrc/admm_kernels.hip, csrc/admm_streamed.hip) have to compute, bit for bit.

Built from the QP-ADMM problem in the reference's construction order (`admm_problem`, qp_admm.h:13-102; checked against
`oracle.admm_matrix`), never from the layout tables of csrc/code.cpp.

  q          q_i = T(2 * double(y_i) / var), formed in double and rounded once (y: float64 or float32 symbols);
             auxiliary variables have q = 0
  constants  alpha, mu, eps_stop rounded to T once; alpha / 2 in T;
             inv_i = T(-1 / (2 * ((mu * e_i - alpha) / 2))) formed in DOUBLE from the double alpha, mu and rounded once
  v-update   B = q_i + alpha/2, then in construction order B += coef * (yl_j + mu * (z_j - b_j)): the subtraction, the
             product and the sum are each rounded to T, the +-1 multiply is exact; v = B * inv (a multiply, never a divide);
             v = v < 0 ? 0 : v; v = 1 < v ? 1 : v   (std::max / std::min of qp_admm.h:140-141: a NaN stays)
  row phase  r_j = b_j, then r_j -= coef * v_i in ascending variable order; z = (r - yl) > 0 ? r - yl : 0 and
             yl = (yl - r) > 0 ? yl - r : 0   (a NaN gives 0)
  residual   the terms (z - r)^2 are formed in T.  The kernels add them up in a tree whose shape follows the placement of
             the constraint groups on lanes, which is partly annealed, so the order of that sum is not restated: the T squares
             are summed in float64 (S) and the frame stops when S < T(eps).  band[f] = min over the sweeps the frame ran of
             |S / T(eps) - 1|: a kernel may stop on another sweep only where its own sum falls on the other side of eps,
             i.e. only for band[f] below the relative error of a float32 sum of n_con non-negative terms (BAND below)
  exit       bits = !(v <= 0.5); iters = sweeps executed; the guard e_min * mu <= alpha (in double) returns zeros, ok = 0;
             a budget of 0 returns (q > 0), ok = 1; early_exit=False or eps <= 0 runs every sweep (band = inf)

No transcendental, no fused multiply-add: numpy's float32 arithmetic restates the fp32 sweep exactly."""
import numpy as np


def llr_variance(snr):
    return 10.0 ** (-(snr / 10.0)) / 2.0        # channel.h:12


def band_width(n_con):
    """Any-order float32 summation of n non-negative terms has relative error <= (n - 1) * 2^-24 to first order; doubled."""
    return 2.0 * n_con * 2.0 ** -24


def admm_problem(H):
    """ConstructADMMProblem without q (qp_admm.h:13-102) -> (col_ptr, con, coef, b): per variable its (row, +-1) entries in
    construction order, as oracle.admm_matrix returns them."""
    H = np.asarray(H) != 0
    m, n = H.shape
    n_aux = int(sum(max(int(r.sum()) - 3, 0) for r in H))
    lists = [[] for _ in range(n + n_aux)]
    b = []

    def three(i, j, h):                           # qp_admm.h:34-57
        nb = len(b)
        b.extend([0.0, 0.0, 0.0, 2.0])
        for w, var in enumerate((i, j, h)):
            for r in range(3):
                lists[var].append((nb + r, 1.0 if r == w else -1.0))
            lists[var].append((nb + 3, 1.0))

    pos = n
    for row in H:
        idx = np.flatnonzero(row).tolist()
        d = len(idx)
        if d == 0:
            continue
        if d == 1:                                # qp_admm.h:70-74
            lists[idx[0]].append((len(b), 1.0))
            b.append(0.0)
        elif d == 2:                              # qp_admm.h:75-83
            nb = len(b)
            b.extend([0.0, 0.0])
            lists[idx[0]] += [(nb, 1.0), (nb + 1, -1.0)]
            lists[idx[1]] += [(nb, -1.0), (nb + 1, 1.0)]
        else:                                     # qp_admm.h:84-91
            last = idx[0]
            for j in range(1, d - 2):
                three(last, idx[j], pos)
                last = pos
                pos += 1
            three(last, idx[d - 2], idx[d - 1])
    col_ptr = np.zeros(len(lists) + 1, dtype=np.int32)
    col_ptr[1:] = np.cumsum([len(x) for x in lists])
    flat = [e for x in lists for e in x]
    con = np.array([e[0] for e in flat], dtype=np.int32)
    coef = np.array([e[1] for e in flat], dtype=np.float64)
    return col_ptr, con, coef, np.array(b, dtype=np.float64)


class _Steps:
    """a ragged list per node, turned into steps: step k touches the nodes that have a k-th entry"""

    def __init__(self, owner, other, coef, n_owner, dtype):
        order = np.argsort(owner, kind="stable")             # entries of one owner stay in the order given
        owner, other, coef = owner[order], other[order], coef[order]
        start = np.searchsorted(owner, np.arange(n_owner))
        rank = np.arange(len(owner)) - start[owner]
        self.steps = []
        for k in range(int(rank.max()) + 1 if len(rank) else 0):
            sel = rank == k
            self.steps.append((owner[sel], other[sel], coef[sel].astype(dtype)))


# deliberately wrong variants, for tests/test_admm_ref.py only: they show that a frame set tells the true sweep from these
MUTANTS = ("reversed_terms", "fused_term", "inv_from_f32", "divide", "q_in_f32")


def qpadmm_ref(H, y, snr, alpha, mu, max_iter, eps_stop, dtype, early_exit=True, problem=None, mutant=None):
    """-> (bits [F, n] uint8, ok [F] uint8, iters [F] int32, band [F] float64).  problem: (col_ptr, con, coef, b) of H when
    the caller has it already (admm_problem(H) or oracle.admm_matrix(H))."""
    assert mutant is None or mutant in MUTANTS
    T = np.dtype(dtype).type
    H = np.asarray(H)
    n = H.shape[1]
    y = np.asarray(y)
    if y.dtype != np.float32:
        y = y.astype(np.float64)
    y = y.reshape(-1, n)
    F = y.shape[0]
    col_ptr, con, coef, b = problem if problem is not None else admm_problem(H)
    n_var, n_con = len(col_ptr) - 1, len(b)
    bits = np.zeros((F, n), dtype=np.uint8)
    iters = np.zeros(F, dtype=np.int32)
    band = np.full(F, np.inf)
    e = np.diff(col_ptr).astype(np.float64)                  # sum of coef^2, qp_admm.h:94-99
    e_min = min(1e9, e.min()) if n_var else 1e9
    if e_min * float(mu) <= float(alpha):                    # qp_admm.h:112-114
        return bits, np.zeros(F, dtype=np.uint8), iters, band
    ok = np.ones(F, dtype=np.uint8)
    var = llr_variance(snr)
    with np.errstate(all="ignore"):
        q = np.zeros((F, n_var), dtype=T)
        if mutant == "q_in_f32":
            q[:, :n] = T(2) * y.astype(T) / T(var)
        else:
            q[:, :n] = (2 * y.astype(np.float64) / var).astype(T)
        if max_iter <= 0:                                    # qp_admm.h:116-119,166-175
            return (q[:, :n] > 0).astype(np.uint8), ok, iters, band
        aT, mT, epsT = T(alpha), T(mu), T(eps_stop)
        half = aT / T(2)
        if mutant == "inv_from_f32":
            inv = T(-1) / (T(2) * ((mT * e.astype(T) - aT) / T(2)))
        else:
            inv = (-1.0 / (2 * ((float(mu) * e - float(alpha)) / 2))).astype(T)
        bT = b.astype(T)
        owner = np.repeat(np.arange(n_var), np.diff(col_ptr))
        if mutant == "reversed_terms":
            rev = np.arange(len(con))[::-1]
            vsteps = _Steps(owner[rev], con[rev], coef[rev], n_var, T).steps
        else:
            vsteps = _Steps(owner, con, coef, n_var, T).steps
        rsteps = _Steps(con, owner, coef, n_con, T).steps    # entries are listed by ascending variable already
        stop_rule = bool(early_exit) and float(eps_stop) > 0
        act = np.arange(F)                                   # frames still sweeping; state rows follow `act`
        z = np.zeros((F, n_con), dtype=T)
        yl = np.zeros((F, n_con), dtype=T)
        v = np.zeros((F, n_var), dtype=T)
        for it in range(1, int(max_iter) + 1):
            if mutant == "fused_term":                       # one rounding for mu * (z - b) + yl
                term = (mT.astype(np.float64) * (z - bT).astype(np.float64) + yl.astype(np.float64)).astype(T)
            else:
                term = yl + mT * (z - bT)
            B = q[act] + half
            for vi, cj, cf in vsteps:
                B[:, vi] = B[:, vi] + cf * term[:, cj]
            v = (B / (T(1) / inv)) if mutant == "divide" else B * inv
            v = np.where(v < 0, T(0), v)
            v = np.where(1 < v, T(1), v)
            r = np.broadcast_to(bT, z.shape).copy()
            for cj, vi, cf in rsteps:
                r[:, cj] = r[:, cj] - cf * v[:, vi]
            zn = r - yl
            yn = yl - r
            z = np.where(zn > 0, zn, T(0))
            yl = np.where(yn > 0, yn, T(0))
            d = z - r
            sq = d * d
            iters[act] = it
            done = np.zeros(len(act), dtype=bool)
            if stop_rule:
                S = sq.astype(np.float64).sum(axis=1)
                band[act] = np.fmin(band[act], np.abs(S / float(epsT) - 1.0))   # a NaN residual never stops in any order
                done = S < float(epsT)                       # qp_admm.h:161-163
            if it == max_iter:
                done[:] = True
            if done.any():
                bits[act[done]] = ~(v[done][:, :n] <= 0.5)   # qp_admm.h:166-175
                keep = ~done
                act, z, yl = act[keep], z[keep], yl[keep]
                if len(act) == 0:
                    break
    return bits, ok, iters, band
