"""numpy restatement of the FLOODING normalised min-sum kernels, operation for operation, vectorised over frames and over
nodes of equal degree — the repo's OWN restatement: min-sum is not in the reference, so what this checks is that
the kernels do what their sources say; `oracle.minsum_decode` (plain double, other summation order, no hard bit in the
magnitude LSB) is the independent yardstick this one is tied to in tests/test_minsum_ref.py.

Written from csrc/bp_core.inc (BpPass::check min-sum branch, var_at, var_init, chan_llr; fused and workgroup-per-frame
kernels), csrc/bp_streamed.hip (StreamPass) and csrc/bp_pair.hip (pair_check / pair_var):

  storage type T    float32 / float64 (bp_core.inc, bp_streamed.hip), float16 (bp_pair.hip)
  domain            every LLR-domain quantity times Dom<T>::scale: log2(e) for float32, 1 for float64 and float16
  channel LLR       double symbols  T(2 * y / var * scale), left to right in double   (float16: half(float(2 * y / var)))
                    float symbols   T(double(y) * (inv_var2 * scale)), inv_var2 = 2.0 / var as decode.hip fill_channel forms it
                                    (float16: half(float(double(y) * inv_var2)))
  message word      sign | magnitude with its LSB cleared | LSB = posterior hard decision of the sending variable
  first sweep       every outgoing word of a variable is |llr| (LSB cleared), sign = hard = (llr <= 0)
  check sweep       m1, m2 = the two smallest magnitudes of the check's edges (padding takes no part, a tie gives m2 == m1),
                    m1s = T(scale) * m1, m2s = T(scale) * m2, each rounded once; edge j receives m2s where mag[j] == m1, else
                    m1s, with the XOR of the other edges' signs; a one-variable check sends inf * scale.  The LSB of the product
                    is NOT cleared.  The streamed engine selects by arg-min index (strict <, so the first of tied edges) and
                    scales the selected minimum per edge: a tie makes m2 == m1 and the products are the same two numbers, so
                    the values are identical.  The syndrome bit of a check is the XOR of the hard bits riding in its words.
  variable sweep    edges in col_edge order (code.cpp: the variable's checks ascending); pre[k] = running prefix sum from +0,
                    total = llr + s, hard = (total <= 0), x_k = llr + (pre[k] + suf) with suf accumulated from the last edge
                    down; outgoing word |x_k| (LSB cleared), sign (x_k <= 0).  float16: every sum rounded to half once (numpy
                    forms a + b and a * b of two halves in float32 and rounds: 24 >= 2 * 11 + 2 bits, so the double rounding is
                    innocuous and the result is the correctly rounded one v_pk_add_f16 / v_pk_mul_f16 give).
  exit              the syndrome of the hard decisions of sweep `it` is taken in the check sweep that follows; a frame converges
                    at the first it in 1..max_iter with zero syndrome (bp.h:183-199) and its word is latched there; fixed work
                    (early_exit=False) keeps sweeping and returns the latched word; a failed frame returns the empty word and
                    max_iter; max_iter = 0 never converges.

There is no transcendental and no multiply-add in any of this, so equality with the kernels is asked bit for bit (finite
symbols; NaN propagation through v_med3_f32 / v_pk_min_f16 is not restated)."""
import numpy as np

LOG2E = 1.44269504088896341        # Dom<float>::scale

_UINT = {np.dtype(np.float16): np.uint16, np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}


def llr_variance(snr):
    return 10.0 ** (-(snr / 10.0)) / 2.0        # channel.h:12; decode.hip fill_channel


def channel_llr(y, snr, dtype):
    """y: float64 symbols (decode_batch) or float32 symbols (decode_batch_f32, the Monte-Carlo kernels) -> LLRs of type T"""
    dtype = np.dtype(dtype)
    var = llr_variance(snr)
    dom = LOG2E if dtype == np.float32 else 1.0
    if y.dtype == np.float32:
        inv_var2 = 2.0 / var
        d = y.astype(np.float64) * (inv_var2 * dom)
    else:
        d = 2 * y.astype(np.float64) / var * dom
    if dtype == np.float16:
        with np.errstate(over="ignore"):
            return d.astype(np.float32).astype(np.float16)      # two roundings, as the kernel's (float) then (_Float16)
    return d.astype(dtype)


class Graph:
    """edges numbered check-major (check ascending, variable ascending inside a check); nodes grouped by degree"""

    def __init__(self, Hm):
        Hm = (np.asarray(Hm) != 0)
        self.m, self.n = Hm.shape
        ci, vi = np.nonzero(Hm)                  # row-major: exactly the check-major edge order
        self.E = len(ci)
        self.edge_var = vi
        cdeg = Hm.sum(axis=1)
        vdeg = Hm.sum(axis=0)
        cstart = np.concatenate([[0], np.cumsum(cdeg)])[:-1]
        self.checks = []                          # (degree, edge ids [count, degree])
        for d in np.unique(cdeg):
            if d == 0:
                continue                          # an empty row: no message, syndrome bit 0
            ids = np.nonzero(cdeg == d)[0]
            self.checks.append((int(d), cstart[ids][:, None] + np.arange(d)[None, :]))
        self.check_vars = [vi[eid] for _, eid in self.checks]      # per degree group: the checks' variables [count, degree]
        order = np.argsort(vi, kind="stable")     # per variable: its edges with the check ascending (col_edge order)
        vstart = np.concatenate([[0], np.cumsum(vdeg)])[:-1]
        self.vars = []                            # (degree, variable ids [count], edge ids [count, degree])
        for d in np.unique(vdeg):
            if d == 0:
                continue                          # an isolated variable: estimate() stays the channel LLR
            ids = np.nonzero(vdeg == d)[0]
            self.vars.append((int(d), ids, order[vstart[ids][:, None] + np.arange(d)[None, :]]))


def _mag(x, U):
    """|x| with the LSB cleared (the hard bit's place), as a value of x's own type"""
    bits = x.dtype.itemsize * 8
    return (x.view(U) & U((1 << (bits - 1)) - 2)).view(x.dtype)


def flooding_minsum(Hm, y, snr, max_iter, scale, dtype=np.float32, early_exit=True, fault=None):
    """Hm: m x n 0/1 (or a Graph); y: frames x n symbols, float64 or float32 (the dtype picks the kernel's LLR path).
    dtype: storage type T of the kernel restated.  fault: a hook for showing that a comparison bites — fault(d, out, m1s, m2s)
    may alter the magnitudes `out` [frames, checks, d] the checks of degree d send; never set by a test that judges a kernel.
    -> bits [F, n] uint8 (zeros for failed frames), ok [F] uint8, iters [F] int32"""
    g = Hm if isinstance(Hm, Graph) else Graph(Hm)
    T = np.dtype(dtype)
    U = _UINT[T]
    y = np.asarray(y)
    F, n = y.shape
    assert n == g.n
    sc = np.float32(scale).astype(T)             # DecodeArgs::ms_scale is a float; the kernels convert it to T
    LLR = channel_llr(y, snr, T)
    INF = T.type(np.inf)

    bits = np.zeros((F, n), dtype=np.uint8)
    ok = np.zeros(F, dtype=np.uint8)
    iters = np.zeros(F, dtype=np.int32)
    latched = np.zeros(F, dtype=bool)
    idx = np.arange(F)                            # the frames still being swept (rows of the state arrays below)

    # first variable -> check sweep (var_init): all mailboxes empty
    hard = LLR <= 0                               # [f, n] posterior hard decisions (ride in the LSB of the words)
    MAG = _mag(LLR, U)[:, g.edge_var]             # [f, E] magnitudes of the v->c words
    SGN = hard[:, g.edge_var]                     # [f, E] their sign bits (x <= 0)
    C2V = np.zeros((F, g.E), dtype=T)
    it = 0
    with np.errstate(invalid="ignore", over="ignore"):
        while len(idx):
            # ---- the check sweep also delivers the syndrome of the hard decisions riding in the words it reads
            bad = np.zeros(len(idx), dtype=bool)
            for cv in g.check_vars:
                bad |= np.logical_xor.reduce(hard[:, cv], axis=2).any(axis=1)
            conv = ~bad if 0 < it <= max_iter else np.zeros(len(idx), dtype=bool)     # bp.h:195 (max_iter = 0: never)
            lat = latched[idx]
            out_now = conv & ~lat
            finish = (conv & early_exit) | (it >= max_iter)
            fail_now = finish & ~conv & ~lat
            f = idx[out_now]
            bits[f] = hard[out_now]
            ok[f] = 1
            iters[f] = it
            iters[idx[fail_now]] = min(it, max_iter)          # (the word stays empty, bp.h:198)
            latched[idx[out_now | fail_now]] = True
            if finish.any():
                keep = ~finish
                idx, LLR, hard, MAG, SGN, C2V = idx[keep], LLR[keep], hard[keep], MAG[keep], SGN[keep], C2V[keep]
                if not len(idx):
                    break
            for d, eid in g.checks:
                a = MAG[:, eid]                   # [f, checks, d]
                s = SGN[:, eid]
                m1 = np.full(a.shape[:2], INF, dtype=T)
                m2 = np.full(a.shape[:2], INF, dtype=T)
                for j in range(d):                # new m2 = median(a, m1, m2), new m1 = min(m1, a)
                    m2 = np.minimum(m2, np.maximum(a[:, :, j], m1))
                    m1 = np.minimum(m1, a[:, :, j])
                m1s = sc * m1
                m2s = sc * m2
                out = np.where(a == m1[:, :, None], m2s[:, :, None], m1s[:, :, None])
                if fault is not None:
                    fault(d, out, m1s, m2s)
                neg = np.logical_xor.reduce(s, axis=2)[:, :, None] ^ s
                C2V[:, eid] = np.where(neg, -out, out)
            # ---- variable sweep
            for d, vid, eid in g.vars:
                llr = LLR[:, vid]
                c = C2V[:, eid]                   # [f, vars, d]
                pre = np.empty_like(c)
                s = np.zeros(llr.shape, dtype=T)
                for k in range(d):
                    pre[:, :, k] = s
                    s = s + c[:, :, k]
                hard[:, vid] = (llr + s) <= 0
                suf = np.zeros(llr.shape, dtype=T)
                x = np.empty_like(c)
                for k in range(d - 1, -1, -1):
                    x[:, :, k] = llr + (pre[:, :, k] + suf)
                    suf = suf + c[:, :, k]
                MAG[:, eid] = _mag(x, U)
                SGN[:, eid] = x <= 0
            it += 1
    return bits, ok, iters
