"""numpy restatement of the FLOODING SUM-PRODUCT kernels, operation for operation, vectorised over frames and over nodes of
equal degree — the repo's OWN restatement of what `bench.py` times.  The reference side is held by tests/test_gpu_parity.py
(hard outputs against the 80-bit oracle, soft messages within a tolerance); this one asks that the kernels do what their
sources say, to the last bit of every message word.  tests/test_spa_ref.py ties it to `oracle.bp_decode` on the CPU.

Written from csrc/bp_core.inc (BpPass::check, check_sat, check_abs, var_at, var_init, chan_llr; the wave-group kernel and,
through BpCore, the workgroup-per-frame kernel of bp_block.hip) and csrc/bp_streamed.hip (StreamPass, check_group / var_group,
RingPass).  Never from BpLayout or a table of code.cpp: the layout does not enter the arithmetic (an absorbed variable is its
check's last edge, where it is anyway as the highest column; padding rows add +0 to sums that are not negative).

  storage type T    float32 / float64
  domain            every LLR-domain and phi-domain quantity times Dom<T>::scale: log2(e) for float32, 1 for float64
  phi               handed in: an array of T -> an array of T, Dom<T>::phi in T's domain.  The device's own function on the GPU
                    (acg_ldpc_debug_phi_sat / acg_ldpc_debug_phi), a host stand-in on the CPU
  channel LLR       minsum_ref.channel_llr: the same two paths (double symbols, float symbols)
  message word      sign | magnitude with its LSB cleared | LSB = posterior hard decision of the sending variable
  first sweep       every outgoing word of a variable is phi(|llr|) (LSB cleared), sign = hard = (llr <= 0)
  check sweep       edges in row order (variables ascending): mag_j = the word without sign and LSB; pre_j = mag_0 + ... +
                    mag_{j-1} summed in that order from +0; suf = mag_{D-1} + ... + mag_{j+1} summed in THAT order from +0;
                    out_j = phi(pre_j + suf), sign bit replaced by the XOR of the other edges' sign bits; the LSB of phi's
                    result is NOT cleared.  A one-variable check sends phi(+0) = +inf.  An empty row sends nothing and has
                    syndrome 0.  The syndrome bit of a check is the XOR of the hard bits riding in its words.
  variable sweep    edges in col_edge order (the variable's checks ascending): pre_k = running prefix sum of the c->v words
                    from +0, s = their sum, total = llr + s, hard = (total <= 0); x_k = llr + (pre_k + suf), suf accumulated
                    from the last edge down from +0; outgoing word phi(|x_k|) (LSB cleared) | hard, sign (x_k <= 0).
                    NaN: every `<= 0` is false, as in the kernels; phi(NaN) is phi's business.
  exit              exactly minsum_ref's: the syndrome of the hard decisions of sweep `it` is taken in the check sweep that
                    follows; a frame converges at the first it in 1..max_iter with zero syndrome (bp.h:183-199) and its word is
                    latched there; fixed work (early_exit=False) keeps sweeping and returns the latched word; a failed frame
                    returns the empty word and max_iter; max_iter = 0 never converges.

Apart from phi every operation is an IEEE add, a compare or a bit operation (no multiply-add to contract), so with the device's
phi equality with the kernels is asked bit for bit."""
import numpy as np

from minsum_ref import _UINT, Graph, _mag, channel_llr

LN2 = 0.693147180559945309         # acg_ldpc_debug_bp_trace returns LN2 * double(word) for the float32 engines


def host_phi64(x):
    """CPU stand-in for Dom<double>::phi (phi_f of bp_core.inc), natural domain: the same three branches with numpy's libm"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore", under="ignore"):
        t = np.exp(-x)
        big = np.log1p(2.0 * t / (1.0 - t))
        small = -np.log(np.tanh(0.5 * x))
        return np.where(x >= 45.747713916956390, 0.0, np.where(x >= 1.0, big, small))


def flooding_sumproduct(Hm, y, snr, max_iter, phi, dtype=np.float32, early_exit=True, trace_at=None, fault=None):
    """Hm: m x n 0/1 (or a minsum_ref.Graph); y: frames x n symbols, float64 or float32 (the dtype picks the kernel's LLR
    path).  dtype: storage type T of the kernel restated.  phi: array of T -> array of T (same shape).
    trace_at = k >= 1: run k full iterations WITHOUT the exit test and return additionally (c2v, v2c, post): the c->v words
    [F, E] of T after the k-th check sweep, the v->c words [F, E] of T (hard bit in the LSB) after the k-th variable sweep and
    the totals llr + s [F, n] of T that sweep formed — per edge check-major with variables ascending, as
    acg_ldpc_debug_bp_trace numbers them.  max_iter is then ignored.
    fault: a hook for showing that a comparison bites — fault(site, d, out, **context) may alter the array `out` in place:
        "check_mag"  out = mag [frames, checks, d]; raw = the same words with the hard bit still in the LSB
        "check_sum"  out = the exclude-self sums pre_j + suf [frames, checks, d]; mag
        "check_out"  out = phi of those sums [frames, checks, d]
        "var_total"  out = llr + s [frames, variables]; llr, c as below
        "var_x"      out = x_k [frames, variables, d]; llr [frames, variables], c = the c->v words [frames, variables, d]
        "var_mag"    out = phi(|x_k|) with the LSB cleared [frames, variables, d]; p = phi(|x_k|) as phi gave it
    never set by a test that judges a kernel.
    -> bits [F, n] uint8 (zeros for failed frames), ok [F] uint8, iters [F] int32 (and the trace)"""
    g = Hm if isinstance(Hm, Graph) else Graph(Hm)
    T = np.dtype(dtype)
    U = _UINT[T]
    SIGN = U(1 << (T.itemsize * 8 - 1))
    y = np.asarray(y)
    F, n = y.shape
    assert n == g.n and T in (np.float32, np.float64)
    assert trace_at is None or trace_at >= 1
    LLR = channel_llr(y, snr, T)

    def f(x):
        out = phi(x)
        assert out.dtype == T and out.shape == x.shape
        return out

    bits = np.zeros((F, n), dtype=np.uint8)
    ok = np.zeros(F, dtype=np.uint8)
    iters = np.zeros(F, dtype=np.int32)
    latched = np.zeros(F, dtype=bool)
    idx = np.arange(F)                            # the frames still being swept (rows of the state arrays below)

    with np.errstate(invalid="ignore", over="ignore"):
        # first variable -> check sweep (var_init): all mailboxes empty, one word per variable
        hard = LLR <= 0                           # [f, n] posterior hard decisions (ride in the LSB of the words)
        MAG = _mag(f(np.abs(LLR)), U)[:, g.edge_var]      # [f, E] magnitudes of the v->c words
        SGN = hard[:, g.edge_var]                 # [f, E] their sign bits (x <= 0)
        C2V = np.zeros((F, g.E), dtype=T)
        POST = LLR + T.type(0)                    # (an isolated variable: estimate() stays the channel LLR)
        it = 0
        while len(idx):
            if trace_at is None:
                # ---- the check sweep also delivers the syndrome of the hard decisions riding in the words it reads
                bad = np.zeros(len(idx), dtype=bool)
                for cv in g.check_vars:
                    bad |= np.logical_xor.reduce(hard[:, cv], axis=2).any(axis=1)
                conv = ~bad if 0 < it <= max_iter else np.zeros(len(idx), dtype=bool)     # bp.h:195 (max_iter = 0: never)
                lat = latched[idx]
                out_now = conv & ~lat
                finish = (conv & early_exit) | (it >= max_iter)
                fail_now = finish & ~conv & ~lat
                fr = idx[out_now]
                bits[fr] = hard[out_now]
                ok[fr] = 1
                iters[fr] = it
                iters[idx[fail_now]] = min(it, max_iter)          # (the word stays empty, bp.h:198)
                latched[idx[out_now | fail_now]] = True
                if finish.any():
                    keep = ~finish
                    idx, LLR, hard, MAG, SGN, C2V, POST = (a[keep] for a in (idx, LLR, hard, MAG, SGN, C2V, POST))
                    if not len(idx):
                        break
            # ---- check sweep
            for d, eid in g.checks:
                a = MAG[:, eid]                   # [f, checks, d]
                s = SGN[:, eid]
                if fault is not None:
                    fault("check_mag", d, a, raw=(a.view(U) | hard[:, g.edge_var[eid]].astype(U)).view(T))
                pre = np.empty_like(a)
                acc = np.zeros(a.shape[:2], dtype=T)
                for j in range(d):
                    pre[:, :, j] = acc
                    acc = acc + a[:, :, j]
                es = np.empty_like(a)
                suf = np.zeros(a.shape[:2], dtype=T)
                for j in range(d - 1, -1, -1):
                    es[:, :, j] = pre[:, :, j] + suf
                    suf = suf + a[:, :, j]
                if fault is not None:
                    fault("check_sum", d, es, mag=a)
                out = np.ascontiguousarray(f(es))
                if fault is not None:
                    fault("check_out", d, out)
                neg = np.logical_xor.reduce(s, axis=2)[:, :, None] ^ s
                C2V[:, eid] = ((out.view(U) & ~SIGN) | np.where(neg, SIGN, U(0))).view(T)
            # ---- variable sweep
            for d, vid, eid in g.vars:
                llr = LLR[:, vid]
                c = C2V[:, eid]                   # [f, vars, d]
                pre = np.empty_like(c)
                s = np.zeros(llr.shape, dtype=T)
                for k in range(d):
                    pre[:, :, k] = s
                    s = s + c[:, :, k]
                total = llr + s
                if fault is not None:
                    fault("var_total", d, total, llr=llr, c=c)
                POST[:, vid] = total
                hard[:, vid] = total <= 0
                suf = np.zeros(llr.shape, dtype=T)
                x = np.empty_like(c)
                for k in range(d - 1, -1, -1):
                    x[:, :, k] = llr + (pre[:, :, k] + suf)
                    suf = suf + c[:, :, k]
                if fault is not None:
                    fault("var_x", d, x, llr=llr, c=c)
                p = f(np.abs(x))
                mg = _mag(p, U)
                if fault is not None:
                    fault("var_mag", d, mg, p=p)
                MAG[:, eid] = mg
                SGN[:, eid] = x <= 0
            it += 1
            if trace_at is not None and it == trace_at:
                v2c = (np.ascontiguousarray(MAG).view(U) | hard[:, g.edge_var].astype(U) | np.where(SGN, SIGN, U(0))).view(T)
                return bits, ok, iters, (C2V, v2c, POST)
    return bits, ok, iters


def fused_post(g, llr, c2v, dtype):
    """the posterior acg_ldpc_debug_bp_trace reports for the FUSED engines: not a word of the kernel but a host-side double sum,
    unscaled llr + (the unscaled c->v words of the variable added up from 0 in col_edge order).  llr [F, n], c2v [F, E] of T"""
    un = LN2 if np.dtype(dtype) == np.float32 else 1.0
    cd = un * c2v.astype(np.float64)
    post = un * llr.astype(np.float64) + 0.0
    with np.errstate(invalid="ignore"):
        for d, vid, eid in g.vars:
            s = np.zeros(post[:, vid].shape)
            for k in range(d):
                s = s + cd[:, eid[:, k]]
            post[:, vid] = un * llr[:, vid].astype(np.float64) + s
    return post


# ------------------------------------------------------------------------------------------ deliberate departures
def _ulps(out, k):
    """move every (non-negative) value of `out` by k places in its type's bit patterns: +inf + 1 is a NaN, +0 - 1 is not asked"""
    U = _UINT[out.dtype]
    v = out.view(U)
    if k > 0:
        v += U(k)
    else:
        v -= U(-k)


def mutant(name, T=np.float32):
    """fault hooks, one changed operation each — the ones hard outputs do not see (tests/test_spa_ref.py)"""
    T = np.dtype(T)
    U = _UINT[T]

    def hook(site, d, out, **kw):
        if name == "total_minus_own" and site == "check_sum":
            mag = kw["mag"]
            tot = np.zeros(mag.shape[:2], dtype=T)
            for j in range(d):
                tot = tot + mag[:, :, j]
            with np.errstate(invalid="ignore"):
                v = tot[:, :, None] - mag
            out[...] = np.where(np.isnan(v), out, v)               # (inf - inf: keep the kernel's sum, the mutant is about rounding)
        elif name == "suffix_ascending" and site == "check_sum":
            mag = kw["mag"]
            acc = np.zeros(mag.shape[:2], dtype=T)
            for j in range(d):
                suf = np.zeros(mag.shape[:2], dtype=T)
                for k in range(j + 1, d):
                    suf = suf + mag[:, :, k]
                out[:, :, j] = acc + suf
                acc = acc + mag[:, :, j]
        elif name == "check_lsb_kept" and site == "check_mag":
            out[...] = kw["raw"]
        elif name == "var_reverse" and site == "var_total":
            s = np.zeros(out.shape, dtype=T)
            for k in range(d - 1, -1, -1):
                s = s + kw["c"][:, :, k]
            out[...] = kw["llr"] + s
        elif name == "var_reverse" and site == "var_x":
            llr, c = kw["llr"], kw["c"][:, :, ::-1]
            pre = np.empty_like(c)
            s = np.zeros(llr.shape, dtype=T)
            for k in range(d):
                pre[:, :, k] = s
                s = s + c[:, :, k]
            suf = np.zeros(llr.shape, dtype=T)
            for k in range(d - 1, -1, -1):
                out[:, :, d - 1 - k] = llr + (pre[:, :, k] + suf)
                suf = suf + c[:, :, k]
        elif name == "llr_first" and site == "var_x":
            llr, c = kw["llr"], kw["c"]
            pre = np.empty_like(c)
            s = np.zeros(llr.shape, dtype=T)
            for k in range(d):
                pre[:, :, k] = s
                s = s + c[:, :, k]
            suf = np.zeros(llr.shape, dtype=T)
            for k in range(d - 1, -1, -1):
                out[:, :, k] = (llr + pre[:, :, k]) + suf
                suf = suf + c[:, :, k]
        elif name == "phi_lsb_kept" and site == "var_mag":
            out[...] = np.abs(kw["p"])
    assert name in MUTANTS
    return hook


# name -> what it does
MUTANTS = {
    "total_minus_own": "check sums as total - own instead of prefix + suffix",
    "var_reverse": "variable edges summed in reverse",
    "llr_first": "(llr + pre) + suf instead of llr + (pre + suf)",
    "phi_lsb_kept": "the hard-decision LSB left inside the phi magnitude (variable side does not clear it)",
    "suffix_ascending": "suffix accumulated ascending",
    "check_lsb_kept": "no LSB clear on the check side",
}


KNIFE_SNR = 0.0        # sigma^2 = 1/2: the double-precision LLR 2 * y / sigma^2 is exact, every wanted LLR has its symbol


def ulp_fault(d_target, k):
    """the messages of the checks of degree d_target moved by k bit patterns"""
    def hook(site, d, out, **kw):
        if site == "check_out" and d == d_target:
            _ulps(out, k)
    return hook


# ------------------------------------------------------------------------------------------ one message, to the last bit
def knife_edge_graph():
    """eight disjoint checks of degree 1 ... 8, n = 36: the graph of layered_ref.knife_edge_case"""
    from layered_ref import host_phi, knife_edge_case
    return knife_edge_case(host_phi, 1.0, 1, 0)[0]


def knife_edge_graph_absorbed():
    """Eight checks of degree 1 ... 8 whose LAST edge (highest column) is a variable of degree 1 and whose other edges are
    variables of degree 2, each shared by two checks (14 of them, columns 0 ... 13; the degree-1 variables are columns 14 ... 21):
    the shape for which the fp32 wave-group kernels keep the degree-1 variable in a register of its check's lane
    (BpPass::check_abs) — every check of the trailing pass has exactly one degree-1 variable, in its highest column.  The
    disjoint graph above does not have it (its checks have up to eight degree-1 variables)."""
    left = list(range(8))                      # check c still needs `left[c]` shared variables; it has degree c + 1
    pairs = []
    while sum(left):
        a, b = sorted(range(8), key=lambda c: (-left[c], c))[:2]
        assert left[a] and left[b]
        pairs.append((a, b))
        left[a] -= 1
        left[b] -= 1
    Hm = np.zeros((8, len(pairs) + 8), dtype=np.uint8)
    for v, (a, b) in enumerate(pairs):
        Hm[a, v] = Hm[b, v] = 1
    for c in range(8):
        Hm[c, len(pairs) + c] = 1
    assert Hm.sum(axis=1).tolist() == list(range(1, 9)) and set(Hm[:, :len(pairs)].sum(axis=0)) == {2}
    return Hm


def knife_edge_case(phi, snr, frames, seed, dtype=np.float32, absorbed=False):
    """Inputs on which ONE message of the first flooding iteration decides the frame's flag, to the last bit; run with
    max_iter = 1.  In iteration 1 a check sees phi(|llr|) of raw channel LLRs, and the total of a variable of degree 1 is
    llr + (+0 + out).  Frame f targets check f mod 8 and an edge j of it that leads to a degree-1 variable — a random one on
    the graph of disjoint checks (absorbed=False), the last one on knife_edge_graph_absorbed (absorbed=True).  The other
    symbols are positive, out_j depends on them alone and is positive, and symbol j is chosen so that its LLR (in T's domain) is
    exactly
        kind A (f // 8 even)   -out_j:                total = +0, and the flooding kernels decide by total <= 0: hard = 1
        kind B (f // 8 odd)    -nextafter(out_j, 0):  total > 0:  hard = 0
    A message one ulp high turns A's total positive (hard 0); one ulp low turns B's total into +0 (hard 1).  (The layered kernel
    decides by sign bit, so layered_ref's kinds are -out and -nextafter(out, inf).)  The targeted variable is negative, so the
    check's other variables receive a negative message and may flip too: the restatement says what the flag is.
    Degree 1: out = phi(+0) = +inf.  Kind A would need llr = -inf and gives NaN (hard 0) whatever the message: such frames
    are built as kind B (llr = -largest finite, total = +inf), which catch a message that is finite; there is no bit pattern
    "one ulp above" +inf but a NaN, and NaN <= 0 is as false as inf <= 0.
    Frames for which no double symbol gives the wanted LLR exactly are dropped.
    -> Hm [8, n], y [F', n] float64, knife [F'] the variable on the edge, kind_b [F'] bool, dropped [8] frames dropped per degree"""
    T = np.dtype(dtype)
    U = _UINT[T]
    Hm = knife_edge_graph_absorbed() if absorbed else knife_edge_graph()
    degs = Hm.sum(axis=1).astype(int).tolist()
    cols = [np.nonzero(Hm[c])[0] for c in range(len(degs))]      # a check's variables ascending: its edges in order
    n = Hm.shape[1]
    rng = np.random.default_rng(seed)
    var = 10.0 ** (-(snr / 10.0)) / 2.0
    dom = 1.44269504088896341 if T == np.float32 else 1.0
    y = rng.uniform(0.6, 6.0, size=(frames, n)) * var / 2.0 / dom          # LLRs of 0.6 ... 6 in T's domain
    edge = np.array([degs[f % len(degs)] - 1 if absorbed else int(rng.integers(0, degs[f % len(degs)])) for f in range(frames)])
    assert all(Hm[:, cols[f % len(degs)][edge[f]]].sum() == 1 for f in range(frames))
    llr = channel_llr(y, snr, T)
    mag = _mag(phi(np.abs(llr)), U)
    keep = np.zeros(frames, dtype=bool)
    kind_b = np.zeros(frames, dtype=bool)
    knife = np.zeros(frames, dtype=np.int64)
    dropped = np.zeros(len(degs), dtype=np.int64)
    # the exclude-self sums of the targeted edges, as the check sweep forms them; one phi call for all frames
    es = np.zeros(frames, dtype=T)
    for f in range(frames):
        c = f % len(degs)
        m = mag[f, cols[c]]
        pre = T.type(0)
        for j in range(edge[f]):
            pre = pre + m[j]
        suf = T.type(0)
        for j in range(degs[c] - 1, edge[f], -1):
            suf = suf + m[j]
        es[f] = pre + suf
    out = phi(es)
    for f in range(frames):
        c = f % len(degs)
        b = (f // len(degs)) % 2 == 1 or degs[c] == 1
        target = np.nextafter(out[f], T.type(0)) if b else out[f]
        t0 = -(np.float64(target) * var / 2.0 / dom)
        cand = [t0]
        lo = hi = t0
        for _ in range(6):
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
            cand += [lo, hi]
        for ys in cand:
            if channel_llr(np.array([[ys]]), snr, T)[0, 0] == -target:
                y[f, cols[c][edge[f]]] = ys
                keep[f], kind_b[f], knife[f] = True, b, cols[c][edge[f]]
                break
        else:
            dropped[c] += 1
    return Hm, y[keep], knife[keep], kind_b[keep], dropped
