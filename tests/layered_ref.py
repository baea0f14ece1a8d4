"""numpy restatements (vectorised over frames) of the layered kernels of csrc/bp_layered.hip — the repo's OWN restatements: the
layered schedule is not in the reference (algo/bp.h:183-199 floods) and neither is min-sum, so what they check is
that the kernel does what its description says, operation for operation; parity with the reference is FER-level only
(tests/test_layered.py).

  layered_minsum            fp32, normalised min-sum (layer_back): exact
  layered_sumproduct_exact  fp32, sum-product (layer_back_spa) with phi handed in: exact when phi is the device's own
                            Dom<float>::phi (acg_ldpc_debug_phi_sat), everything else being plain IEEE fp32 adds, minima and bit
                            operations in a fixed order
  layered_sumproduct        float64 sum-product with the exact phi: what the fp32 kernel approximates, agreement is a rate

All three share one control skeleton (_run_layered): the quiet-round rule, latching, the iteration count and the final
syndrome pass."""
import numpy as np

LOG2E_F32 = np.float32(1.44269504088896341)      # (float) Dom<float>::scale
SPA_SATURATION = np.float32(83.25)               # LAYERED_SPA_SATURATION


def _variance(snr):
    return 10.0 ** (-(snr / 10.0)) / 2.0


def channel_llr_f32(y, snr, symbols_f32=False):
    """the kernel's fp32 channel LLR (channel.h:14-16): double symbols go through 2 * y / var, float symbols through
    (double) y * (2 / var) — two different roundings of the same number"""
    var = _variance(snr)
    with np.errstate(over="ignore"):
        if symbols_f32:
            return (np.asarray(y).astype(np.float32).astype(np.float64) * (2.0 / var)).astype(np.float32)
        return (2.0 * np.asarray(y).astype(np.float64) / var).astype(np.float32)


def _edges(Hm):
    """edge j of a check = its j-th variable ascending (the CSR order of bp_layered_build; block-column order for a quasi-cyclic H)"""
    return [np.nonzero(Hm[c])[0] for c in range(Hm.shape[0])]


def _run_layered(Hm, layers, P, max_iter, layer_step):
    """control flow shared by the restatements.  P: [F, n] posteriors, updated in place by layer_step(index of the layer, its check
    ids, live) -> [F] bool, True where the step was NOT quiet (a check of the layer unsatisfied by the signs it read, or a
    posterior it wrote changed sign); layer_step writes P and its messages for the `live` frames only.  A frame stops (and its
    word is latched) after the first iteration in which every step was quiet; one that runs out of iterations gets one explicit
    syndrome pass; 0 iterations -> every frame fails.
    -> bits [F, n] uint8 (zeros for failed frames), ok [F] uint8, iters [F] int32"""
    F, n = P.shape
    done = np.zeros(F, dtype=bool)
    bits = np.zeros((F, n), dtype=np.uint8)
    ok = np.zeros(F, dtype=np.uint8)
    iters = np.full(F, max_iter, dtype=np.int32)
    occupied = [(li, np.asarray(layer)[np.asarray(layer) >= 0]) for li, layer in enumerate(layers)]
    for it in range(1, max_iter + 1):
        live = ~done
        if not live.any():
            break
        loud = np.zeros(F, dtype=bool)
        for li, ids in occupied:
            if len(ids):
                loud |= layer_step(li, ids, live)
        newly = live & ~loud
        bits[newly] = np.signbit(P[newly]).astype(np.uint8)
        ok[newly] = 1
        iters[newly] = it
        done |= newly
    rest = ~done
    if rest.any() and max_iter > 0:     # out of iterations without a quiet round: one explicit syndrome pass
        hb = np.signbit(P[rest]).astype(np.uint8)
        good = ((hb @ np.asarray(Hm).T.astype(np.int64)) % 2 == 0).all(axis=1)
        idx = np.nonzero(rest)[0][good]
        bits[idx] = hb[good]
        ok[idx] = 1
    return bits, ok, iters


def _messages_in_processing_order(layers, of_check, F):
    """[F, E] fp32: the messages of the checks of `layers`, set by set in processing order, each check's edges in the order the
    restatement took them (of_check(c) -> [F, D])"""
    parts = [of_check(c) for layer in layers for c in np.asarray(layer)[np.asarray(layer) >= 0]]
    return np.concatenate(parts + [np.zeros((F, 0), dtype=np.float32)], axis=1).astype(np.float32)


def layered_minsum(Hm, layers, y, snr, max_iter, scale, msg_dtype=np.float32, symbols_f32=False, posteriors=None, messages=None):
    """Hm: m x n 0/1; layers: [n_layers, G] check ids (-1 = none) in processing order; y: frames x n symbols.
    msg_dtype: storage type of the check-to-variable messages (np.float16 = precision PREC_F16: the scaled minima are rounded
    to half precision once per check; the posteriors stay fp32 and add / subtract exactly the rounded message).
    symbols_f32: the symbols reach the kernel as float32 (the (double) y * (2 / var) LLR path).
    posteriors: optional list; the final [F, n] fp32 posteriors are appended to it.
    messages: optional list; the final [F, E] fp32 messages are appended to it, edges in processing order (the sets of `layers`,
    set by set, each check's variables ascending).
    -> bits [F, n] uint8 (zeros for failed frames), ok [F] uint8, iters [F] int32"""
    Hm = np.asarray(Hm)
    F, n = y.shape
    P = channel_llr_f32(y, snr, symbols_f32)                           # channel.h:14-16, rounded to the kernel's fp32
    edges = _edges(Hm)
    R = [np.zeros((F, len(e)), dtype=np.float32) for e in edges]
    scale = np.float32(scale)

    def layer_step(li, ids, live):
        loud = np.zeros(F, dtype=bool)
        for c in ids:
            v = edges[c]
            p = P[:, v]
            q = p - R[c]
            a = np.abs(q)
            srt = np.sort(a, axis=1)
            m1, m2 = srt[:, 0], (srt[:, 1] if a.shape[1] > 1 else np.full(F, np.inf, np.float32))
            # the kernel forms scale * min and rounds it to the storage type in ONE step (v_fma_mixlo_f16 for fp16): the
            # product of two fp32 numbers is exact in float64, so rounding that once is the same thing
            with np.errstate(over="ignore"):
                m1s = (np.float64(scale) * m1.astype(np.float64)).astype(msg_dtype).astype(np.float32)
                m2s = (np.float64(scale) * m2.astype(np.float64)).astype(msg_dtype).astype(np.float32)
            if a.shape[1] == 1:       # a one-variable check: its message saturates instead of being infinite
                m2s = np.full(F, np.float32(59968.0), dtype=np.float32)
            mag = np.where(a == m1[:, None], m2s[:, None], m1s[:, None]).astype(np.float32)
            sq = np.signbit(q)
            S = np.logical_xor.reduce(sq, axis=1)
            neg = S[:, None] ^ sq
            rn = np.where(neg, -mag, mag).astype(np.float32)
            pn = (q + rn).astype(np.float32)
            parity = np.logical_xor.reduce(np.signbit(p), axis=1)
            loud |= parity | (np.signbit(pn) != np.signbit(p)).any(axis=1)
            P[np.ix_(live, v)] = pn[live]
            R[c][live] = rn[live]
        return loud
    res = _run_layered(Hm, layers, P, max_iter, layer_step)
    if posteriors is not None:
        posteriors.append(P)
    if messages is not None:
        messages.append(_messages_in_processing_order(layers, lambda c: R[c], F))
    return res


def host_phi(x):
    """CPU stand-in for the device phi in the kernels' log2(e)-scaled domain: F(x') = log2(e) * phi(x' ln 2), phi(x) =
    -log(tanh(x / 2)), evaluated in float64 and rounded to fp32; 0 for x' >= 66 (the saturation of Dom<float>::phi, +inf
    included), +inf at 0.  Not the device's bits (v_log_f32 / v_exp_f32 and two minimax fits): with it the restatement is a
    faithful fp32 layered sum-product, not an exact copy of the kernel."""
    x = np.asarray(x, dtype=np.float32)
    xl = x.astype(np.float64) * np.log(2.0)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore", under="ignore"):
        t = np.exp(-xl)
        big = np.log1p(2 * t / (1 - t))                 # = -log(tanh(x / 2)), accurate where tanh(x / 2) is close to 1
        small = -np.log(np.tanh(xl / 2))
        f = np.where(xl >= 1, big, small) / np.log(2.0)
        out = np.where(x >= np.float32(66), 0, f).astype(np.float32)
    return out


def spa_messages(q, phi, msg_dtype=np.float32, variant=None):
    """the check rule of layer_back_spa on q [..., D] (fp32, edges in processing order along the last axis) -> new messages r':
        mag_j = phi(|q_j|)
        pre_j = mag_0 + ... + mag_{j-1}, summed in that order from +0;  suf_j = mag_{D-1} + ... + mag_{j+1}, in THAT order from +0
        out_j = fmin(phi(pre_j + suf_j), 83.25), rounded ONCE to msg_dtype;  sign = XOR of all sign bits of q XOR that of q_j"""
    D = q.shape[-1]
    mag = phi(np.abs(q))
    assert mag.dtype == np.float32 and mag.shape == q.shape
    pre = np.empty_like(mag)
    suf = np.empty_like(mag)
    s = np.zeros(mag.shape[:-1], dtype=np.float32)
    for j in range(D):
        pre[..., j] = s
        s = s + mag[..., j]
    s = np.zeros(mag.shape[:-1], dtype=np.float32)
    for j in range(D - 1, -1, -1):
        suf[..., j] = s
        s = s + mag[..., j]
    if variant == "suffix_ascending":                  # (not the kernel: mag_{j+1} + ... + mag_{D-1} in THAT order)
        for j in range(D):
            s = np.zeros(mag.shape[:-1], dtype=np.float32)
            for k in range(j + 1, D):
                s = s + mag[..., k]
            suf[..., j] = s
    out = np.fmin(phi(pre + suf), SPA_SATURATION)
    assert out.dtype == np.float32
    out = out.astype(msg_dtype).astype(np.float32)
    if variant == "round_twice":
        out = out.astype(msg_dtype).astype(np.float32)
    sq = np.signbit(q)
    neg = np.logical_xor.reduce(sq, axis=-1)[..., None] ^ sq
    return np.where(neg, -np.abs(out), np.abs(out)).astype(np.float32)


def layered_sumproduct_exact(Hm, layers, y, snr, max_iter, phi, msg_dtype=np.float32, symbols_f32=False, variant=None,
                             posteriors=None, messages=None):
    """fp32 restatement of the SUM-PRODUCT layered kernel (layer_back_spa), operation for operation, in the log2(e)-scaled
    message domain.  phi: float32 array -> float32 array of the same shape, the map F of Dom<float>::phi; with the device's own
    (acg_ldpc_debug_phi_sat) every other operation is reproduced exactly: word, flag and iteration count of every frame are
    the kernel's.  One layer at a time as [F, cnt, D] arrays (a layer's checks share no variable and have one degree), so phi
    is called twice per layer step.

    Per check, edges j = 0..D-1 in ascending variable order:
        q_j = p_j - r_j;  mag_j = phi(|q_j|)
        pre_j = mag_0 + ... + mag_{j-1}, summed in that order from +0;  suf_j = mag_{D-1} + ... + mag_{j+1}, in THAT order from +0
        out_j = fmin(phi(pre_j + suf_j), 83.25), rounded ONCE to msg_dtype;  sign = XOR of all sign bits of q XOR that of q_j
        p'_j = q_j + r'_j
    variant (CPU tests only — deliberate departures, to show which ones are observable): "reverse_edges" takes the edges in
    descending variable order (an exact symmetry: prefix and suffix swap roles and their sum commutes); "rotate_edges" starts
    each check at its last variable; "suffix_ascending" accumulates the suffix sums in ascending edge order; "round_twice"
    rounds out to msg_dtype twice (idempotent: the kernel's second (RT) at the store).
    posteriors: optional list; the final [F, n] fp32 posteriors are appended to it.
    messages: optional list; the final [F, E] fp32 messages are appended to it, edges in processing order (the sets of `layers`,
    set by set, each check's edges in the order this run took them: variables ascending unless a variant says otherwise).
    -> bits [F, n] uint8 (zeros for failed frames), ok [F] uint8, iters [F] int32"""
    assert variant in (None, "reverse_edges", "rotate_edges", "suffix_ascending", "round_twice")
    Hm = np.asarray(Hm)
    F, n = y.shape
    P = channel_llr_f32(y, snr, symbols_f32) * LOG2E_F32
    edges = _edges(Hm)
    if variant == "reverse_edges":
        edges = [e[::-1] for e in edges]
    if variant == "rotate_edges":
        edges = [np.roll(e, 1) for e in edges]
    V, R = {}, {}
    for li, layer in enumerate(layers):
        ids = np.asarray(layer)[np.asarray(layer) >= 0]
        if len(ids):
            V[li] = np.stack([edges[c] for c in ids])                   # [cnt, D]: one degree per layer
            R[li] = np.zeros((F,) + V[li].shape, dtype=np.float32)

    def layer_step(li, ids, live):
        v = V[li]
        p = P[:, v]                                                     # [F, cnt, D]
        q = p - R[li]
        rn = spa_messages(q, phi, msg_dtype, variant)
        pn = q + rn
        parity = np.logical_xor.reduce(np.signbit(p), axis=2)
        loud = (parity | (np.signbit(pn) != np.signbit(p)).any(axis=2)).any(axis=1)
        P[np.ix_(live, v.ravel())] = pn[live].reshape(int(live.sum()), -1)
        R[li][live] = rn[live]
        return loud
    res = _run_layered(Hm, layers, P, max_iter, layer_step)
    if posteriors is not None:
        posteriors.append(P)
    if messages is not None:
        messages.append(np.concatenate([R[li].reshape(F, -1) for li in sorted(R)] + [np.zeros((F, 0), dtype=np.float32)], axis=1))
    return res


def knife_edge_case(phi, snr, frames, seed, msg_dtype=np.float32):
    """Inputs on which ONE message of the first layered sum-product iteration decides the frame's flag, to the last bit.
    The graph is eight checks of degree 1 ... 8 on disjoint variables (n = 36), so in iteration 1 every check sees raw channel
    LLRs.  Frame f targets check f mod 8 and a random edge j of it: the other symbols are positive, the message out_j the check
    sends to j depends on them alone, and symbol j is chosen so that its scaled LLR is exactly -out_j (frames with f // 8 even:
    P'_j = -out_j + out_j = +0, hard decision 0, H x = 0, ok = 1) or exactly -nextafter(out_j, inf) (f // 8 odd: P'_j < 0, hard
    decision 1, ok = 0).  A kernel whose out_j is one ulp low fails the first kind, one ulp high the second, whatever the
    cause: the order of the prefix / suffix sums (D >= 4), the saturation constant (D = 1: out = 83.25), a missing or doubled
    rounding to the storage type, another phi.  Run with max_iter = 1.
    Frames for which no symbol gives the wanted fp32 LLR exactly are dropped.
    (The other variables of the targeted check receive a negative message and may flip too — always so for D = 2, where that
    message is as large as their own LLR — so the flag is not simply "even kind"; the restatement says what it is.)
    -> Hm [8, 36], y [F', 36] float64, knife [F'] the variable on the edge, high [F'] bool: the second kind"""
    degs = list(range(1, 9))
    n = sum(degs)
    Hm = np.zeros((len(degs), n), dtype=np.uint8)
    first = np.concatenate([[0], np.cumsum(degs)])
    for c, D in enumerate(degs):
        Hm[c, first[c]:first[c] + D] = 1
    rng = np.random.default_rng(seed)
    var = _variance(snr)
    y = rng.uniform(0.6, 6.0, size=(frames, n)) * var / 2.0 / float(LOG2E_F32)      # scaled LLRs of 0.6 ... 6
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


def layered_sumproduct(Hm, layers, y, snr, max_iter, sat=83.25 / 1.4426950408889634):
    """float64 restatement of the SUM-PRODUCT variant of the layered kernel (the reference's check rule, bp.h:49-57, with
    phi(x) = -log(tanh(x/2)) evaluated exactly; messages saturate at `sat` natural units like the kernel's).  The kernel works in
    fp32 with its own phi, so agreement is a RATE (tests/test_layered.py), not word for word."""
    Hm = np.asarray(Hm)
    F, n = y.shape
    P = 2.0 * y.astype(np.float64) / _variance(snr)
    edges = _edges(Hm)
    R = [np.zeros((F, len(e))) for e in edges]

    def phi(x):
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            return np.where(x >= 45.747713916956390, 0.0, -np.log(np.tanh(0.5 * x)))

    def layer_step(li, ids, live):
        loud = np.zeros(F, dtype=bool)
        for c in ids:
            v = edges[c]
            p = P[:, v]
            q = p - R[c]
            mag = phi(np.abs(q))
            # exclude-self sums formed directly (never total - own: an infinite term would turn into NaN), bp.h:50-55
            others = np.stack([np.delete(mag, j, axis=1).sum(axis=1) for j in range(mag.shape[1])], axis=1)
            out = np.minimum(phi(others), sat)
            sq = np.signbit(q)
            neg = np.logical_xor.reduce(sq, axis=1)[:, None] ^ sq
            rn = np.where(neg, -out, out)
            pn = q + rn
            parity = np.logical_xor.reduce(np.signbit(p), axis=1)
            loud |= parity | (np.signbit(pn) != np.signbit(p)).any(axis=1)
            P[np.ix_(live, v)] = pn[live]
            R[c][live] = rn[live]
        return loud
    return _run_layered(Hm, layers, P, max_iter, layer_step)
