"""numpy restatement (vectorised over frames) of the fixed-point layered min-sum kernel of csrc/bp_layered_q.hip — the arithmetic
that include/acg_ldpc.h writes next to acg_ldpc_quant, over the control skeleton the float restatements share
(layered_ref._run_layered: the quiet-round rule, latching, the iteration count, the final syndrome pass).  Every value is an
integer, so word, flag and exit iteration of every frame are the kernel's.

A quantiser is the 7-tuple (llr_step, ch_bits, msg_bits, post_bits, scale_num, scale_shift, offset)."""
import numpy as np

from layered_ref import _edges, _run_layered, channel_llr_f32

DEFAULT = (0.5, 6, 6, 8, 1, 0, 1)


def limits(quant):
    """-> Cmax, Rmax, Pmax"""
    _, ch, msg, post = quant[:4]
    return (1 << (ch - 1)) - 1, (1 << (msg - 1)) - 1, (1 << (post - 1)) - 1


def quantize_llr(llr32, quant):
    """fp32 channel LLRs -> channel values: t = llr32 * (float) (1 / llr_step), ONE fp32 multiply; round half to even; clamp to
    +-Cmax; NaN -> 0, +-inf -> +-Cmax"""
    cmax = limits(quant)[0]
    llr32 = np.asarray(llr32)
    assert llr32.dtype == np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        t = llr32 * np.float32(1.0 / quant[0])
        assert t.dtype == np.float32
        c = np.clip(np.rint(t), -cmax, cmax)
    return np.where(np.isnan(t), 0, c).astype(np.int32)


def quantize(y, snr, quant, symbols_f32=False):
    """channel symbols -> channel values, through the fp32 LLR of the float layered kernels"""
    return quantize_llr(channel_llr_f32(y, snr, symbols_f32), quant)


def check_update(p, r, quant):
    """one check on every leading index: p, r [..., D] int32 posteriors and old messages of its edges ->
    (p' [..., D], r' [..., D], loud [...]: the check was not quiet)"""
    _, rmax, pmax = limits(quant)
    num, shift, offset = quant[4:]
    rnd = (1 << (shift - 1)) if shift > 0 else 0
    q = p - r
    s = q < 0
    a = np.minimum(np.abs(q), rmax)
    srt = np.sort(a, axis=-1)
    m1 = srt[..., 0]
    m2 = srt[..., 1] if a.shape[-1] > 1 else np.full_like(m1, rmax)
    mu = np.where(a == m1[..., None], m2[..., None], m1[..., None])
    mu = np.maximum(((mu * num + rnd) >> shift) - offset, 0)
    neg = np.logical_xor.reduce(s, axis=-1)[..., None] ^ s
    rn = np.where(neg, -mu, mu)
    pn = np.clip(q + rn, -pmax, pmax)
    loud = np.logical_xor.reduce(p < 0, axis=-1) | ((pn < 0) != (p < 0)).any(axis=-1)
    return pn.astype(np.int32), rn.astype(np.int32), loud


def layered_minsum_q(Hm, layers, y, snr, max_iter, quant=DEFAULT, symbols_f32=False):
    """Hm: m x n 0/1; layers: [n_layers, width] check ids (-1 = none) in processing order (ParityCheckMatrix.layers_wide());
    y: frames x n symbols.  One layer at a time as [F, cnt, D] arrays: a layer's checks share no variable and have one degree.
    -> bits [F, n] uint8 (zeros for failed frames), ok [F] uint8, iters [F] int32"""
    Hm = np.asarray(Hm)
    F, n = y.shape
    P = quantize(y, snr, quant, symbols_f32)
    edges = _edges(Hm)
    V, R = {}, {}
    for li, layer in enumerate(layers):
        ids = np.asarray(layer)[np.asarray(layer) >= 0]
        if len(ids):
            V[li] = np.stack([edges[c] for c in ids])                   # [cnt, D]: one degree per layer
            R[li] = np.zeros((F,) + V[li].shape, dtype=np.int32)

    def layer_step(li, ids, live):
        v = V[li]
        pn, rn, loud = check_update(P[:, v], R[li], quant)
        P[np.ix_(live, v.ravel())] = pn[live].reshape(int(live.sum()), -1)
        R[li][live] = rn[live]
        return loud.any(axis=1)
    bits, ok, iters = _run_layered(Hm, layers, _Signed(P), max_iter, layer_step)
    return bits, ok, iters


class _Signed(np.ndarray):
    """the posteriors as _run_layered reads them: it takes hard decisions with np.signbit, which integers do not have"""
    def __new__(cls, a):
        return a.view(cls)

    def __array_ufunc__(self, ufunc, method, *inputs, **kw):
        inputs = tuple(np.asarray(x) for x in inputs)
        if ufunc is np.signbit:
            return inputs[0] < 0
        return getattr(ufunc, method)(*inputs, **kw)
