"""numpy restatement of the INTEGER entrance of the fixed-point layered min-sum engine (acg_ldpc_decode_batch_q*, the IO instances
of bp_layered_q_kernel): int16 channel values in, word, flag, exit iteration and int16 posteriors out.  Nothing new is restated:
the check is layered_q_ref.check_update, the limits layered_q_ref.limits, the control skeleton layered_ref._run_layered.

The posterior of a frame is what the kernel holds when it writes the frame's outputs.  _run_layered hands layer_step the `live`
frames and layer_step writes only those, so the row of a frame that latched stays as it was at its latch, and the row of one that
never latched is the state after max_iter iterations: the final P IS the posterior, whatever early_exit says on the device."""
import numpy as np

from layered_q_ref import DEFAULT, _Signed, check_update, limits
from layered_ref import _edges, _run_layered


def clamp_channel(c, quant):
    """int channel values of any width -> what the decoder starts from: clamp(c, -Cmax, +Cmax) (so -32768 -> -Cmax)"""
    cmax = limits(quant)[0]
    return np.clip(np.asarray(c).astype(np.int64), -cmax, cmax).astype(np.int32)


def decode_int(Hm, layers, c, max_iter, quant=DEFAULT, keep_sweeping=False):
    """Hm: m x n 0/1; layers: ParityCheckMatrix.layers_wide()'s sets; c: frames x n integer channel values.
    keep_sweeping (tests only, NOT the engine): latched frames go on being updated, so the posteriors returned are the state
    after the last iteration anybody ran — what an implementation that copied P out at the end of a fixed-work run would give.
    -> bits [F, n] uint8 (zeros for failed frames), ok [F] uint8, iters [F] int32, post [F, n] int16"""
    Hm = np.asarray(Hm)
    P = clamp_channel(c, quant)
    F = P.shape[0]
    edges = _edges(Hm)
    V, R = {}, {}
    for li, layer in enumerate(layers):
        ids = np.asarray(layer)[np.asarray(layer) >= 0]
        if len(ids):
            V[li] = np.stack([edges[k] for k in ids])                   # [cnt, D]: one degree per layer
            R[li] = np.zeros((F,) + V[li].shape, dtype=np.int32)

    def layer_step(li, ids, live):
        if keep_sweeping:
            live = np.ones(F, dtype=bool)
        v = V[li]
        pn, rn, loud = check_update(P[:, v], R[li], quant)
        P[np.ix_(live, v.ravel())] = pn[live].reshape(int(live.sum()), -1)
        R[li][live] = rn[live]
        return loud.any(axis=1)
    bits, ok, iters = _run_layered(Hm, layers, _Signed(P), max_iter, layer_step)
    assert np.abs(P).max(initial=0) <= limits(quant)[2]
    return bits, ok, iters, np.asarray(P).astype(np.int16)
