"""numpy restatement of the streamed fixed-point layered min-sum engine (acg_ldpc_decoder_create_quantized_streamed,
csrc/bp_streamed_q.hip) on a SPARSE graph: an edge list instead of the dense Hm of tests/layered_q_io_ref.py, whose control
skeleton (layered_ref._run_layered) forms its final syndrome as a dense product of 8 m n bytes — 670 MB for the 2050 x 41 000
code this engine exists for.  Nothing of the arithmetic is restated: the check is layered_q_ref.check_update, the limits
layered_q_ref.limits, the channel clamp layered_q_io_ref.clamp_channel.  Only the control skeleton is written again, and
tests/test_streamed_q_ref.py holds it to decode_int frame for frame.

The sets are ParityCheckMatrix.layers_any()'s (or any list of layers whose checks share no variable and have one degree);
a list of single-check layers gives the same results, since a set's checks share no variable."""
import numpy as np

from layered_q_io_ref import clamp_channel
from layered_q_ref import DEFAULT, check_update, limits


def edges_of(Hm):
    """check -> its variables ascending (layered_ref._edges), from a dense matrix"""
    Hm = np.asarray(Hm)
    return [np.nonzero(Hm[c])[0] for c in range(Hm.shape[0])]


def single_check_layers(edges):
    """one layer per check with at least one variable, in row order"""
    return [[c] for c, e in enumerate(edges) if len(e)]


def decode_int_sparse(edges, n, layers, c, max_iter, quant=DEFAULT, messages=None):
    """edges: check -> variables ascending; layers: sets of check ids in processing order (-1 = none); c: frames x n integer
    channel values.
    messages: optional list; the final [F, E] int8 messages are appended to it, edges in processing order (the sets of `layers`,
    set by set, each check's variables ascending).
    -> bits [F, n] uint8 (zeros for failed frames), ok [F] uint8, iters [F] int32, post [F, n] int16"""
    P = clamp_channel(c, quant)
    F = P.shape[0]
    assert P.shape[1] == n
    sets = []
    for layer in layers:
        ids = np.asarray(layer)[np.asarray(layer) >= 0]
        ids = [k for k in ids if len(edges[k])]
        if ids:
            V = np.stack([edges[k] for k in ids])                      # [cnt, D]: one degree per set
            sets.append((V, np.zeros((F,) + V.shape, dtype=np.int32)))
    done = np.zeros(F, dtype=bool)
    bits = np.zeros((F, n), dtype=np.uint8)
    ok = np.zeros(F, dtype=np.uint8)
    iters = np.full(F, max_iter, dtype=np.int32)
    for it in range(1, max_iter + 1):
        live = ~done
        if not live.any():
            break
        loud = np.zeros(F, dtype=bool)
        for V, R in sets:
            pn, rn, l = check_update(P[:, V], R, quant)
            P[np.ix_(live, V.ravel())] = pn[live].reshape(int(live.sum()), -1)     # a latched frame keeps its posteriors
            R[live] = rn[live]
            loud |= l.any(axis=1)
        newly = live & ~loud
        bits[newly] = P[newly] < 0
        ok[newly] = 1
        iters[newly] = it
        done |= newly
    rest = np.nonzero(~done)[0]
    if len(rest) and max_iter > 0:          # out of iterations without a quiet round: one explicit syndrome pass
        hb = P[rest] < 0
        bad = np.zeros(len(rest), dtype=bool)
        for V, _ in sets:
            bad |= np.logical_xor.reduce(hb[:, V], axis=2).any(axis=1)
        good = rest[~bad]
        bits[good] = hb[~bad]
        ok[good] = 1
    assert np.abs(P).max(initial=0) <= limits(quant)[2]
    if messages is not None:
        R = np.concatenate([r.reshape(F, -1) for _, r in sets] + [np.zeros((F, 0), dtype=np.int32)], axis=1)
        assert np.abs(R).max(initial=0) <= 127
        messages.append(R.astype(np.int8))
    return bits, ok, iters, P.astype(np.int16)
