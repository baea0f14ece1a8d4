"""numpy restatement of the detail run (acg_ldpc_mc_run_detail, include/acg_ldpc.h): the classification of the reference's
exp() (experiment.h:109-120) extended by post-decoding bit errors and the log of the frames that are not correct.

It sees only what a decoder returned — symbols, packed output words, flags, sweep counts — never the library's own
classification, so tests use it as the expectation for the device and the host path alike."""
import numpy as np

EVENT_PSEUDO, EVENT_NO_WORD, EVENT_NONCODEWORD = 1, 2, 3

EVENT_DTYPE = np.dtype([("frame", "<i8"), ("kind", "<i4"), ("iters", "<i4"), ("raw_errors", "<i4"), ("bit_errors", "<i4"),
                        ("syndrome_weight", "<i4"), ("reserved", "<i4")])

COUNTERS = ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong", "sum_iters", "word_frames",
            "bit_errors", "noncodeword_frames", "sum_syndrome_weight", "n_events", "n_stored", "min_pseudo_frame",
            "min_pseudo_weight")


def pack_bits(bits):
    """[F, n] 0/1 -> [F, (n+31)//32] uint32, bit v of a frame = word v >> 5, bit v & 31 (acg_ldpc_decode_batch_dev)"""
    bits = np.asarray(bits, dtype=np.uint8)
    F, n = bits.shape
    nw = (n + 31) // 32
    pad = np.zeros((F, nw * 32), dtype=np.uint64)
    pad[:, :n] = bits != 0
    return (pad.reshape(F, nw, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def unpack_bits(words, n):
    """the inverse; bits >= n of the last word are dropped, whatever they hold"""
    words = np.asarray(words, dtype=np.uint32)
    b = (words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return b.reshape(words.shape[0], words.shape[1] * 32)[:, :n].astype(np.uint8)


def mc_detail(y, words, ok, iters, sent, H, first_frame=0, cap=0):
    """y [F, n] channel symbols; words [F, nwords] packed returned words; ok [F] the decoder's flag; iters [F]; sent [F, n]
    the transmitted bits of every frame; H [m, n].  -> (counters dict, events [n_stored], xor rows [n_stored, nwords])."""
    y = np.asarray(y)
    sent = np.asarray(sent, dtype=np.uint8)
    H = (np.asarray(H) != 0).astype(np.int64)
    F, n = sent.shape
    nw = (n + 31) // 32
    ok = np.asarray(ok).reshape(F) != 0
    iters = np.asarray(iters, dtype=np.int64).reshape(F)
    bits = unpack_bits(np.asarray(words).reshape(F, nw), n)
    # raw-channel hard-decision errors (HammingDistanceTracker, experiment.h:25-47): y <= 0 reads as 1
    ham = (((sent == 0) & (y <= 0)) | ((sent != 0) & (y > 0))).sum(axis=1).astype(np.int64)
    diff = (bits ^ sent) * ok[:, None]                       # no word returned: nothing to compare
    dist = diff.sum(axis=1).astype(np.int64)
    synw = ((bits.astype(np.int64) @ H.T) & 1).sum(axis=1) * ok
    correct = ok & (synw == 0) & (dist == 0)
    pseudo = ok & (synw == 0) & (dist > 0)
    noncw = ok & (synw > 0)
    kind = np.where(correct, 0, np.where(pseudo, EVENT_PSEUDO, np.where(noncw, EVENT_NONCODEWORD, EVENT_NO_WORD)))
    c = dict(correct=int(correct.sum()), pseudo=int(pseudo.sum()), total=F, sum_hamming=int(ham.sum()),
             sum_hamming_ok=int(ham[correct].sum()), sum_hamming_wrong=int(ham[~correct].sum()), sum_iters=int(iters.sum()),
             word_frames=int(ok.sum()), bit_errors=int(dist.sum()), noncodeword_frames=int(noncw.sum()),
             sum_syndrome_weight=int(synw[noncw].sum()), n_events=int((~correct).sum()))
    if pseudo.any():
        w = int(dist[pseudo].min())
        c["min_pseudo_weight"] = w
        c["min_pseudo_frame"] = int(first_frame) + int(np.flatnonzero(pseudo & (dist == w))[0])   # the lowest frame wins ties
    else:
        c["min_pseudo_weight"] = c["min_pseudo_frame"] = -1
    idx = np.flatnonzero(~correct)[:max(int(cap), 0)]       # the cap lowest frames, ascending
    c["n_stored"] = len(idx)
    ev = np.zeros(len(idx), dtype=EVENT_DTYPE)
    ev["frame"] = int(first_frame) + idx
    ev["kind"] = kind[idx]
    ev["iters"] = iters[idx]
    ev["raw_errors"] = ham[idx]
    ev["bit_errors"] = dist[idx]
    ev["syndrome_weight"] = (synw * noncw)[idx]
    return c, ev, pack_bits(diff[idx]).reshape(len(idx), nw)


def merge(a, b, cap):
    """two shards (counters, events, rows) -> one, as acg_ldpc_mc_detail_merge and the mirrors do"""
    (ca, ea, wa), (cb, eb, wb) = a, b
    c = {k: ca[k] + cb[k] for k in COUNTERS if k not in ("n_stored", "min_pseudo_frame", "min_pseudo_weight")}
    best = min([(x["min_pseudo_weight"], x["min_pseudo_frame"]) for x in (ca, cb) if x["min_pseudo_weight"] > 0], default=(-1, -1))
    c["min_pseudo_weight"], c["min_pseudo_frame"] = best
    ev = np.concatenate([ea, eb])
    order = np.argsort(ev["frame"], kind="stable")[:cap]
    c["n_stored"] = len(order)
    return c, ev[order], np.concatenate([wa, wb])[order]
