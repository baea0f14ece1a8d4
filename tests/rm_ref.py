"""numpy restatement of what acg_ldpc_mc_run_rm (include/acg_ldpc.h) forms around the decoder for a punctured / shortened code:
the channel value of every position from its symbol, the raw-error count of a frame over the sent positions, and the seven
counters.  The symbols are those of acg_ldpc_awgn_dev (pinned by tests/awgn_ref.py); the LLR and the quantiser are the pinned
ones of tests/layered_ref.py and tests/layered_q_ref.py; nothing here comes from the code under test.

A pattern is uint8 [n]: 0 sent, 1 punctured, 2 shortened (None: all sent).  `sent` is the transmitted word of every frame,
uint8 [frames, n]."""
import numpy as np

from layered_q_ref import limits, quantize_llr
from layered_ref import channel_llr_f32

SENT, PUNCTURED, SHORTENED = 0, 1, 2
LLR_KNOWN = np.float32(1048576.0)      # the LLR entrance's clamp, 2^20


def _pattern(pattern, n):
    p = np.zeros(n, dtype=np.uint8) if pattern is None else np.asarray(pattern, dtype=np.uint8)
    assert p.shape == (n,) and p.max(initial=0) <= SHORTENED
    return p


def channel_values(y32, sent, snr, pattern, quant=None):
    """float32 LLRs [frames, n] (quant None: the float handles) or int16 channel values (quant: the 7-tuple of a quantized
    handle).  sent: the symbol entrance's value for a float symbol; punctured: +0; shortened: +-2^20 / +-Cmax, + for bit 0"""
    y32 = np.asarray(y32)
    assert y32.dtype == np.float32 and y32.ndim == 2
    sent = np.asarray(sent)
    assert sent.shape == y32.shape
    p = _pattern(pattern, y32.shape[1])
    llr = channel_llr_f32(y32, snr, symbols_f32=True)
    assert llr.dtype == np.float32
    one = sent != 0
    if quant is None:
        out = llr.copy()
        out[:, p == PUNCTURED] = np.float32(0.0)
        out[:, p == SHORTENED] = np.where(one[:, p == SHORTENED], -LLR_KNOWN, LLR_KNOWN)
        return out
    cmax = limits(quant)[0]
    out = quantize_llr(llr, quant).astype(np.int16)
    out[:, p == PUNCTURED] = 0
    out[:, p == SHORTENED] = np.where(one[:, p == SHORTENED], -cmax, cmax)
    return out


def raw_errors(y32, sent, pattern):
    """int32 [frames]: the sent positions with (bit == 0 and y <= 0) or (bit == 1 and y > 0)"""
    y32 = np.asarray(y32)
    one = np.asarray(sent) != 0
    p = _pattern(pattern, y32.shape[1])
    with np.errstate(invalid="ignore"):
        wrong = np.where(one, y32 > 0, y32 <= 0)
    return wrong[:, p == SENT].sum(axis=1).astype(np.int32)


FIELDS = ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong", "sum_iters")


def counters(raw, bits, ok, iters, sent):
    """the seven counters of acg_ldpc_mc_result: correct <=> ok and the word equals the sent one on all n positions, pseudo <=> ok
    and they differ; the raw-error counts in place of the Hamming figures"""
    raw, ok, iters = np.asarray(raw).astype(np.int64), np.asarray(ok) != 0, np.asarray(iters).astype(np.int64)
    same = (np.asarray(bits) != 0) == (np.asarray(sent) != 0)
    correct = ok & same.all(axis=1)
    pseudo = ok & ~same.all(axis=1)
    return {"correct": int(correct.sum()), "pseudo": int(pseudo.sum()), "total": int(ok.size), "sum_hamming": int(raw.sum()),
            "sum_hamming_ok": int(raw[correct].sum()), "sum_hamming_wrong": int(raw[~correct].sum()), "sum_iters": int(iters.sum())}
