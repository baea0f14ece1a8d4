"""CPU: the numpy restatement of the detail run (tests/mc_detail_ref.py) on hand-built frames whose answers are written
out here.  The GPU tests use that restatement as their expectation, so it is pinned first."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mc_detail_ref as R  # noqa: E402


@pytest.fixture(scope="module", params=["H.txt", "H05.txt"])
def case(request):
    """data/H.txt: n = 128, whole words.  data/H05.txt: n = 280, 24 live bits in the last word, the other 8 filled with
    garbage below.  The pseudo frames are built from real codewords: rows of the generator get_orthogonal returns."""
    import acg_alp_ldpc_amd as A
    A.build()
    H = A.read_pcm(os.path.join(ROOT, "data", request.param)).dense()
    n = H.shape[1]
    G, ok = A.ParityCheckMatrix(H).get_orthogonal()
    assert ok and G.shape[1] == n and G.shape[0] >= 3
    assert not ((H.astype(int) @ G.T.astype(int)) & 1).any()        # rows of G are codewords of H
    c1, c2 = G[0].copy(), G[1].copy()
    w1 = int(c1.sum())
    assert w1 > 0 and c2.any() and (c1 != c2).any()
    return H, n, c1, c2, w1


def garbage(n):
    """ones in the unused bits of the last word (none when n is a multiple of 32)"""
    return np.uint32((0xFFFFFFFF << (n & 31)) & 0xFFFFFFFF) if n & 31 else np.uint32(0)


def build_frames(case):
    H, n, c1, c2, w1 = case
    m = H.shape[0]
    sent = np.zeros((7, n), dtype=np.uint8)
    sent[1] = c2                                     # frame 1 transmits c2, everything else the zero word
    out = np.zeros((7, n), dtype=np.uint8)
    ok = np.ones(7, dtype=np.uint8)
    # 0: correct (zero word returned for the zero word)
    # 1: pseudo: c2 sent, c1 ^ c2 returned -> word ^ sent = c1, weight w1
    out[1] = c1 ^ c2
    # 2: flag false: whatever lies in the word buffer is ignored
    ok[2] = 0
    out[2] = 1
    # 3: flag set, not a codeword: exactly one bit set -> the checks of that column are unsatisfied
    col = int(np.argmax(H.sum(axis=0)))
    out[3, col] = 1
    # 4: pseudo again, the same weight w1 (c1 returned for the zero word): the tie goes to frame 1
    out[4] = c1
    # 5: correct;  6: flag false
    ok[6] = 0
    y = 1.0 - 2.0 * sent.astype(np.float64)
    y[0, :3] = -0.5                                  # three raw errors on a correct frame
    y[1, 0] = 0.25 if sent[1, 0] else -0.25          # one raw error on the first pseudo frame
    y[2, :5] = 0.0                                   # y == 0 reads as 1: five raw errors (sent 0)
    y[3, 7] = -2.0
    words = R.pack_bits(out)
    words[:, -1] |= garbage(n)                       # garbage in the unused bits of the last word
    iters = np.array([2, 9, 50, 100, 11, 1, 50], dtype=np.int32)
    return sent, out, ok, y, words, iters, int(H[:, col].sum())


def test_pack_roundtrip():
    rng = np.random.default_rng(0)
    b = rng.integers(0, 2, size=(5, 100), dtype=np.uint8)
    w = R.pack_bits(b)
    assert w.shape == (5, 4) and w.dtype == np.uint32
    assert (w[:, 3] >> 4 == 0).all()
    assert w[0, 0] & 1 == b[0, 0] and (w[2, 1] >> 5) & 1 == b[2, 37]
    assert (R.unpack_bits(w | np.array([0, 0, 0, 0xFFFFFFF0], dtype=np.uint32), 100) == b).all()


def test_counters_and_events_of_the_hand_built_frames(case):
    H, n, c1, c2, w1 = case
    sent, out, ok, y, words, iters, colw = build_frames(case)
    first = (1 << 33) + 5
    c, ev, rows = R.mc_detail(y, words, ok, iters, sent, H, first_frame=first, cap=10)
    assert c == dict(correct=2, pseudo=2, total=7, sum_hamming=3 + 1 + 5 + 1, sum_hamming_ok=3, sum_hamming_wrong=7,
                     sum_iters=223, word_frames=5, bit_errors=2 * w1 + 1, noncodeword_frames=1, sum_syndrome_weight=colw,
                     n_events=5, n_stored=5, min_pseudo_weight=w1, min_pseudo_frame=first + 1)
    assert colw >= 1
    assert ev["frame"].tolist() == [first + k for k in (1, 2, 3, 4, 6)]
    assert ev["kind"].tolist() == [R.EVENT_PSEUDO, R.EVENT_NO_WORD, R.EVENT_NONCODEWORD, R.EVENT_PSEUDO, R.EVENT_NO_WORD]
    assert ev["iters"].tolist() == [9, 50, 100, 11, 50]
    assert ev["raw_errors"].tolist() == [1, 5, 1, 0, 0]
    assert ev["bit_errors"].tolist() == [w1, 0, 1, w1, 0]
    assert ev["syndrome_weight"].tolist() == [0, 0, colw, 0, 0]
    assert (ev["reserved"] == 0).all() and ev.dtype.itemsize == 32
    # XOR rows: word ^ sent with the garbage bits gone, zeros for NO_WORD
    assert rows.shape == (5, (n + 31) // 32) and rows.dtype == np.uint32
    assert (R.unpack_bits(rows, n) == np.stack([c1, np.zeros(n, np.uint8), out[3], c1, np.zeros(n, np.uint8)])).all()
    assert (rows[:, -1] & garbage(n) == 0).all()


def test_tie_on_min_pseudo_weight_takes_the_lower_frame(case):
    H, n, c1, c2, w1 = case
    sent, out, ok, y, words, iters, _ = build_frames(case)
    # swap frames 1 and 4: the other pseudo frame is now first, same weight
    p = np.array([0, 4, 2, 3, 1, 5, 6])
    c, _, _ = R.mc_detail(y[p], words[p], ok[p], iters[p], sent[p], H, first_frame=100, cap=0)
    assert (c["min_pseudo_weight"], c["min_pseudo_frame"]) == (w1, 101)
    # a lighter pseudo word later in the run wins over the earlier heavier ones
    G, _ = __import__("acg_alp_ldpc_amd").ParityCheckMatrix(H).get_orthogonal()
    ws = G.sum(axis=1)
    if ws.min() < w1:
        out2 = out.copy()
        out2[5] = G[int(np.argmin(ws))]
        c, _, _ = R.mc_detail(y, R.pack_bits(out2), ok, iters, sent, H, first_frame=0, cap=0)
        assert (c["min_pseudo_weight"], c["min_pseudo_frame"]) == (int(ws.min()), 5)


@pytest.mark.parametrize("cap,stored", [(0, 0), (1, 1), (5, 5), (9, 5)])
def test_cap(case, cap, stored):
    H, n, c1, c2, w1 = case
    sent, out, ok, y, words, iters, _ = build_frames(case)
    c, ev, rows = R.mc_detail(y, words, ok, iters, sent, H, first_frame=0, cap=cap)
    assert c["n_events"] == 5 and c["n_stored"] == stored == len(ev) == len(rows)
    assert ev["frame"].tolist() == [1, 2, 3, 4, 6][:stored]          # the lowest frames, ascending
    assert rows.shape == (stored, (n + 31) // 32)


def test_no_pseudo_frame_and_empty_run(case):
    H, n, *_ = case
    c, ev, rows = R.mc_detail(np.ones((2, n)), np.zeros((2, (n + 31) // 32), np.uint32), [1, 0], [3, 4], np.zeros((2, n), np.uint8), H, cap=4)
    assert (c["min_pseudo_weight"], c["min_pseudo_frame"], c["n_events"], c["word_frames"], c["bit_errors"]) == (-1, -1, 1, 1, 0)
    assert ev["kind"].tolist() == [R.EVENT_NO_WORD]
    c, ev, rows = R.mc_detail(np.ones((0, n)), np.zeros((0, (n + 31) // 32), np.uint32), [], [], np.zeros((0, n), np.uint8), H, cap=4)
    assert c["total"] == 0 and c["n_events"] == 0 and len(ev) == 0 and rows.shape == (0, (n + 31) // 32)


def test_merge_of_two_shards_equals_the_whole(case):
    H, n, c1, c2, w1 = case
    sent, out, ok, y, words, iters, _ = build_frames(case)
    whole = R.mc_detail(y, words, ok, iters, sent, H, first_frame=40, cap=3)
    for cut in (1, 2, 4, 5):
        a = R.mc_detail(y[:cut], words[:cut], ok[:cut], iters[:cut], sent[:cut], H, first_frame=40, cap=3)
        b = R.mc_detail(y[cut:], words[cut:], ok[cut:], iters[cut:], sent[cut:], H, first_frame=40 + cut, cap=3)
        for x, yy in ((a, b), (b, a)):
            c, ev, rows = R.merge(x, yy, 3)
            assert c == whole[0]
            assert (ev == whole[1]).all() and (rows == whole[2]).all()


def test_python_mirror_merges_like_the_restatement(case):
    """merge_exp_details (acg_alp_ldpc_amd.experiment) on ExperimentDetail objects built from the restatement"""
    import acg_alp_ldpc_amd as A
    H, n, c1, c2, w1 = case
    sent, out, ok, y, words, iters, _ = build_frames(case)

    def obj(lo, hi, cap):
        c, ev, rows = R.mc_detail(y[lo:hi], words[lo:hi], ok[lo:hi], iters[lo:hi], sent[lo:hi], H, first_frame=lo, cap=cap)
        return A.ExperimentDetail(n=n, cap=cap, events=ev, words=rows, **c)
    whole = obj(0, 7, 3)
    m = A.merge_exp_details(obj(4, 7, 3), obj(0, 4, 3))
    for f in R.COUNTERS:
        assert getattr(m, f) == getattr(whole, f), f
    assert (m.events == whole.events).all() and (m.words == whole.words).all()
    assert m.BER() == (2 * w1 + 1) / (7 * n) and m.FER() == 5 / 7
    assert A.experiment.EVENT_DTYPE == R.EVENT_DTYPE
