"""CPU: tests/spa_ref.py — the operation-exact restatement of the flooding sum-product kernels — tied to the independent
yardstick (`oracle.bp_decode`, 80-bit, direct exclude-self sums) before it judges any kernel (tests/test_spa_exact_gpu.py),
and the comparisons that file makes shown to bite.

  float64 restatement    identical to the oracle: word, flag AND exit iteration on every frame (golden frames of the three
                         matrices at four SNRs, the 192-frame case sets, two ragged graphs); float32 is MEASURED and printed
  both exits             every case set of the GPU file fails some frames and decodes some, after a few sweeps ... the budget
  mutants                six one-operation departures change a message word after two iterations on every traced set — and
                         no word, flag or exit iteration of the 576 frames of the case sets (the census is printed)
  knife edges            frames on which one message of the first iteration decides the flag: a message one ulp high or one
                         ulp low changes the flag vector, for every check degree 1 ... 8
  trace inversion        acg_ldpc_debug_bp_trace returns ln2 * double(word) for the float32 engines: dividing by ln2 and rounding
                         to float32 gives the word back, so the GPU file may compare bits"""
import numpy as np
import pytest

from golden_util import MATS, SNRS, load
from layered_ref import host_phi
from minsum_ref import Graph, channel_llr
from spa_cases import (SPA_FRAMES, SPA_SNR, SPA_TRACE_FRAMES, SPA_TRACE_SNRS, irregular, irregular_frames, ragged, ragged_frames,
                       spa_frames, wide_code, wide_frames)
from spa_ref import KNIFE_SNR, LN2, MUTANTS, flooding_sumproduct, host_phi64, knife_edge_case, mutant, ulp_fault



def _same(a, b):
    return (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[2] == b[2]).all()


@pytest.mark.parametrize("name", MATS)
def test_float64_restatement_equals_oracle(oracle, matrices, name):
    """prefix + suffix exclude-self sums with the hard bit's LSB cleared, in double with numpy's libm, against the oracle's
    80-bit direct sums: no frame may differ in word, flag or exit iteration.  The float32 restatement (log2(e)-scaled domain,
    layered_ref.host_phi) is measured against the same oracle and printed; observed: no frame of any set differs."""
    Hm = matrices[name]
    g = Graph(Hm)
    sets = [(snr, load(name, snr)["y"]) for snr in SNRS] + [(SPA_SNR[name], spa_frames(oracle, Hm, SPA_SNR[name])[1])]
    for snr, y in sets:
        want = oracle.bp_decode(Hm, y, snr, 50, threads=8)
        for ee in (True, False):
            assert _same(flooding_sumproduct(g, y, snr, 50, host_phi64, np.float64, early_exit=ee), want), (name, snr, ee)
        fb, fok, fit = flooding_sumproduct(g, y, snr, 50, host_phi, np.float32)
        same = (fok == want[1]) & (fb == want[0]).all(axis=1)
        print("%-9s %+5.1f dB float32: word+flag %d/%d  +iteration %d/%d" % (name, snr, same.sum(), len(y), (same & (fit == want[2])).sum(), len(y)))
    for it in (3, 1, 0):
        snr, y = sets[-1]
        assert _same(flooding_sumproduct(g, y, snr, it, host_phi64, np.float64), oracle.bp_decode(Hm, y, snr, it, threads=8)), (name, it)


def test_float64_restatement_equals_oracle_on_ragged_graphs(oracle):
    """one-variable checks (phi(+0) = +inf), an empty row, isolated and degree-1 variables"""
    Hi = irregular()
    for Hm, (y, snr), it in ((ragged(), ragged_frames(), 12), (Hi, irregular_frames(Hi.shape[1]), 30)):
        want = oracle.bp_decode(Hm, y, snr, it, threads=4)
        for ee in (True, False):
            assert _same(flooding_sumproduct(Hm, y, snr, it, host_phi64, np.float64, early_exit=ee), want), (Hm.shape, ee)
        assert 0 < want[1].sum()


def test_case_sets_take_both_exits(oracle, matrices):
    """the sets the GPU file decodes: some frames fail, some decode, and the exit iterations reach from a few sweeps to the
    budget.  Observed (ok of 192; exit iterations of the frames that decode): H05 -2 dB 174, 3..33; optimalH -2 dB 181, 3..49;
    H -1 dB 128, 2..50; ragged 0 dB 180, 1..11 of 12; irregular +1 dB 187, 2..10 of 30.  The frames that fail report the budget,
    so on every set the reported iterations reach from a few sweeps to max_iter."""
    Hi = irregular()
    sets = [(n, matrices[n], spa_frames(oracle, matrices[n], SPA_SNR[n])[1], SPA_SNR[n], 50) for n in MATS]
    sets.append(("ragged", ragged(), *ragged_frames(), 12))
    sets.append(("irregular", Hi, *irregular_frames(Hi.shape[1]), 30))
    for name, Hm, y, snr, it in sets:
        rb, rok, rit = flooding_sumproduct(Hm, y, snr, it, host_phi, np.float32)
        its = sorted(set(rit[rok == 1].tolist()))
        print("%-9s %+5.1f dB: %d of %d ok, exit iterations %d..%d (%d distinct), failed frames report %d"
              % (name, snr, rok.sum(), len(y), its[0], its[-1], len(its), it))
        assert len(y) == SPA_FRAMES and 0 < rok.sum() < len(y), (name, rok.sum())
        assert not rb[rok == 0].any() and (rit[rok == 0] == it).all() and rit.max() == it and rit.min() <= 3
        if name in MATS:
            assert its[0] <= 5 and its[-1] > 20 and len(its) > 8, (name, its)
        fixed = flooding_sumproduct(Hm, y, snr, it, host_phi, np.float32, early_exit=False)
        assert _same(fixed, (rb, rok, rit)), name


def _traced_sets(oracle, matrices):
    """(name, H, symbols, snr): what test_spa_exact_gpu.py traces — 64 frames each"""
    out = []
    for n in MATS:
        for snr in SPA_TRACE_SNRS:
            out.append(("%s %+.0f dB" % (n, snr), matrices[n], spa_frames(oracle, matrices[n], snr, SPA_TRACE_FRAMES)[1], snr))
    out.append(("ragged", ragged(), *ragged_frames(SPA_TRACE_FRAMES)))
    Hi = irregular()
    out.append(("irregular", Hi, *irregular_frames(Hi.shape[1], SPA_TRACE_FRAMES)))
    out.append(("wide", wide_code(), *wide_frames()))
    return out


def _words(trace):
    """what the GPU file compares: c->v bits, v->c bits without the LSB (the trace API strips it), the totals' bits"""
    c2v, v2c, post = trace
    U = np.uint32 if c2v.dtype == np.float32 else np.uint64
    return c2v.view(U), v2c.view(U) & ~U(1), post.view(U)


# exact symmetries, not gaps: with at most two edges per variable both orders of a sum are the same sum (ragged: variable degree
# <= 2), and x_k = llr + (pre + suf) has one non-zero partner
SYMMETRIES = {("ragged", "var_reverse"), ("ragged", "llr_first")}


def test_mutants_change_a_message_word_and_no_output(oracle, matrices):
    """Each departure changes at least one word of (c2v, v2c, totals) after two iterations on every traced set — the comparison of
    test_spa_exact_gpu.py a. sees it — while word, flag and exit iteration of the 3 x 192 frames of the case sets (50 sweeps) do
    not move: (bits, ok, iters) alone would let every one of them through.  Census (printed; host phi):

      mutant              words differing after 2 iterations, the 9 traced sets together    frames of 576 with another output
      total_minus_own     386083                                                              0
      var_reverse          21844  (totals only)                                               0
      llr_first           107598                                                              0
      phi_lsb_kept        162989                                                              0
      suffix_ascending    118902                                                              0
      check_lsb_kept      212800                                                              0

    var_reverse reaches no v->c or c->v word: x_k = llr + (pre_k + suf) is symmetric under it (prefix and suffix swap and their sum
    commutes); only s = ((c0 + c1) + c2) is not, so it shows in the totals — the streamed posterior word — and in the hard bit.
    The smallest counts per set are on the ragged graph (suffix_ascending: 13 words, its one degree-4 check).  The zero output
    census is asserted for all six."""
    traced = _traced_sets(oracle, matrices)
    census = {m: 0 for m in MUTANTS}
    for name, Hm, y, snr in traced:
        g = Graph(Hm)
        base = _words(flooding_sumproduct(g, y, snr, 0, host_phi, np.float32, trace_at=2)[3])
        for m in MUTANTS:
            got = _words(flooding_sumproduct(g, y, snr, 0, host_phi, np.float32, trace_at=2, fault=mutant(m))[3])
            diff = [int((a != b).sum()) for a, b in zip(got, base)]
            census[m] += sum(diff)
            print("%-16s %-18s words differing (c2v, v2c, totals): %s" % (name, m, diff))
            if (name.split()[0], m) in SYMMETRIES:
                assert sum(diff) == 0, (name, m)
            else:
                assert sum(diff) > 0, (name, m, "invisible at word level")
    moved = {m: 0 for m in MUTANTS}
    for n in MATS:
        Hm, snr = matrices[n], SPA_SNR[n]
        g = Graph(Hm)
        y = spa_frames(oracle, Hm, snr)[1]
        rb, rok, rit = flooding_sumproduct(g, y, snr, 50, host_phi, np.float32)
        for m in MUTANTS:
            mb, mok, mit = flooding_sumproduct(g, y, snr, 50, host_phi, np.float32, fault=mutant(m))
            moved[m] += int(((mok != rok) | (mit != rit) | (mb != rb).any(axis=1)).sum())
    for m in MUTANTS:
        print("%-18s %-90s words %8d   frames of %d with another word, flag or exit iteration: %d"
              % (m, MUTANTS[m], census[m], 3 * SPA_FRAMES, moved[m]))
    assert all(moved[m] == 0 for m in MUTANTS), moved     # what (bits, ok, iters) alone would let through


@pytest.mark.parametrize("absorbed", [False, True])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_knife_edges_see_one_ulp(dt, absorbed):
    """spa_ref.knife_edge_case with the host phi: per check degree the frames kept, and a message of that degree one bit pattern
    higher / lower changes the flag vector of the restatement at max_iter = 1.  Degree 1 sends +inf: one lower (the largest
    finite number) is caught; one higher is a NaN, which no compare tells from +inf — asserted to change nothing, so that
    nobody reads the set as covering it.
    Drops (frames of 40 per degree for which no double symbol gives the LLR exactly): none for either type at KNIFE_SNR = 0 dB,
    where sigma^2 = 1/2 and the double LLR 2 * y / sigma^2 = 4 y is exact (at +1 dB float64 loses up to 9 of 40 per degree)."""
    phi = host_phi if dt == np.float32 else host_phi64
    frames = 320
    Hm, y, knife, kind_b, dropped = knife_edge_case(phi, KNIFE_SNR, frames, 3, dt, absorbed)
    degs = Hm.sum(axis=1).astype(int)
    print("%s knife edges%s: %d of %d frames kept; dropped per degree 1..8: %s" % (np.dtype(dt).name, ", absorbed graph" if absorbed else "", len(y), frames, dropped.tolist()))
    assert (dropped <= frames // 8 // 4).all(), dropped
    g = Graph(Hm)
    rb, rok, rit, (c2v, v2c, post) = flooding_sumproduct(g, y, KNIFE_SNR, 1, phi, dt, trace_at=1)
    pk = post[np.arange(len(y)), knife]
    assert (pk[~kind_b] == 0).all() and (pk[kind_b] > 0).all()          # totals of exactly +0 (hard = 1) / just above (hard = 0)
    _, ok, it = flooding_sumproduct(g, y, KNIFE_SNR, 1, phi, dt)
    assert 0 < ok.sum() < len(y) and (it == 1).all()
    for d in range(1, 9):
        for k in (+1, -1):
            _, mok, _ = flooding_sumproduct(g, y, KNIFE_SNR, 1, phi, dt, fault=ulp_fault(d, k))
            changed = np.nonzero(mok != ok)[0]
            if d == 1 and k == +1:
                assert len(changed) == 0
                continue
            assert len(changed) > 0, (d, k)
            assert (degs[np.nonzero(Hm[:, knife[changed]].T)[1]] == d).all()      # (only frames that target this degree)
            # kind A sees "high", kind B sees "low" (the check's other variables receive a moved message too, and at degree 2,
            # where it is as large as their own LLR, some flip on it: frames of the other kind may change as well)
            assert (kind_b[changed] == (k < 0)).any(), (d, k)


def test_trace_doubles_give_the_float32_words_back():
    rng = np.random.default_rng(11)
    w = rng.integers(0, 1 << 32, size=1_000_000, dtype=np.uint64).astype(np.uint32)
    special = np.array([0, 0x80000000, 1, 2, 0x007FFFFF, 0x00800000, 0x80000001, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000],
                       dtype=np.uint32)
    w = np.concatenate([w, special]).view(np.float32)
    with np.errstate(invalid="ignore"):
        t = LN2 * w.astype(np.float64)
        back = (t / LN2).astype(np.float32)
    nan = np.isnan(w)
    assert (back[~nan].view(np.uint32) == w[~nan].view(np.uint32)).all()
    assert np.isnan(back[nan]).all() and 1000 < nan.sum()


def test_restatement_reads_the_llr_paths_of_minsum_ref(oracle, matrices):
    """float symbols take the other LLR path; the two differ on few frames and both are restated (minsum_ref.channel_llr)"""
    Hm = matrices["H05"]
    y = spa_frames(oracle, Hm, -2.0, 64)[1]
    a = channel_llr(y, -2.0, np.float32)
    b = channel_llr(y.astype(np.float32), -2.0, np.float32)
    assert a.dtype == b.dtype == np.float32 and (a != b).any()
    r32 = flooding_sumproduct(Hm, y.astype(np.float32), -2.0, 50, host_phi, np.float32)
    assert 0 < r32[1].sum() < 64
