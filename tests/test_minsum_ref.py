"""CPU: tests/minsum_ref.py — the operation-exact restatement of the flooding min-sum kernels — tied to the independent
yardstick (`oracle.minsum_decode`, plain double, its own summation order) before it judges any kernel
(tests/test_minsum_exact_gpu.py).

  float64 restatement   identical to the oracle: word, flag AND exit iteration on every frame (3 matrices x 2 SNRs that straddle
                        the waterfall x 2 scales x 600 frames, plus two ragged graphs)
  float32 / float16     may part from the double oracle: the agreement rates are MEASURED and printed; on H05 they are asserted
                        not to fall below what was observed (one frame in 600 of margin) — see the table in
                        test_float32_float16_agreement_is_measured
  the restatement alone all-zero-codeword symmetry, max_iter = 0, fixed work == early exit"""
import numpy as np
import pytest

from minsum_ref import Graph, flooding_minsum

# two SNRs (Es/N0, dB) per matrix that straddle the min-sum waterfall: FER(scale 0.75, 50 sweeps) = 0.74 / 0.06 (H),
# 0.16 / 0.003 (H05), 0.56 / 0.008 (optimalH)
STRADDLE = {"H": (-2.0, 0.0), "H05": (-2.0, -1.0), "optimalH": (-3.0, -1.0)}
FRAMES = 600


def _frames(oracle, Hm, snr, frames=FRAMES):
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 5, frames)
    return cws, oracle.transmit_frames(cws, snr, first_seed=99)


def _ragged():
    """the graph of test_gpu_parity.test_bp_edge_cases: degree-1 check (its message is inf * scale), degree-2 check, an empty
    row, two isolated variables"""
    H = np.zeros((5, 9), np.uint8)
    H[0, [0, 1, 2, 3]] = 1
    H[1, [2, 3, 4]] = 1
    H[2, [5]] = 1
    H[3, [0, 6]] = 1
    return H


def _mixed():
    """the irregular graph of test_gpu_parity.test_pair_f16_minsum_kernels (b): variable degree 2..4, check degree <= 8"""
    Hi = np.zeros((300, 600), np.uint8)
    r2 = np.random.default_rng(8)
    for v in range(600):
        Hi[r2.choice(300, size=2 + (v % 3), replace=False), v] = 1
    Hi = Hi[(Hi.sum(1) >= 2)].copy()
    for i in np.nonzero(Hi.sum(1) > 8)[0]:
        Hi[i, np.nonzero(Hi[i])[0][8:]] = 0
    return Hi


@pytest.mark.parametrize("name", ["H", "H05", "optimalH"])
def test_float64_restatement_equals_oracle(oracle, matrices, name):
    """prefix + suffix exclude-self sums with the hard bit's LSB cleared against the oracle's direct sums: no frame may differ
    in word, flag or exit iteration.  (A genuine double knife edge between the two summation orders would be pinned here by
    frame, with the reason; none was met.)"""
    Hm = matrices[name]
    g = Graph(Hm)
    for snr in STRADDLE[name]:
        _, y = _frames(oracle, Hm, snr)
        for scale in (1.0, 0.75):
            ob, ook, oit = oracle.minsum_decode(Hm, y, snr, 50, scale, threads=8)
            rb, rok, rit = flooding_minsum(g, y, snr, 50, scale, np.float64)
            assert (rb == ob).all() and (rok == ook).all() and (rit == oit).all(), (name, snr, scale)
    fers = []
    for snr in STRADDLE[name]:
        _, y = _frames(oracle, Hm, snr)
        fers.append(1 - oracle.minsum_decode(Hm, y, snr, 50, 0.75, threads=8)[1].mean())
    assert fers[0] > 0.15 and fers[1] < 0.07, fers            # the two SNRs really straddle the waterfall


def test_float64_restatement_equals_oracle_on_ragged_graphs(oracle):
    rng = np.random.default_rng(3)
    cases = [(_ragged(), 1.0 + 0.9 * rng.standard_normal((600, 9)), 0.0, 12)]
    Hi = _mixed()
    assert Hi.sum(1).min() >= 2 and Hi.sum(1).max() <= 8 and set(Hi.sum(0)) <= {0, 1, 2, 3, 4} and len(set(Hi.sum(0))) > 2
    for snr in (1.0, 4.0):
        sig = np.sqrt(10.0 ** (-snr / 10.0) / 2.0)
        cases.append((Hi, 1.0 + sig * rng.standard_normal((500, Hi.shape[1])), snr, 30))
    for Hm, y, snr, it in cases:
        for scale in (1.0, 0.75):
            ob, ook, oit = oracle.minsum_decode(Hm, y, snr, it, scale, threads=4)
            for ee in (True, False):
                rb, rok, rit = flooding_minsum(Hm, y, snr, it, scale, np.float64, early_exit=ee)
                assert (rb == ob).all() and (rok == ook).all() and (rit == oit).all(), (Hm.shape, snr, scale, ee)
            assert 0 < ook.sum()


# H05, scale 0.75, 50 sweeps, 600 frames (codewords seed 5, noise seeds 99..): what the restatements were observed to do
# against the double oracle; the test allows one frame in 600 less, for another draw.
# {dtype: {snr: (frames equal in word + flag, frames equal in exit iteration too)}}
OBSERVED_H05 = {np.float32: {-2.0: (600, 600), -1.0: (600, 600)}, np.float16: {-2.0: (600, 596), -1.0: (600, 599)}}


def test_float32_float16_agreement_is_measured(oracle, matrices):
    """How far honest float32 / float16 rounding moves min-sum results off the double oracle — a MEASUREMENT, printed (run with
    -s), so that nobody reintroduces a 99.5 % bar on the kernels: the kernels are held to the restatement of their own type,
    exactly.  Only H05 at scale 0.75 is asserted, as a floor.  Measured (frames of 600 equal to the oracle in word + flag /
    also in exit iteration; 50 sweeps; in brackets the largest difference in exit iteration among the frames with equal word):

      matrix    SNR    scale   float32          float16
      H         -2.0   0.75    600 / 600 (0)    594 / 582 (11)
      H          0.0   0.75    600 / 600 (0)    594 / 583 (5)
      H05       -2.0   0.75    600 / 600 (0)    600 / 596 (2)
      H05       -1.0   0.75    600 / 600 (0)    600 / 599 (1)
      optimalH  -3.0   0.75    600 / 600 (0)    600 / 593 (5)
      optimalH  -1.0   0.75    600 / 600 (0)    600 / 599 (1)
      H         -2.0   1.0     585 / 576 (8)    584 / 564 (27)
      H          0.0   1.0     591 / 584 (7)    579 / 552 (24)
      H05       -2.0   1.0     598 / 595 (2)    581 / 549 (20)
      H05       -1.0   1.0     600 / 599 (1)    597 / 592 (20)
      optimalH  -3.0   1.0     598 / 595 (1)    580 / 548 (15)
      optimalH  -1.0   1.0     600 / 600 (0)    598 / 591 (8)

    With scale 0.75 float32 rounding moved no frame of 3600.  Scale 1.0 is another matter: the messages are then copies of
    channel LLRs, sums of them cancel to exactly zero in double (where x <= 0 decides for -1) and to a last-bit residue in the
    log2(e) domain of the float32 kernels or on the half-precision grid — a property of that scale, not of a kernel."""
    for name in ("H", "H05", "optimalH"):
        Hm = matrices[name]
        g = Graph(Hm)
        for snr in STRADDLE[name]:
            _, y = _frames(oracle, Hm, snr)
            for scale in (0.75, 1.0):
                ob, ook, oit = oracle.minsum_decode(Hm, y, snr, 50, scale, threads=8)
                for dt in (np.float32, np.float16):
                    rb, rok, rit = flooding_minsum(g, y, snr, 50, scale, dt)
                    same = (rok == ook) & (rb == ob).all(axis=1)
                    n_wf, n_it = int(same.sum()), int((same & (rit == oit)).sum())
                    print("%-9s %5.1f dB scale %.2f %-8s word+flag %d/%d  +iteration %d/%d  max |iteration difference| %d"
                          % (name, snr, scale, np.dtype(dt).name, n_wf, FRAMES, n_it, FRAMES, int(np.abs(rit - oit)[same].max())))
                    if name == "H05" and scale == 0.75:
                        want_wf, want_it = OBSERVED_H05[dt][snr]
                        assert n_wf >= want_wf - 1 and n_it >= want_it - 1, (np.dtype(dt).name, snr, n_wf, n_it)


@pytest.mark.parametrize("dt", [np.float64, np.float32, np.float16])
def test_restatement_properties(oracle, matrices, dt):
    Hm = matrices["H05"]
    g = Graph(Hm)
    cws, y = _frames(oracle, Hm, -1.5, 300)
    rb, rok, rit = flooding_minsum(g, y, -1.5, 50, 0.75, dt)
    assert 0 < rok.sum() < len(rok) and len(set(rit[rok == 1].tolist())) > 5
    # every word returned with ok = 1 is a codeword; failed frames return the empty word and the budget
    assert not ((rb[rok == 1].astype(np.int64) @ Hm.T.astype(np.int64)) & 1).any()
    assert not rb[rok == 0].any() and (rit[rok == 0] == 50).all()
    # fixed work latches the outputs of early exit
    fb, fok, fit = flooding_minsum(g, y, -1.5, 50, 0.75, dt, early_exit=False)
    assert (fb == rb).all() and (fok == rok).all() and (fit == rit).all()
    # all-zero-codeword symmetry: the same noise on the all-zero word decodes to the same error pattern, at the same sweep
    # Every rule is odd in the LLRs but for x == 0 exactly (sign -1 whatever was sent, bp.h:82): scale 0.75 produces no exact
    # zero in float64 / float32 on these frames; on the 11-bit grid of float16 sums do cancel exactly, so there the symmetry
    # is not a property of the algorithm and is not asked.
    if dt != np.float16:
        zb, zok, zit = flooding_minsum(g, y * (1.0 - 2.0 * cws), -1.5, 50, 0.75, dt)
        assert (zok == rok).all() and (zit == rit).all() and (zb[rok == 1] == (rb ^ cws)[rok == 1]).all()
    # float symbols take the other LLR path (one double multiply): same decisions on all but knife-edge frames, and clean
    # codewords come back after one sweep on either path
    clean = 1.0 - 2.0 * cws.astype(np.float64)
    for yy in (clean, clean.astype(np.float32)):
        cb, cok, cit = flooding_minsum(g, yy, 2.0, 50, 0.75, dt)
        assert cok.all() and (cb == cws).all() and (cit == 1).all()
    # max_iter = 0 never converges (bp.h:195), max_iter = 1 allows exactly one sweep
    b0, k0, i0 = flooding_minsum(g, clean, 2.0, 0, 0.75, dt)
    assert not k0.any() and not b0.any() and (i0 == 0).all()
    b1, k1, i1 = flooding_minsum(g, y, -1.5, 1, 0.75, dt)
    assert (i1 == 1).all() and (k1 == (rit == 1)).all() and (b1[k1 == 1] == rb[k1 == 1]).all()


def test_a_rare_wrong_second_minimum_passes_a_rate_and_fails_exact_comparison(oracle, matrices):
    """The kind of fault agreement rates hide: the last edge of every degree-7 check of H05 (20 of 160 checks) receives the
    first minimum where it should receive the second.  At -1 dB nearly every frame still decodes to the word the oracle
    finds (the rate is printed: 0.9933 of these 600 frames, 0.992 of the 2000 of test_minsum_against_own_restatement), while
    the comparison the kernels are held to — word, flag and exit iteration against the unmutated restatement of the same
    type — fails on 171 of the 600 frames."""
    Hm = matrices["H05"]
    g = Graph(Hm)
    _, y = _frames(oracle, Hm, -1.0)

    def fault(d, out, m1s, m2s):
        if d == 7:
            out[:, :, d - 1] = m1s
    ob, ook, oit = oracle.minsum_decode(Hm, y, -1.0, 50, 0.75, threads=8)
    rb, rok, rit = flooding_minsum(g, y, -1.0, 50, 0.75, np.float32)
    mb, mok, mit = flooding_minsum(g, y, -1.0, 50, 0.75, np.float32, fault=fault)
    rate = ((mok == ook) & (mb == ob).all(axis=1)).mean()
    differ = int(((mok != rok) | (mb != rb).any(axis=1) | (mit != rit)).sum())
    print("wrong second minimum on 1 edge of the degree-7 checks: word + flag agree with the oracle on %.4f of %d frames; "
          "%d frames differ from the exact restatement" % (rate, FRAMES, differ))
    assert (Hm.sum(1) == 7).sum() > 0 and differ > 0
