"""GPU: the one classification kernel behind acg_ldpc_mc_run (engines that classify in a separate kernel),
acg_ldpc_mc_run_grid and acg_ldpc_mc_run_codes, against an expectation it never computes: the symbols of acg_ldpc_awgn_dev,
decoded through decode_batch_dev on the same parameters, classified by the numpy restatement tests/mc_detail_ref.py.
The seven counters must be equal.  Shapes: 1 frame (one wavefront has work), 257, and 1001 — with 9 or more units that is
more virtual frames than the launch has wavefronts (8192), so a wavefront takes a run of frames that crosses a unit."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mc_detail_ref as R  # noqa: E402
from mc_decode_path import decode_device_noise, sent_words  # noqa: E402
import test_mc_codes_gpu as TC  # noqa: E402  (the protograph helpers of the batch-of-codes tests)

pytestmark = pytest.mark.gpu

INT_FIELDS = ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong", "sum_iters")
FRAMES = 1001
FIRST = (1 << 33) + 5         # the high half of the global frame index matters
NCW = 7                       # codewords cycle with a period that divides nothing


def ints(r):
    return tuple(getattr(r, f) for f in INT_FIELDS)


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    return A


@pytest.fixture(scope="module")
def codes(A):
    """name -> (ParityCheckMatrix, dense H, 7 codewords)"""
    out = {}
    for name, H in (("H05", A.read_pcm(os.path.join(DATA, "H05.txt"))), ("reg40", A.ParityCheckMatrix(A.regular_ldpc(20, 40, 3, 6)))):
        G, ok = H.get_orthogonal()
        assert ok
        out[name] = (H, H.dense(), A.gen_random_codewords(G, NCW, 2024))
    return out


class Decoded:
    """what a decoder returned for global frames [FIRST, FIRST + frames), decoded once; expect(F) classifies the first F"""

    def __init__(self, A, dec, H, Hd, cws, snr, seed, frames=FRAMES):
        self.out = decode_device_noise(A, dec, H, cws, snr, frames, FIRST, seed)
        self.sent, self.Hd = sent_words(cws, H.n, FIRST, frames), Hd

    def expect(self, frames=None):
        y, words, ok, it = (x[:frames] for x in self.out)
        c = R.mc_detail(y, words, ok, it, self.sent[:frames], self.Hd, first_frame=FIRST)[0]
        return tuple(c[f] for f in INT_FIELDS)


def single_unit_decoders(A):
    """engines whose acg_ldpc_mc_run classifies in a separate kernel -> (constructor, code, snr, seed): the settings
    tests/test_mc_detail_gpu.py documents as producing pseudo and no-word frames"""
    return {
        "bp_streamed": (lambda: A.BeliefPropagationDecoder(50, engine=A.ENGINE_STREAMED), "H05", -2.0, 2),
        "ms_layered_block256": (lambda: A.MinSumDecoder(25, 0.75, schedule=A.SCHEDULE_LAYERED, lanes_per_frame=256), "H05", -2.0, 2),
        "ms_pair_f16": (lambda: A.MinSumDecoder(50, 0.75, precision=A.PREC_F16), "reg40", 0.0, 1),   # n = 40: the last word is partly used
    }


@pytest.mark.parametrize("name", ["bp_streamed", "ms_layered_block256", "ms_pair_f16"])
def test_single_unit(A, codes, name):
    make, code, snr, seed = single_unit_decoders(A)[name]
    H, Hd, cws = codes[code]
    dec = make()
    ref = Decoded(A, dec, H, Hd, cws, snr, seed)
    for frames in (1, 257, FRAMES):
        want = ref.expect(frames)
        got = ints(A.run_experiment(dec, cws, H, snr, frames=frames, first_frame=FIRST, noise="device", seed=seed))
        print(name, frames, got, want)
        assert got == want, frames
    assert 0 < want[0] < want[2] == FRAMES     # some frames correct, some not: the equality is not vacuous
    # the all-zero word
    want = Decoded(A, dec, H, Hd, None, snr, seed, frames=257).expect()
    got = ints(A.run_experiment(dec, None, H, snr, frames=257, first_frame=FIRST, noise="device", seed=seed))
    print(name, "codewords=None", got, want)
    assert got == want
    dec.close()


def test_grid(A, codes):
    """>= 9 decoding points and a guard point at 1001 frames: >= 9009 virtual frames for 8192 wavefronts"""
    H, Hd, cws = codes["H05"]
    snr, seed, sweeps = -2.0, 2, 100
    e_min = H.admm_shape()["e_min"]
    cand = [(a, m) for a in (0.4, 0.8, 1.2, 1.6, 1.95) for m in (0.3, 0.5, 0.7, 0.9)]
    run = [p for p in cand if not e_min * p[1] <= p[0]][:9]      # qp_admm.h:108-114
    guard = [p for p in cand if e_min * p[1] <= p[0]][:1] + [(e_min * 0.5, 0.5)]
    assert len(run) == 9 and len(guard) >= 1
    points = run[:4] + guard[:1] + run[4:] + guard[1:]              # guard points between and behind the decoding ones
    dec = A.QPADMMDecoder(1.95, 0.5, sweeps, fast_setup=True)
    assert "mc_grid=single-launch" in dec.describe(H)
    got = A.run_experiment_grid(dec, cws, H, snr, [p[0] for p in points], [p[1] for p in points], frames=FRAMES, first_frame=FIRST,
                                noise="device", seed=seed)
    assert len(got) == len(points)
    raw = None
    for (a, m), r in zip(points, got):
        if (a, m) in guard:
            continue
        own = A.QPADMMDecoder(a, m, sweeps, fast_setup=True)
        want = Decoded(A, own, H, Hd, cws, snr, seed).expect()
        own.close()
        print("grid", a, m, ints(r), want)
        assert ints(r) == want, (a, m)
        raw = want[3]
    n_ok = sum(r.correct for r in got)
    assert 0 < n_ok < FRAMES * len(run)
    for (a, m), r in zip(points, got):
        if (a, m) in guard:
            assert (r.correct, r.pseudo, r.sum_iters, r.total, r.sum_hamming_ok) == (0, 0, 0, FRAMES, 0), (a, m)
            assert r.sum_hamming == r.sum_hamming_wrong == raw, (a, m)
    dec.close()


def test_codes(A):
    """nine codes of one m x n: H05 and single-block mutations of it, each with its own 7 codewords"""
    P0 = TC.proto_of(A.read_pcm(os.path.join(DATA, "H05.txt")).dense())
    present = np.argwhere(P0 >= 0)
    batch = [TC.make_code(A, P0)]
    for k in range(1, 30):
        if len(batch) == 9:
            break
        P = P0.copy()
        at = tuple(present[(3 * k) % len(present)])
        P[at] = (P[at] + k) % TC.Z     # one shift changed
        try:
            batch.append(TC.make_code(A, P))
        except AssertionError:   # (no generator for this mutation)
            continue
    assert len(batch) == 9
    batch = [(H, np.ascontiguousarray(cws[:NCW]), e) for H, cws, e in batch]
    alpha = TC.safe_alpha(batch)
    snr, seed = TC.SNR, 11
    ev = A.CodesEvaluator(A.QPADMMDecoder(alpha, TC.MU, TC.ITERS, 1e-5))
    got = ev.run([(H, cws) for H, cws, _ in batch], snr, frames=FRAMES, first_frame=FIRST, noise="device", seed=seed)
    d = ev.describe()
    ev.close()
    assert "mc_codes=single-launch" in d and "per_code=0" in d, d
    for k, (H, cws, _) in enumerate(batch):
        own = A.QPADMMDecoder(alpha, TC.MU, TC.ITERS, 1e-5, fast_setup=True)
        want = Decoded(A, own, H, H.dense(), cws, snr, seed).expect()
        own.close()
        print("code", k, ints(got[k]), want)
        assert ints(got[k]) == want, k
    assert 0 < sum(r.correct for r in got) < FRAMES * len(batch)
