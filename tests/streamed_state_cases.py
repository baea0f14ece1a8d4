"""What the tests of the streamed layered engines' STATE share (tests/test_streamed_state.py on the CPU,
tests/test_streamed_state_gpu.py on the device): the `tails` graph, its symbols, and the posteriors and messages of the
restatements on them (tests/layered_ref.py: layered_minsum, layered_sumproduct_exact; tests/streamed_q_ref.py:
decode_int_sparse), computed once per (rule, iterations, phi, symbol type).

  tails   23 x 120, plain numpy from a fixed seed, not quasi-cyclic: ONE check of each degree 1 ... 17, 21, 22, 29, 30, 33, 40 —
          every instance of the one-pass step (1 ... 8) and, among the wide checks, a short last chunk of every length 1 ... 7
          behind one, two and three full chunks of 8 edges (9 ... 15, 17; 21, 22; 29, 30) as well as none (16, 40) and four
          full chunks (33, 40) — on variables that most checks share, so that from the second iteration on every check
          subtracts messages another iteration stored.

The all-zero word is sent, 101 frames: one full tile of 64 and one of 37.  The SNR is chosen from the restatements alone
(layered_minsum and layered_sumproduct_exact with layered_ref.host_phi, 25 iterations): at SNR dB both latch some frames of
either tile and fail others, with exit iterations on both sides of 3; test_streamed_state.py asserts it."""
import numpy as np

import layered_q_cases as Q
from layered_q_ref import quantize
from layered_ref import host_phi, layered_minsum, layered_sumproduct_exact
from streamed_q_ref import decode_int_sparse, edges_of

TAILS_DEGREES = list(range(1, 18)) + [21, 22, 29, 30, 33, 40]
FRAMES = 101
SNR = 2.0
MS_SCALE = 0.75
ALGOS = ("minsum", "bp")
T = 64


def tails_23x120(seed=7):
    """23 checks, one of each degree of TAILS_DEGREES in an order drawn from the seed, on 120 variables.  As
    layered_wide_cases.ragged_60x400: check r first takes the lowest-numbered variables no check has used yet, at most 8 of them
    (so every variable is used: min(D, 8) sums to 156 > 120), then random others."""
    rng = np.random.default_rng(seed)
    m, n = len(TAILS_DEGREES), 120
    degs = [TAILS_DEGREES[i] for i in rng.permutation(m)]
    Hm = np.zeros((m, n), dtype=np.uint8)
    fresh = 0
    for r, D in enumerate(degs):
        take = min(D, n - fresh, 8)
        v = list(range(fresh, fresh + take))
        fresh += take
        pool = np.setdiff1d(np.arange(n), v)
        v += list(rng.choice(pool, D - take, replace=False))
        Hm[r, v] = 1
    assert fresh == n
    return Hm


_Hm = tails_23x120()
_Hm.setflags(write=False)
_deg = _Hm.sum(axis=1)
assert sorted(int(d) for d in _deg) == TAILS_DEGREES
assert {int(d) % 8 for d in _deg if d > 8} == set(range(8)), "a short last chunk of every length 1 ... 7, and none"
assert {(int(d) // 8, int(d) % 8) for d in _deg if d > 8} >= {(k, t) for k in (1, 2, 3) for t in (5, 6)}
assert (_Hm.sum(axis=0) > 0).all() and (_Hm.sum(axis=0) >= 2).mean() > 0.75


def matrix():
    return _Hm


class Tails:
    """the graph behind the library's analysis, its sets, symbols, channel values per quantiser, and the restatements' answers
    with their final state: ref() -> (bits, ok, iters, P [F, n], R [F, E]), R in processing order"""

    def __init__(self, A):
        self.Hm = _Hm
        self.H = A.ParityCheckMatrix(self.Hm)
        self.Z, self.layers = self.H.layers_any()
        self.frames, self.n, self.snr = FRAMES, self.Hm.shape[1], SNR
        self.y = A.transmit_frames(np.zeros((FRAMES, self.n), dtype=np.uint8), SNR)
        self.y.setflags(write=False)
        self.edges = edges_of(self.Hm)
        # the checks in processing order, and the variable of every edge in that order
        self.order = [int(c) for layer in self.layers for c in layer[layer >= 0]]
        self.edge_var = np.concatenate([self.edges[c] for c in self.order])
        self.E = len(self.edge_var)
        self._ref, self._chan, self._qref = {}, {}, {}

    def ref(self, algo, it, phi=None, phi_name="device", f32=False, y=None, key=None):
        """phi: the map handed to layered_sumproduct_exact (None: host_phi).  y: other symbols of the same shape rules (then key
        names them in the cache)"""
        if phi is None:
            phi, phi_name = host_phi, "host"
        k = (algo, it, f32, key) + ((phi_name,) if algo == "bp" else ())
        if k not in self._ref:
            y = self.y if y is None else y
            y = y.astype(np.float32) if f32 else y
            P, R = [], []
            if algo == "minsum":
                r = layered_minsum(self.Hm, self.layers, y, self.snr, it, MS_SCALE, symbols_f32=f32, posteriors=P, messages=R)
            else:
                r = layered_sumproduct_exact(self.Hm, self.layers, y, self.snr, it, phi, symbols_f32=f32, posteriors=P, messages=R)
            r = tuple(r) + (P[0], R[0])
            assert r[3].shape == (len(y), self.n) and r[4].shape == (len(y), self.E) and r[3].dtype == r[4].dtype == np.float32
            for a in r:
                a.setflags(write=False)
            self._ref[k] = r
        return self._ref[k]

    def channel(self, qname="default"):
        if qname not in self._chan:
            self._chan[qname] = quantize(self.y, self.snr, Q.QUANTS[qname]).astype(np.int16)
            self._chan[qname].setflags(write=False)
        return self._chan[qname]

    def qref(self, qname, it):
        """decode_int_sparse -> (bits, ok, iters, post [F, n] int16, R [F, E] int8)"""
        k = (qname, it)
        if k not in self._qref:
            R = []
            r = decode_int_sparse(self.edges, self.n, self.layers, self.channel(qname), it, Q.QUANTS[qname], messages=R)
            r = tuple(r) + (R[0],)
            assert r[4].shape == (self.frames, self.E)
            for a in r:
                a.setflags(write=False)
            self._qref[k] = r
        return self._qref[k]


_made = {}


def tails(A):
    if "tails" not in _made:
        _made["tails"] = Tails(A)
    return _made["tails"]


def decoder(A, algo, it, ee=True):
    """the streamed float layered decoder of `algo`"""
    if algo == "minsum":
        return A.StreamedLayeredMinSumDecoder(it, MS_SCALE, early_exit=ee)
    return A.StreamedLayeredBPDecoder(it, early_exit=ee)


def exits(ref, ref_next, it):
    """of the restatement's answers with max_iter = it and with max_iter = it + 1 -> three [F] bool arrays: the frames that latched
    before round `it`, those that ran out of iterations and passed the final syndrome pass, those that failed.  (A frame that
    latches in round `it` itself also reports ok = 1 and iters = it; it belongs to none of the three.  With one more round allowed
    it still reports it, while one that only passed the syndrome pass goes on and reports it + 1.)"""
    ok, iters = ref[1], ref[2]
    return (ok == 1) & (iters < it), (ok == 1) & (iters == it) & (ref_next[2] == it + 1), ok == 0
