"""The code, the frames and the failure patterns of the cascade hand-over tests (tests/test_cascade_shapes.py on the CPU,
tests/test_cascade_shapes_gpu.py on the device): the shapes at which cascade_select_kernel walks more than one tile of 1024
flags, cascade_gather_kernel takes one of its three element-wide instances and the gather and scatter grids stride.

  H05m1   data/H05.txt without its last column, 160 x 279 of rank 160, no longer quasi-cyclic.  Rows of 279 elements are
          1116 bytes as float32 (12 mod 16), 2232 as float64 (8 mod 16) and 558 as int16 posteriors (14 mod 16): never a multiple
          of 16, so cascade_gather_launch cannot take uint4.  NCW random codewords from the generator of get_orthogonal();
          global frame g carries word g mod NCW, as everywhere in the Monte-Carlo code.

WHICH frames the first stage fails is designed, not left to the noise: for a boolean mask fail[F], a frame with fail false is
its clean codeword (y = 1 - 2 cw: a one-iteration layered min-sum passes it with iters = 1) and a frame with fail true is its
codeword through transmit_frames at -2 dB (one iteration never decodes it; 20 iterations decode most, each to its own word).
test_cascade_shapes.py asserts both halves with the restatement tests/layered_ref.py::layered_minsum for every mask that has a
CPU expectation.  The masks put the failures where a tile of the select scan begins and ends."""
import os

import numpy as np

from layered_ref import layered_minsum
from mc_decode_path import sent_words
from mc_detail_ref import pack_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data")

SNR = -2.0
SCALE = 0.75
ITERS = (1, 20)       # stage 0, stage 1: MinSumDecoder(it, SCALE, schedule=SCHEDULE_LAYERED)
NCW = 1021            # codewords; a prime, so no tile, wavefront or chunk size divides the period
TILE = 1024           # SELECT_THREADS of cascade_kernels.hip


class Code:
    """H05m1: matrix, handle, the library's own layering (what bp_layered_kernel walks) and NCW codewords"""

    def __init__(self, A):
        full = A.read_pcm(os.path.join(DATA, "H05.txt")).dense()
        self.Hm = np.ascontiguousarray(full[:, :-1])
        self.H = A.ParityCheckMatrix(self.Hm)
        self.m, self.n = self.Hm.shape
        G, ok = self.H.get_orthogonal()
        assert ok and G.shape == (self.n - self.m, self.n)
        self.cws = A.gen_random_codewords(G, NCW, 4245)
        assert not (self.cws @ self.Hm.T.astype(np.int64) % 2).any() and self.cws.any(axis=1).mean() > 0.9
        self.G, self.Z, self.layers = self.H.layers()


_code = []


def code(A):
    if not _code:
        _code.append(Code(A))
    return _code[0]


def gf2_rank(M):
    M = (np.asarray(M) != 0).astype(np.uint8).copy()
    r = 0
    for c in range(M.shape[1]):
        p = np.flatnonzero(M[r:, c])
        if not len(p):
            continue
        M[[r, r + p[0]]] = M[[r + p[0], r]]
        rows = np.flatnonzero(M[:, c])
        rows = rows[rows != r]
        M[rows] ^= M[r]
        r += 1
        if r == M.shape[0]:
            break
    return r


# ------------------------------------------------------------------------------------------------------- the masks
def bernoulli(F, p, seed, also=()):
    m = np.random.default_rng(seed).random(F) < p
    m[list(also)] = True
    return m


def tile_masks():
    """five chunks of two tiles, each with its own pattern -> fail [5 * 2048]"""
    m = np.zeros((5, 2 * TILE), dtype=bool)
    m[0, TILE - 1] = True                      # only the last lane of tile 0
    m[1, [TILE, 2 * TILE - 1]] = True          # only the first and the last lane of tile 1
    m[2, TILE:] = True                         # tile 0 clean, tile 1 all failed: base = 0 into a full tile
    m[3, 0::64] = m[3, 63::64] = True          # lanes 0 and 63 of every wavefront
    m[4] = bernoulli(2 * TILE, 0.5, 20261)
    return m.reshape(-1)


def odd_mask():
    """2051 frames for chunks of 1025: every chunk ends one frame into its second tile"""
    return bernoulli(2051, 0.3, 20262, also=(1024, 1025, 2050))


# name -> (mask, first global frame of the noise: the seed of the pattern's noisy frames); these two have a CPU expectation
def masks():
    return {"tiles": (tile_masks(), 1 << 20), "odd": (odd_mask(), 2 << 20)}


def base_mask():
    """1100 frames of H05 (n = 280): more than one tile, rows that ARE multiples of 16 bytes"""
    return bernoulli(1100, 0.3, 20263), 3 << 20


def cap_mask():
    """one frame more than the chunk cap of 65536: about 13 000 failures and the lone frame of the second chunk"""
    return bernoulli(65537, 0.2, 20264, also=(65536,)), 4 << 20


def q_mask():
    """1100 frames for the fixed-point first stage"""
    return bernoulli(1100, 0.3, 20265), 5 << 20


# ------------------------------------------------------------------------------------------------------ the frames
def sent(c, F, first):
    return sent_words(c.cws, c.n, first, F)


def symbols(A, c, fail, first, dtype=np.float64):
    """y [F, n]: frame f carries word (first + f) mod NCW; clean where fail is false, at SNR through the host generator (global
    frame first + f) where it is true"""
    fail = np.asarray(fail, dtype=bool)
    F = len(fail)
    y = 1.0 - 2.0 * sent(c, F, first).astype(np.float64)
    if fail.any():
        y[fail] = A.transmit_frames(c.cws, SNR, first, F)[fail]
    return np.ascontiguousarray(y.astype(dtype))


class Restated:
    """the cascade of the two restatements on y: stage 0 on all frames, stage 1 on flatnonzero(ok == 0), merged
    -> .out = (packed words, ok, iters, stage), .ok0 = stage 0's flags, .ok1 = stage 1's flags on the failed frames"""

    def __init__(self, c, y, snr=SNR, iters=ITERS):
        f32 = y.dtype == np.float32
        bits, ok, it = layered_minsum(c.Hm, c.layers, y, snr, iters[0], SCALE, symbols_f32=f32)
        self.bits0, self.ok0, self.it0 = bits.copy(), ok.copy(), it.copy()
        stage = np.ones(len(ok), dtype=np.uint8)
        failed = np.flatnonzero(ok == 0)
        self.ok1 = np.zeros(0, dtype=np.uint8)
        if len(failed):
            b1, self.ok1, it1 = layered_minsum(c.Hm, c.layers, np.ascontiguousarray(y[failed]), snr, iters[1], SCALE, symbols_f32=f32)
            bits[failed], ok[failed], it[failed], stage[failed] = b1, self.ok1, it1, 2
        self.bits = bits
        self.out = (pack_bits(bits), ok, it, stage)


_restated = {}


def restated(A, name, dtype=np.float64):
    """the named mask's frames and their restated cascade, computed once -> (fail, y, Restated)"""
    k = (name, np.dtype(dtype).name)
    if k not in _restated:
        c = code(A)
        fail, first = masks()[name]
        y = symbols(A, c, fail, first, dtype)
        _restated[k] = (fail, y, Restated(c, y))
    return _restated[k]
