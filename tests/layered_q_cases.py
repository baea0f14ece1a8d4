"""The codes, frames and quantisers the tests of the fixed-point layered min-sum engine share (tests/test_layered_q.py on the CPU,
tests/test_layered_q_gpu.py on the device): the smallest codes that reach every path of bp_layered_q_kernel.

  H          data/H.txt, 64 x 128, check degree 8, first-fit colouring; random codewords
  H05        data/H05.txt, quasi-cyclic Z = 20, check degrees 4-7, degree-1 variables; random codewords from data/G05.txt
  ragged     layered_wide_cases: degrees 3 ... 19, one and several chunks of 8 edges in one code
  qc4x24z27  layered_wide_cases: degree 22-23, sets smaller than a wavefront
  qc2x10z300 layered_wide_cases: sets of 300 checks — two passes at L = 256 (five at L = 64), a partly filled one at 512
  diag10     ten checks of degree 1, 2, 9, 12, 16, 17, 24, 25, 31, 32 on disjoint variables: the degree cap, the one-variable
             rule (m2 = Rmax) and both sides of every chunk boundary

The all-zero word is sent where no generator is at hand.  The SNRs are those at which the restatement (layered_q_ref) with the
default quantiser decodes some frames and fails others; test_layered_q.py asserts it for every case."""
import os

import numpy as np

import layered_wide_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data")

QUANTS = {
    "default": (0.5, 6, 6, 8, 1, 0, 1),
    "scaled": (0.5, 6, 6, 8, 3, 2, 0),          # normalised 3/4, no offset
    "saturating": (1.0, 4, 4, 4, 1, 0, 0),      # posteriors clip constantly
}

DIAG_DEGREES = [1, 2, 9, 12, 16, 17, 24, 25, 31, 32]

# name -> (SNR in dB, iterations, frames)
CASES = {
    "H": (0.0, 20, 300),
    "H05": (-2.0, 15, 400),
    "ragged": (3.0, 25, 300),
    "qc4x24z27": (2.5, 25, 300),
    "qc2x10z300": (3.0, 25, 300),
    "diag10": (3.0, 5, 400),
}


def diag10():
    n = sum(DIAG_DEGREES)
    Hm = np.zeros((len(DIAG_DEGREES), n), dtype=np.uint8)
    first = np.concatenate([[0], np.cumsum(DIAG_DEGREES)])
    for c, D in enumerate(DIAG_DEGREES):
        Hm[c, first[c]:first[c] + D] = 1
    return Hm


class Case:
    """matrix, sets of layers_wide(), sent words and noisy symbols of one case; the restatement's answers, computed once each"""

    def __init__(self, A, name):
        from layered_q_ref import layered_minsum_q
        self._ref_fn = layered_minsum_q
        self.name = name
        self.snr, self.iters, self.frames = CASES[name]
        cws = None
        if name == "H":
            self.H = A.read_pcm(os.path.join(DATA, "H.txt"))
            G, ok = self.H.get_orthogonal()
            assert ok
            cws = A.gen_random_codewords(G, self.frames, 4245)
        elif name == "H05":
            self.H = A.read_pcm(os.path.join(DATA, "H05.txt"))
            G = A.read_pcm(os.path.join(DATA, "G05.txt")).dense()
            cws = A.gen_random_codewords(G, self.frames, 239239239)
        elif name == "diag10":
            self.H = A.ParityCheckMatrix(diag10())
        else:
            self.H = A.ParityCheckMatrix(np.array(W.matrix(name)))
        self.Hm = np.array(self.H.dense())
        self.n = self.Hm.shape[1]
        self.Z, self.layers = self.H.layers_wide()
        self.width = max(int((l >= 0).sum()) for l in self.layers)
        self.cws = np.zeros((self.frames, self.n), dtype=np.uint8) if cws is None else cws
        if cws is not None:
            assert not (self.cws @ self.Hm.T.astype(np.int64) % 2).any() and self.cws.any(axis=1).mean() > 0.9
        self.y = A.transmit_frames(self.cws, self.snr)
        self._ref = {}

    def ref(self, quant, it=None, symbols_f32=False):
        it = self.iters if it is None else it
        k = (quant, it, symbols_f32)
        if k not in self._ref:
            y = self.y.astype(np.float32) if symbols_f32 else self.y
            self._ref[k] = self._ref_fn(self.Hm, self.layers, y, self.snr, it, QUANTS[quant], symbols_f32=symbols_f32)
        return self._ref[k]


_made = {}


def case(A, name):
    if name not in _made:
        _made[name] = Case(A, name)
    return _made[name]


def build_cxx_check(tmp_path):
    """tests/cxx_quant_check.cpp compiled and linked as tests/test_cxx_adaptor.py builds its program -> the executable"""
    import subprocess
    exe = str(tmp_path / "cxx_quant_check")
    libdir = os.path.join(ROOT, "acg_alp_ldpc_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx_quant_check.cpp"), "-o", exe, "-L" + libdir,
                           "-lacg_ldpc_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe
