"""What the tests of the LLR entrance of the streamed float layered engine share (tests/test_streamed_layered_io.py on the CPU,
tests/test_streamed_layered_io_gpu.py on the device): the codes of tests/streamed_layered_cases.py, their LLRs in three forms,
and the answers of tests/streamed_layered_io_ref.py on them, computed once per (case, form, algorithm, iterations, phi).

  plain      the fp32 channel LLRs of the case's symbols travelling as float32: layered_ref.channel_llr_f32(y, snr, True)
  special    those with NaN, +-inf, +-3e38, +0 and -0 written over 1 ... 7 positions of every frame; frame 0 all NaN (every LLR
             +0), frame 1 all -inf (every LLR -2^20: the all-ones word, which an even check degree accepts)
  punctured  those with PUNCTURED positions set to 0 and SHORTENED ones to +2^20 (the all-zero word is sent: a known 0)

At these SNRs the restatement decodes some frames of every form and fails others — on the CPU with layered_ref.host_phi
(tests/test_streamed_layered_io.py asserts it), on the device with its own phi (the GPU tests do)."""
import os
import subprocess

import numpy as np

import streamed_layered_cases as SL
from layered_ref import channel_llr_f32, host_phi
from streamed_layered_io_ref import LLR_CLAMP, decode_llr

ROOT = SL.ROOT
FORMS = ("plain", "special", "punctured")
SPECIAL = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 0.0, -0.0], dtype=np.float32)
# positions of a frame of deg40 (n = 400, check degree 40, rate 0.925) that carry no channel value / a known one.  PUNCTURED was
# chosen on the CPU: with 1 / 2 / 4 / 6 / 8 of them the restatement (host_phi) decodes 146 / 132 / 121 / 104 / 86 (min-sum) and 145 /
# 136 / 121 / 102 / 83 (sum-product) of the 200 frames at 4 dB, so 6 leaves about as many decoded as failed.
PUNCTURED = 6
SHORTENED = 16

_llr, _ref = {}, {}


class H05:
    """data/H05.txt (check degree <= 8: the one-pass step), 300 random codewords at -2 dB, 25 iterations, with the members of
    streamed_layered_cases.WideF that llr() and ref() read"""
    name, iters, frames = "H05", 25, 300

    def __init__(self, A):
        self.H = A.read_pcm(os.path.join(ROOT, "data", "H05.txt"))
        self.Hm = np.array(self.H.dense())
        self.Hm.setflags(write=False)
        self.n = self.Hm.shape[1]
        self.Z, self.layers = self.H.layers_any()
        G = A.read_pcm(os.path.join(ROOT, "data", "G05.txt")).dense()
        self._y = A.transmit_frames(A.gen_random_codewords(G, self.frames, 239239239), -2.0)
        self._y.setflags(write=False)

    def snr(self, algo):
        return -2.0

    def y(self, algo):
        return self._y


_cases = {}


def case(A, name):
    """H05, or one of streamed_layered_cases.wide: deg48, deg40, big"""
    if name != "H05":
        return SL.wide(A, name)
    if name not in _cases:
        _cases[name] = H05(A)
    return _cases[name]


def positions(n):
    """(punctured, shortened): disjoint positions of a frame of n values"""
    perm = np.random.default_rng(40).permutation(n)
    return np.sort(perm[:PUNCTURED]), np.sort(perm[PUNCTURED:PUNCTURED + SHORTENED])


def llr(c, algo, form="plain"):
    """[frames, n] float32 LLRs of the case c (streamed_layered_cases.WideF) in the given form, read-only"""
    k = (c.name, algo, form)
    if k not in _llr:
        L = channel_llr_f32(c.y(algo).astype(np.float32), c.snr(algo), True).copy()
        assert L.dtype == np.float32 and np.abs(L).max() < LLR_CLAMP
        if form == "special":
            rng = np.random.default_rng(7)
            for f in range(len(L)):
                cnt = 1 + f % 7
                L[f, rng.choice(c.n, cnt, replace=False)] = rng.choice(SPECIAL, cnt)
            L[0, :] = np.nan
            L[1, :] = -np.inf
        elif form == "punctured":
            punctured, shortened = positions(c.n)
            L[:, punctured] = 0.0
            L[:, shortened] = LLR_CLAMP
        else:
            assert form == "plain"
        L.setflags(write=False)
        _llr[k] = L
    return _llr[k]


def ref(c, algo, form="plain", it=None, phi=None, phi_name="device"):
    """(bits, ok, iters, post) of the restatement on llr(c, algo, form), read-only;
    phi: the map handed to layered_sumproduct_exact (None: host_phi)"""
    it = c.iters if it is None else it
    if phi is None:
        phi, phi_name = host_phi, "host"
    k = (c.name, algo, form, it) + (() if algo == "minsum" else (phi_name,))
    if k not in _ref:
        r = decode_llr(c.Hm, c.layers, llr(c, algo, form), it, algo, SL.MS_SCALE, phi)
        for a in r:
            a.setflags(write=False)
        _ref[k] = r
    return _ref[k]


def build_cxx_check(tmp_path):
    """tests/cxx_streamed_layered_io_check.cpp compiled with plain g++ against include/ and linked to the library -> the executable"""
    exe = str(tmp_path / "cxx_streamed_layered_io_check")
    libdir = os.path.join(ROOT, "acg_alp_ldpc_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx_streamed_layered_io_check.cpp"), "-o", exe, "-L" + libdir,
                           "-lacg_ldpc_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe
