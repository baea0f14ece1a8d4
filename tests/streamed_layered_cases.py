"""What the tests of the streamed float layered engine share (tests/test_streamed_layered_cabi.py on the CPU,
tests/test_streamed_layered_gpu.py on the device): the codes of tests/streamed_q_cases.py no LDS engine takes — deg48, deg40,
big — their symbols, and the answers of tests/layered_ref.py (layered_minsum, layered_sumproduct_exact) on them over the sets
of ParityCheckMatrix.layers_any(), computed once per (algorithm, iterations, phi).

The all-zero word is sent.  At these SNRs both restatements decode some frames and fail others (on the CPU with
layered_ref.host_phi: test_streamed_layered_cabi.py asserts it; on the device with its own phi: the GPU tests do)."""
import os
import subprocess

import numpy as np

import streamed_q_cases as S
from layered_ref import host_phi, layered_minsum, layered_sumproduct_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS_SCALE = 0.75
ALGOS = ("minsum", "bp")

# SNR in dB per (case, algorithm) where it is not the one of streamed_q_cases.WIDE: within 5.0 ... 5.6 dB for `big`
SNR = {}


class WideF:
    """a case of streamed_q_cases.WIDE for the float engine: dense matrix, sets, symbols per algorithm, restatements"""

    def __init__(self, A, name):
        self.w = S.wide(A, name)
        self.name = name
        shape = S.WIDE[name][0]
        self.Hm = A.regular_ldpc(*shape[:4], seed=shape[4])
        self.Hm.setflags(write=False)
        self.H, self.layers, self.iters, self.frames, self.n = self.w.H, self.w.layers, self.w.iters, self.w.frames, self.w.n
        self._y, self._ref = {}, {}
        self._A = A

    def snr(self, algo):
        return SNR.get((self.name, algo), self.w.snr)

    def y(self, algo):
        snr = self.snr(algo)
        if snr == self.w.snr:
            return self.w.y
        if snr not in self._y:
            self._y[snr] = self._A.transmit_frames(np.zeros((self.frames, self.n), dtype=np.uint8), snr)
            self._y[snr].setflags(write=False)
        return self._y[snr]

    def ref(self, algo, phi=None, it=None, phi_name="device"):
        """(bits, ok, iters) of the restatement; phi: the map handed to layered_sumproduct_exact (None: host_phi)"""
        it = self.iters if it is None else it
        if phi is None:
            phi, phi_name = host_phi, "host"
        k = (algo, it) if algo == "minsum" else (algo, it, phi_name)
        if k not in self._ref:
            if algo == "minsum":
                r = layered_minsum(self.Hm, self.layers, self.y(algo), self.snr(algo), it, MS_SCALE)
            else:
                r = layered_sumproduct_exact(self.Hm, self.layers, self.y(algo), self.snr(algo), it, phi)
            for a in r:
                a.setflags(write=False)
            self._ref[k] = r
        return self._ref[k]


_made = {}


def wide(A, name):
    if name not in _made:
        _made[name] = WideF(A, name)
    return _made[name]


def decoder(A, algo, it, ee=True, **kw):
    """the streamed float layered decoder of `algo`"""
    if algo == "minsum":
        return A.StreamedLayeredMinSumDecoder(it, MS_SCALE, early_exit=ee, **kw)
    return A.StreamedLayeredBPDecoder(it, early_exit=ee, **kw)


def lds_decoder(A, algo, it, ee=True, L=256):
    """the workgroup-per-frame LDS layered decoder of `algo`"""
    kw = dict(schedule=A.SCHEDULE_LAYERED, early_exit=ee, lanes_per_frame=L)
    return A.MinSumDecoder(it, MS_SCALE, **kw) if algo == "minsum" else A.BeliefPropagationDecoder(it, **kw)


def build_cxx_check(tmp_path):
    """tests/cxx_streamed_layered_check.cpp compiled with plain g++ against include/ and linked to the library -> the executable"""
    exe = str(tmp_path / "cxx_streamed_layered_check")
    libdir = os.path.join(ROOT, "acg_alp_ldpc_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx_streamed_layered_check.cpp"), "-o", exe, "-L" + libdir,
                           "-lacg_ldpc_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe
