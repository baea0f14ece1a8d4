"""What the tests of the streamed fixed-point layered min-sum engine share (tests/test_streamed_q_ref.py on the CPU,
tests/test_streamed_q_gpu.py on the device): the codes no other engine of the library takes, their channel values, and the
answers of tests/streamed_q_ref.py on them, computed once each.

  deg48   regular_ldpc(12, 192, 3, 48, seed=3): a check of 48 variables — six full chunks of 8 edges
  deg40   regular_ldpc(30, 400, 3, 40, seed=3): a check of 40 variables, several checks per set
  big     regular_ldpc(2050, 41000, 2, 40, seed=1): 164 000 bytes of state per frame, more than the LDS of a CU

The all-zero word is sent.  At these SNRs the restatement with the default quantiser decodes some frames and fails others; the
tests assert it on their own frames."""
import os
import subprocess

import numpy as np

import layered_q_cases as Q
from layered_q_ref import quantize
from streamed_q_ref import decode_int_sparse, edges_of

# name -> ((m, n, dv, dc, seed), SNR in dB, iterations, frames)
WIDE = {
    "deg48": ((12, 192, 3, 48, 3), 4.0, 10, 200),
    "deg40": ((30, 400, 3, 40, 3), 4.0, 10, 200),
    "big": ((2050, 41000, 2, 40, 1), 5.3, 8, 32),
}


class Wide:
    def __init__(self, A, name):
        shape, self.snr, self.iters, self.frames = WIDE[name]
        self.name = name
        Hm = A.regular_ldpc(*shape[:4], seed=shape[4])
        self.m, self.n = Hm.shape
        self.edges = edges_of(Hm)
        self.H = A.ParityCheckMatrix(Hm)
        self.Z, self.layers = self.H.layers_any()
        self.y = A.transmit_frames(np.zeros((self.frames, self.n), dtype=np.uint8), self.snr)
        self._chan, self._ref = {}, {}

    def channel(self, qname="default"):
        if qname not in self._chan:
            self._chan[qname] = quantize(self.y, self.snr, Q.QUANTS[qname]).astype(np.int16)
            self._chan[qname].setflags(write=False)
        return self._chan[qname]

    def ref(self, qname="default", it=None):
        it = self.iters if it is None else it
        k = (qname, it)
        if k not in self._ref:
            self._ref[k] = decode_int_sparse(self.edges, self.n, self.layers, self.channel(qname), it, Q.QUANTS[qname])
            for a in self._ref[k]:
                a.setflags(write=False)
        return self._ref[k]


_made = {}


def wide(A, name):
    if name not in _made:
        _made[name] = Wide(A, name)
    return _made[name]


def build_cxx_check(tmp_path):
    """tests/cxx_streamed_q_check.cpp compiled and linked as layered_q_cases.build_cxx_check builds its program -> the executable"""
    exe = str(tmp_path / "cxx_streamed_q_check")
    libdir = os.path.join(Q.ROOT, "acg_alp_ldpc_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(Q.ROOT, "include"),
                           os.path.join(Q.ROOT, "tests", "cxx_streamed_q_check.cpp"), "-o", exe, "-L" + libdir,
                           "-lacg_ldpc_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe
