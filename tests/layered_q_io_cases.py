"""What the tests of the integer entrance of the fixed-point layered min-sum engine share (tests/test_layered_q_io.py on the CPU,
tests/test_layered_q_io_gpu.py on the device): the channel values of the cases of tests/layered_q_cases.py — the restatement's
quantiser on each case's symbols — and the answers of tests/layered_q_io_ref.py on them, computed once each."""
import os

import numpy as np

import layered_q_cases as Q
from layered_q_io_ref import decode_int
from layered_q_ref import quantize

ROOT = Q.ROOT
# the cases on which a latched frame's posteriors go on moving when it is swept further (diag10 reaches a fixed point)
MOVING = ("H", "H05", "ragged", "qc4x24z27", "qc2x10z300")

_chan, _ref = {}, {}


def channel(A, name, qname):
    """int16 [frames, n]: layered_q_ref.quantize on the case's double symbols"""
    k = (name, qname)
    if k not in _chan:
        c = Q.case(A, name)
        _chan[k] = quantize(c.y, c.snr, Q.QUANTS[qname]).astype(np.int16)
        _chan[k].setflags(write=False)
    return _chan[k]


def ref(A, name, qname, it=None, keep_sweeping=False):
    """decode_int on channel(name, qname) -> bits, ok, iters, post (read-only)"""
    c = Q.case(A, name)
    it = c.iters if it is None else it
    k = (name, qname, it, keep_sweeping)
    if k not in _ref:
        _ref[k] = decode_int(c.Hm, c.layers, channel(A, name, qname), it, Q.QUANTS[qname], keep_sweeping=keep_sweeping)
        for a in _ref[k]:
            a.setflags(write=False)
    return _ref[k]


def disjoint4(checks=6000):
    """`checks` checks of degree 4 on disjoint variables (n = 4 * checks), built like diag10: ONE set of `checks` checks.  6000:
    48 008 + 24 000 + 3 000 bytes of LDS, above the 64 KiB a kernel gets without asking; six passes at L = 1024."""
    Hm = np.zeros((checks, 4 * checks), dtype=np.uint8)
    Hm[np.repeat(np.arange(checks), 4), np.arange(4 * checks)] = 1
    return Hm


def build_cxx_io_check(tmp_path):
    """tests/cxx_quant_io_check.cpp compiled and linked as layered_q_cases.build_cxx_check builds its program -> the executable"""
    import subprocess
    exe = str(tmp_path / "cxx_quant_io_check")
    libdir = os.path.join(ROOT, "acg_alp_ldpc_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx_quant_io_check.cpp"), "-o", exe, "-L" + libdir,
                           "-lacg_ldpc_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe
