"""The phi fast path of the fused sum-product sweeps (BpPass::phi_c / phi_v, the SAT instances that fixed-work decoders
use) changes no result: every decode and Monte-Carlo counter of the fused kernels is equal with the fast path on and with
ACG_BP_NO_SATSKIP=1 (the switch is read when a decoder handle is created, so each side runs in a fresh process; early-exit
decoders run the plain instances on both sides), and at the boundaries of the two constant regions the fast path returns
the bits of the full evaluation.  Run with `-m gpu` on an MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import acg_alp_ldpc_amd as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import acg_alp_ldpc_amd as A
from oracle.pyoracle import Oracle
out = {}
o = Oracle()
for name in ("H05", "optimalH"):
    H = A.ParityCheckMatrix(o.read_pcm(os.path.join(sys.argv[1], "data", name + ".txt")))
    G, ok = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 64, 4243)
    for snr in (-2.0, 0.0, 2.0):
        y = A.transmit_frames(cws[np.arange(3000) % len(cws)], snr)
        for L in (16, 32, 64):
            for ee in (False, True):
                dec = A.BeliefPropagationDecoder(50, early_exit=ee, lanes_per_frame=L)
                b, k, it = dec.decode_batch(H, y, snr)
                np.savez(os.path.join(sys.argv[2], "%s_%g_%d_%d.npz" % (name, snr, L, ee)), b=b, k=k, it=it)
        for ee in (False, True):
            dec = A.BeliefPropagationDecoder(50, early_exit=ee, lanes_per_frame=32)
            r = A.run_experiment(dec, cws, H, snr, frames=20000, noise="device", seed=12)
            out["%s_%g_%d" % (name, snr, ee)] = [int(x) for x in r.as_vector()]  # the seven counters
json.dump(out, open(os.path.join(sys.argv[2], "mc.json"), "w"))
"""


def run_side(tmp, no_skip):
    d = tmp / ("off" if no_skip else "on")
    d.mkdir()
    env = dict(os.environ)
    env.pop("ACG_BP_NO_SATSKIP", None)
    if no_skip:
        env["ACG_BP_NO_SATSKIP"] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(d)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return d


def test_satskip_changes_no_result(tmp_path):
    on, off = run_side(tmp_path, False), run_side(tmp_path, True)
    files = sorted(f for f in os.listdir(off) if f.endswith(".npz"))
    assert len(files) == 2 * 3 * 3 * 2
    for f in files:
        a, b = np.load(on / f), np.load(off / f)
        for key in ("b", "k", "it"):
            assert np.array_equal(a[key], b[key]), (f, key)
    mon, moff = json.load(open(on / "mc.json")), json.load(open(off / "mc.json"))
    assert len(mon) == 2 * 3 * 2 and all(len(v) == 7 for v in mon.values())
    assert mon == moff


def test_phi_fast_path_boundaries():
    # scaled-domain inputs: the saturation point 66 and its neighbours, +inf, NaN, +0 / -0, the smallest denormal (a message
    # word of magnitude 0 with the hard-decision LSB set, read as a number), the smallest normal, and a spread of ordinary values
    bits = np.array([0x00000000, 0x80000000, 0x00000001, 0x00000003, 0x007FFFFF, 0x00800000, 0x7F800000, 0x7FC00000,
                     0x7F800001, 0xFFC00000], dtype=np.uint32)
    special = np.concatenate([bits.view(np.float32),
                              np.array([66.0, np.nextafter(np.float32(66), np.float32(0)), np.nextafter(np.float32(66), np.float32(1e9)),
                                        65.0, 67.0, 1e30, 1e-30, 1.0, 1.4426950408889634, 1e-3], dtype=np.float32)])
    rng = np.random.default_rng(5)
    x = np.concatenate([special, rng.uniform(0, 80, 4000).astype(np.float32),
                        np.exp(rng.uniform(-40, 4.5, 4000)).astype(np.float32)]).astype(np.float32)
    out = np.zeros(3 * len(x), dtype=np.uint32)
    assert A.lib().acg_ldpc_debug_phi_sat(x.ctypes.data, out.ctypes.data, len(x)) == 0
    full, chk, var = out[0::3], out[1::3], out[2::3]
    ax = np.abs(x)
    full_abs = np.zeros(len(x), dtype=np.uint32)
    assert A.lib().acg_ldpc_debug_phi_sat(ax.ctypes.data, out.ctypes.data, len(x)) == 0
    full_abs = out[0::3]
    # check side: every input a sweep can hand it (sums of non-negative magnitudes, NaN included) gives the full bits
    nonneg = ~np.signbit(x)
    assert np.array_equal(chk[nonneg], full[nonneg])
    # variable side (on |x|): the full bits everywhere
    assert np.array_equal(var, full_abs)
    # the constants themselves: phi(+0) = +inf, phi(x >= 66) = +0, and NaN stays NaN on both sides
    assert chk[0] == 0x7F800000 and full[0] == 0x7F800000
    sat = ~np.isnan(ax) & (ax >= 66)
    assert sat.sum() >= 5 and np.all(var[sat] == 0)
    below = np.nextafter(np.float32(66), np.float32(0))
    assert var[np.flatnonzero(x == below)[0]] != 0
    nan = np.isnan(x)
    assert np.all(np.isnan(var[nan].view(np.float32))) and np.all(np.isnan(chk[nan & nonneg].view(np.float32)))
