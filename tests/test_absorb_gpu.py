"""Absorbed degree-1 variables (BpPass::check_abs) change no result: every decode and Monte-Carlo counter of the fused
sum-product kernels is equal with absorption on and with ACG_BP_NO_ABSORB=1 (the switch is read when a decoder handle is
created, so each side runs in a fresh process).  Run with `-m gpu` on an MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

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
    cws = A.gen_random_codewords(G, 64, 4242)
    for snr in (-2.0, 0.0, 2.0):
        y = A.transmit_frames(cws[np.arange(3000) % len(cws)], snr)
        for L in (16, 32, 64):
            for ee in (False, True):
                dec = A.BeliefPropagationDecoder(50, early_exit=ee, lanes_per_frame=L)
                b, k, it = dec.decode_batch(H, y, snr)
                np.savez(os.path.join(sys.argv[2], "%s_%g_%d_%d.npz" % (name, snr, L, ee)), b=b, k=k, it=it)
        for ee in (False, True):
            dec = A.BeliefPropagationDecoder(50, early_exit=ee, lanes_per_frame=32)
            r = A.run_experiment(dec, cws, H, snr, frames=20000, noise="device", seed=11)
            out["%s_%g_%d" % (name, snr, ee)] = [int(x) for x in r.as_vector()]  # the seven counters
json.dump(out, open(os.path.join(sys.argv[2], "mc.json"), "w"))
"""


def run_side(tmp, no_absorb):
    d = tmp / ("off" if no_absorb else "on")
    d.mkdir()
    env = dict(os.environ)
    env.pop("ACG_BP_NO_ABSORB", None)
    if no_absorb:
        env["ACG_BP_NO_ABSORB"] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(d)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return d


def test_absorption_changes_no_result(tmp_path):
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
