"""The phi memo of the absorbed check passes (BpPass::phi_c / check_abs in the SAT instances that fixed-work decoders use)
changes no result: every decode and Monte-Carlo counter of the fused kernels is equal with the memo on and with
ACG_BP_NO_PHIMEMO=1 (the switch is read when a decoder handle is created, so each side runs in a fresh process).  H05 is the
code with absorbed passes; H and optimalH have none and run the same instances with the memo idle.  Run with `-m gpu` on an
MI355X."""
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
for name, snrs, lanes in (("H05", (-3.0, -2.0, 2.0), (16, 32, 64)), ("H", (1.0,), (32,)), ("optimalH", (-2.0,), (32,))):
    H = A.ParityCheckMatrix(o.read_pcm(os.path.join(sys.argv[1], "data", name + ".txt")))
    G, ok = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 64, 4244)
    for snr in snrs:
        y = A.transmit_frames(cws[np.arange(3000) % len(cws)], snr)
        for L in lanes:
            dec = A.BeliefPropagationDecoder(50, early_exit=False, lanes_per_frame=L)
            b, k, it = dec.decode_batch(H, y, snr)
            np.savez(os.path.join(sys.argv[2], "%s_%g_%d.npz" % (name, snr, L)), b=b, k=k, it=it)
        dec = A.BeliefPropagationDecoder(50, early_exit=False, lanes_per_frame=32)
        r = A.run_experiment(dec, cws, H, snr, frames=20000, noise="device", seed=13)
        out["%s_%g" % (name, snr)] = [int(x) for x in r.as_vector()]  # the seven counters
json.dump(out, open(os.path.join(sys.argv[2], "mc.json"), "w"))
"""


def run_side(tmp, no_memo):
    d = tmp / ("off" if no_memo else "on")
    d.mkdir()
    env = dict(os.environ)
    env.pop("ACG_BP_NO_PHIMEMO", None)
    env.pop("ACG_BP_NO_SATSKIP", None)
    if no_memo:
        env["ACG_BP_NO_PHIMEMO"] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(d)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return d


def test_phimemo_changes_no_result(tmp_path):
    on, off = run_side(tmp_path, False), run_side(tmp_path, True)
    files = sorted(f for f in os.listdir(off) if f.endswith(".npz"))
    assert len(files) == 3 * 3 + 1 + 1
    for f in files:
        a, b = np.load(on / f), np.load(off / f)
        for key in ("b", "k", "it"):
            assert np.array_equal(a[key], b[key]), (f, key)
    mon, moff = json.load(open(on / "mc.json")), json.load(open(off / "mc.json"))
    assert len(mon) == 3 + 1 + 1 and all(len(v) == 7 for v in mon.values())
    assert mon == moff
