#!/usr/bin/env python3
"""Check-matrix local search rate: proposals/s of tools/drivers/bin/acg_optimize_h at the reference's settings
(optimize_H.cpp: 1000 frames at -3 dB, alpha 1.95, mu 0.5, at most 1000 sweeps, host noise) for several --batch sizes.

    python tools/optimize_h_rate.py [--exe tools/drivers/bin/acg_optimize_h] [--batches 1,4,16,64] [--proposals 1000]
                                    [--runs 3] [--label new] [--out profiles/x.json]

A driver built from another commit is measured the same way: --exe <that binary> --batches 1 (with ACG_LDPC_LIB /
LD_LIBRARY_PATH naming that commit's library, see tools/ab_variant.sh).  Prints min-max proposals/s over the runs (proposals over the wall time of the whole process) and the
driver's own summary line: proposals scored, speculated proposals discarded, host / device seconds of the search.
"""
import argparse, json, os, re, subprocess, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--exe", default=os.path.join(ROOT, "tools", "drivers", "bin", "acg_optimize_h"))
ap.add_argument("--batches", default="1,4,16,64")
ap.add_argument("--proposals", type=int, default=1000)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--label", default="new")
ap.add_argument("--no-batch-flag", action="store_true", help="a driver from before --batch existed")
ap.add_argument("--out")
a = ap.parse_args()

rows = []
for K in [int(x) for x in a.batches.split(",")]:
    rates, notes, stdouts, accepts = [], [], set(), []
    for _ in range(a.runs):
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [a.exe, "--random", "8,14", "--Z", "20", "--tests", "1000", "--snr", "-3", "--alpha", "1.95", "--mu", "0.5",
                   "--admm-iters", "1000", "--noise", "host", "--iters", str(a.proposals), "--out", os.path.join(tmp, "H.txt")]
            if not a.no_batch_flag:
                cmd += ["--batch", str(K)]
            t0 = time.time()
            p = subprocess.run(cmd, capture_output=True, text=True)
            wall = time.time() - t0
        if p.returncode != 0:
            sys.exit("driver failed: " + p.stderr[-400:])
        m = re.search(r"\[acg_optimize_h\] (.*)", p.stderr)
        d = dict(kv.split("=") for kv in m.group(1).split()) if m else {}
        # wall time of the whole process for every driver, old or new: start, HIP initialisation and the initial FER included
        sec = wall
        rates.append(a.proposals / sec)
        notes.append(d)
        stdouts.add(p.stdout)
        accepts.append(p.stdout.count("accept"))
    row = dict(label=a.label, batch=K, proposals=a.proposals, proposals_per_s=[round(r, 2) for r in rates], summary=notes[-1],
               stdout_identical_across_runs=len(stdouts) == 1, accepts=accepts)
    rows.append(row)
    s = notes[-1]
    print("%-8s batch %3d: %7.2f - %7.2f proposals/s over %d runs; scored %s discarded %s host %s s device %s s of %s s search; accepts %s"
          % (a.label, K, min(rates), max(rates), a.runs, s.get("scored", "?"), s.get("discarded", "?"), s.get("host_s", "?"),
             s.get("device_s", "?"), s.get("search_s", "?"), accepts), flush=True)
if a.out:
    json.dump(rows, open(a.out, "w"), indent=1)
