#!/usr/bin/env python3
"""frames/s, kernel ms, FER and mean iterations of the wide-check layered engine (bp_layered_wide_kernel, 25 iterations) next to
the flooding engine lanes_per_frame = 0 selects (50 sweeps, the same check rule) on the (6,32)-regular quasi-cyclic 384 x 2048
code of tests/layered_wide_cases.py (the 10GBASE-T shape: check degree 32, the engine's cap), at +2.5 dB, device-resident
batch, fixed work.  Every leg is timed `--runs` times (default 3), each run `--steps` steps behind `--warmup` warm-up steps; the
lines give every run, the summary the slowest layered run over the fastest flooding run of the same check rule.

    python3 tools/layered_wide_rate.py                      every leg
    python3 tools/layered_wide_rate.py --mode exit          early exit instead of fixed work"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", choices=("all", "flooding", "layered"), default="all")
    ap.add_argument("--mode", choices=("fixed", "exit"), default="fixed", help="fixed work or early exit")
    ap.add_argument("--frames", type=int, default=32768)
    ap.add_argument("--snr", type=float, default=2.5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401  (first: one HIP runtime per process, see _lib.lib)
    import acg_alp_ldpc_amd as A
    import bench
    import layered_wide_cases as W
    rig = bench.Rig(type("a", (), dict(inproc=0, gpus=1))())
    Hm = np.array(W.matrix("qc6x32z64"))
    H = A.ParityCheckMatrix(Hm)
    cws = np.zeros((1, Hm.shape[1]), dtype=np.uint8)
    batch = bench.Batch(rig, H, cws, args.frames)
    LAY = A.SCHEDULE_LAYERED
    ee = args.mode == "exit"
    legs = []
    if args.legs in ("all", "flooding"):
        legs += [("minsum", "flooding min-sum 50 fp32        ", lambda dev: A.MinSumDecoder(50, 0.75, early_exit=ee, device=dev)),
                 ("bp", "flooding sum-product 50 fp32    ", lambda dev: A.BeliefPropagationDecoder(50, early_exit=ee, device=dev))]
    if args.legs in ("all", "layered"):
        for L in (256, 512, 1024):
            for msg, prec in (("fp32", A.PREC_DEFAULT), ("fp16", A.PREC_F16)):
                legs += [("minsum", "layered min-sum 25 %s L=%-4d   " % (msg, L),
                          lambda dev, L=L, prec=prec: A.MinSumDecoder(25, 0.75, early_exit=ee, device=dev, schedule=LAY, lanes_per_frame=L, precision=prec)),
                         ("bp", "layered sum-product 25 %s L=%-4d" % (msg, L),
                          lambda dev, L=L, prec=prec: A.BeliefPropagationDecoder(25, early_exit=ee, device=dev, schedule=LAY, lanes_per_frame=L, precision=prec))]
    rates = {}
    for algo, tag, ctor in legs:
        runs = [bench.decode_leg(rig, batch, ctor, args.snr, args.steps, args.warmup) for _ in range(args.runs)]
        r = runs[-1]
        v = [x["value"] / 1e6 for x in runs]
        rates[(algo, tag.strip())] = v
        print("384x2048 %+.1f dB %s  %s  %s M frames/s  kernel %8.2f ms  FER %.5f  mean iters %5.2f  [%s]"
              % (args.snr, args.mode, tag, " / ".join("%7.3f" % x for x in v), r["kernel_ms"], r["fer"], r["mean_iters"], r["instance"]), flush=True)
    for algo in ("minsum", "bp"):
        flo = [v for (a, t), v in rates.items() if a == algo and t.startswith("flooding")]
        if not flo:
            continue
        for (a, t), v in rates.items():
            if a == algo and t.startswith("layered"):
                print("%-36s slowest run %7.3f / fastest flooding-50 run %7.3f = %.2f x" % (t, min(v), max(flo[0]), min(v) / max(flo[0])))


if __name__ == "__main__":
    main()
