#!/usr/bin/env python3
"""points x frames / s of a quantiser grid on the fixed-point layered min-sum engine: ONE acg_ldpc_mc_run_quants call
(run_experiment_quants) against the loop that call replaces — one acg_ldpc_decoder_create_quantized + acg_ldpc_mc_run + destroy
per point (QuantizedMinSumDecoder + run_experiment + close).  Device noise, 64 points, 25 iterations, fixed work.

  c5         BASELINE configs[4], the (3,6)-regular 5000 x 10000, +2 dB, L = 512
  qc6x32z64  the (6,32)-regular quasi-cyclic 384 x 2048 of tests/layered_wide_cases.py, +2.5 dB, L = 0

Two shapes per code: 1 000 frames per point (a format search: the loop's launches under-fill the chip) and 32 768 (they do not).
Both legs include creating and closing their handles — the grid leg one, the loop 64.  One warm-up round, then the legs alternate
`--runs` times (default 3); the counters of the two legs must be equal point for point, the tool checks it before it prints.
Reported: points x frames / s of every run of both legs, the ratio slowest grid over fastest loop, and the decode kernel's
frames / s inside the grid call (points x frames over the sum of the points' kernel_ms; for the 64 points, whose FER differ, and
for 64 copies of the default quantiser) next to the leg of tools/layered_q_rate.py for the same code (the symbol entrance's own
instance with the default quantiser on a resident batch of 32 768 frames), timed here in the same session.

    python3 tools/quant_grid_rate.py                 both codes, both shapes
    python3 tools/quant_grid_rate.py --code c5 --frames 1000"""
import argparse
import itertools
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# 2^6 valid quantisers: step x channel bits x message bits x posterior bits x (scale_num, scale_shift) x offset
POINTS = [(st, ch, ms, po, num, sh, of) for st, ch, ms, po, (num, sh), of in
          itertools.product((0.5, 0.25), (5, 6), (5, 6), (8, 9), ((1, 0), (3, 2)), (0, 1))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--code", choices=("both", "c5", "qc6x32z64"), default="both")
    ap.add_argument("--frames", type=int, nargs="*", default=[1000, 32768], help="frames per point")
    ap.add_argument("--points", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3, help="steps of the resident-batch leg")
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401  (first: one HIP runtime per process, see _lib.lib)
    import acg_alp_ldpc_amd as A
    import bench
    import layered_wide_cases as W
    rig = bench.Rig(type("a", (), dict(inproc=0, gpus=1))())
    dev = rig.devs[0].idx
    points = POINTS[:args.points]
    fields = A.ExperimentResult.FIELDS

    def make(L, quant=None):
        return A.QuantizedMinSumDecoder(25, quant=None if quant is None else A.QuantConfig(*quant), early_exit=False, device=dev, lanes_per_frame=L)

    def grid_leg(H, cws, snr, L, F, points=points):
        t0 = time.perf_counter()
        dec = make(L)
        try:
            res = A.run_experiment_quants(dec, cws, H, snr, points, frames=F, noise="device", seed=1)
        finally:
            dec.close()
        return time.perf_counter() - t0, res

    def loop_leg(H, cws, snr, L, F):
        t0 = time.perf_counter()
        res = []
        for q in points:
            dec = make(L, q)
            try:
                res.append(A.run_experiment(dec, cws, H, snr, frames=F, noise="device", seed=1))
            finally:
                dec.close()
        return time.perf_counter() - t0, res

    def run(name, snr, H, cws, L):
        batch = bench.Batch(rig, H, cws, 32768)
        base = [bench.decode_leg(rig, batch, lambda d: A.QuantizedMinSumDecoder(25, early_exit=False, device=d, lanes_per_frame=L), snr, args.steps,
                                 args.warmup) for _ in range(args.runs)]
        del batch
        print("%s %+.1f dB fixed  resident batch of 32768 frames (tools/layered_q_rate.py's leg)  %s M frames/s  kernel %s ms per step"
              % (name, snr, " / ".join("%7.3f" % (x["value"] / 1e6) for x in base), " / ".join("%8.2f" % x["kernel_ms"] for x in base)), flush=True)
        for F in args.frames:
            work = len(points) * F
            grid_leg(H, cws, snr, L, F)
            loop_leg(H, cws, snr, L, F)
            tg, tl, kern = [], [], []
            for _ in range(args.runs):
                dt, rg = grid_leg(H, cws, snr, L, F)
                tg.append(dt)
                kern.append(work / (sum(r.kernel_ms for r in rg) * 1e-3))
                dt, rl = loop_leg(H, cws, snr, L, F)
                tl.append(dt)
                for k, (a, b) in enumerate(zip(rg, rl)):
                    if any(getattr(a, f) != getattr(b, f) for f in fields):
                        raise SystemExit("%s: point %d %r: the grid call and the loop count differently: %r / %r" % (name, k, points[k], a, b))
            fer = [r.FER() for r in rg]
            # like for like with the resident-batch leg: the same call with the default quantiser at every point
            same = [A.QuantConfig().as_tuple()] * len(points)
            kern_same = [work / (sum(r.kernel_ms for r in grid_leg(H, cws, snr, L, F, same)[1]) * 1e-3) for _ in range(args.runs)]
            print("%s %+.1f dB fixed  %d points x %d frames  grid %s M frames/s  loop %s M frames/s  slowest grid / fastest loop %.2fx  "
                  "decode kernel inside the grid call %s M frames/s, with the default quantiser at every point %s M frames/s  FER %.4f ... %.4f"
                  % (name, snr, len(points), F, " / ".join("%7.3f" % (work / t / 1e6) for t in tg), " / ".join("%7.3f" % (work / t / 1e6) for t in tl),
                     min(tl) / max(tg), " / ".join("%7.3f" % (k / 1e6) for k in kern), " / ".join("%7.3f" % (k / 1e6) for k in kern_same), min(fer), max(fer)), flush=True)

    if args.code in ("both", "c5"):
        H, cws = bench.load_c5(A)
        run("5000x10000", 2.0, H, cws, 512)
    if args.code in ("both", "qc6x32z64"):
        Hm = np.array(W.matrix("qc6x32z64"))
        run("384x2048", 2.5, A.ParityCheckMatrix(Hm), np.zeros((1, Hm.shape[1]), dtype=np.uint8), 0)


if __name__ == "__main__":
    main()
