#!/usr/bin/env python3
"""frames/s, kernel ms, FER and mean iterations of the fixed-point layered min-sum engine (bp_layered_q_kernel, 25 iterations,
fixed work) next to the float layered engines and the flooding half-precision pairs, device-resident batch of 32 768 frames:

  c5         BASELINE configs[4], the (3,6)-regular 5000 x 10000, at the +2 dB of tools/layered_block_rate.py: the integer engine
             at L = 512 and L = 1024 against layered min-sum 25 with fp32 and fp16 messages (bp_layered_block_kernel, L = 512 and
             1024) and flooding min-sum 50 on half-precision pairs
  qc6x32z64  the (6,32)-regular quasi-cyclic 384 x 2048 of tests/layered_wide_cases.py at the +2.5 dB of
             tools/layered_wide_rate.py: the integer engine at L = 0 against layered min-sum 25 fp32 / fp16 (bp_layered_wide_kernel,
             L = 0)

Every leg is timed `--runs` times (default 3), each run `--steps` steps behind `--warmup` warm-up steps, all in one session.  The
float kernels are those of the parent commit: this engine adds a kernel file and touches none of theirs.

    python3 tools/layered_q_rate.py                 both codes
    python3 tools/layered_q_rate.py --code c5       one of them"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCALED = dict(scale_num=3, scale_shift=2, offset=0)      # normalised 3/4: the float legs' 0.75


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--code", choices=("both", "c5", "qc6x32z64"), default="both")
    ap.add_argument("--frames", type=int, default=32768)
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
    LAY = A.SCHEDULE_LAYERED

    def q_leg(L, quant):
        return lambda dev: A.QuantizedMinSumDecoder(25, quant=quant, early_exit=False, device=dev, lanes_per_frame=L)

    def f_leg(L, prec):
        return lambda dev: A.MinSumDecoder(25, 0.75, early_exit=False, device=dev, schedule=LAY, lanes_per_frame=L, precision=prec)

    def run(name, snr, H, cws, legs):
        batch = bench.Batch(rig, H, cws, args.frames)
        for tag, ctor in legs:
            runs = [bench.decode_leg(rig, batch, ctor, snr, args.steps, args.warmup) for _ in range(args.runs)]
            r = runs[-1]
            print("%s %+.1f dB fixed  %-44s  %s M frames/s  kernel %8.2f ms  FER %.5f  mean iters %5.2f  [%s]"
                  % (name, snr, tag, " / ".join("%7.3f" % (x["value"] / 1e6) for x in runs), r["kernel_ms"], r["fer"], r["mean_iters"],
                     r["instance"]), flush=True)
        del batch

    if args.code in ("both", "c5"):
        H, cws = bench.load_c5(A)
        legs = []
        for L in (512, 1024):
            legs += [("integer offset-1 (6, 6, 8 bits) L=%d" % L, q_leg(L, None)),
                     ("integer 3/4 (6, 6, 8 bits) L=%d" % L, q_leg(L, SCALED)),
                     ("layered min-sum 25 fp32 L=%d" % L, f_leg(L, A.PREC_DEFAULT)),
                     ("layered min-sum 25 fp16 L=%d" % L, f_leg(L, A.PREC_F16))]
        legs += [("flooding min-sum 50 f16 pairs", lambda dev: A.MinSumDecoder(50, 0.75, early_exit=False, device=dev, precision=A.PREC_F16))]
        run("5000x10000", 2.0, H, cws, legs)
    if args.code in ("both", "qc6x32z64"):
        Hm = np.array(W.matrix("qc6x32z64"))
        run("384x2048", 2.5, A.ParityCheckMatrix(Hm), np.zeros((1, Hm.shape[1]), dtype=np.uint8),
            [("integer offset-1 (6, 6, 8 bits) L=0", q_leg(0, None)), ("integer 3/4 (6, 6, 8 bits) L=0", q_leg(0, SCALED)),
             ("layered min-sum 25 fp32 L=0", f_leg(0, A.PREC_DEFAULT)), ("layered min-sum 25 fp16 L=0", f_leg(0, A.PREC_F16))])


if __name__ == "__main__":
    main()
