#!/usr/bin/env python3
"""frames/s, kernel ms, FER and mean iterations of the workgroup-per-frame layered engine (bp_layered_block_kernel, 25 iterations)
next to the flooding engines (50 sweeps) on the code it exists for: BASELINE configs[4], the (3,6)-regular 5000 x 10000, at the
+2 dB of the README's configs[4] row, device-resident batch, fixed work and early exit.

    python3 tools/layered_block_rate.py                      every leg
    ACG_LDPC_LIB=<library of the parent commit> python3 tools/layered_block_rate.py --legs flooding
                                                             the flooding legs of another build of the library (A/B: the
                                                             flooding figures of this build are the cross-check that they
                                                             did not move; tools/ab_variant.sh builds variants)
A library older than the Python package lacks the entry points added since: they are left unbound here."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", choices=("all", "flooding", "layered"), default="all")
    ap.add_argument("--mode", choices=("both", "fixed", "exit"), default="both", help="fixed work, early exit, or both")
    ap.add_argument("--frames", type=int, default=32768)
    ap.add_argument("--snr", type=float, default=2.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime per process, see _lib.lib)
    from acg_alp_ldpc_amd import _lib
    probe = ctypes.CDLL(_lib.LIB_PATH)
    for name in [s for s in _lib.SYMBOLS if not hasattr(probe, s)]:
        print("library %s has no %s: left unbound" % (_lib.LIB_PATH, name))
        del _lib.SYMBOLS[name]
    import acg_alp_ldpc_amd as A
    import bench
    print("library: %s" % _lib.LIB_PATH)
    rig = bench.Rig(type("a", (), dict(inproc=0, gpus=1))())
    H, cws = bench.load_c5(A)
    batch = bench.Batch(rig, H, cws, args.frames)
    LAY = A.SCHEDULE_LAYERED
    legs = []
    for mode, ee in (("fixed", False), ("exit ", True)):
        if args.mode != "both" and args.mode != mode.strip():
            continue
        if args.legs in ("all", "flooding"):
            legs += [("flooding min-sum 50 fp32        %s" % mode, lambda dev, ee=ee: A.MinSumDecoder(50, 0.75, early_exit=ee, device=dev)),
                     ("flooding min-sum 50 f16 pairs   %s" % mode, lambda dev, ee=ee: A.MinSumDecoder(50, 0.75, early_exit=ee, device=dev, precision=A.PREC_F16)),
                     ("flooding sum-product 50         %s" % mode, lambda dev, ee=ee: A.BeliefPropagationDecoder(50, early_exit=ee, device=dev))]
        if args.legs in ("all", "layered"):
            for L in (512, 1024):
                legs += [("layered min-sum 25 fp32 L=%-4d  %s" % (L, mode),
                          lambda dev, ee=ee, L=L: A.MinSumDecoder(25, 0.75, early_exit=ee, device=dev, schedule=LAY, lanes_per_frame=L)),
                         ("layered min-sum 25 fp16 L=%-4d  %s" % (L, mode),
                          lambda dev, ee=ee, L=L: A.MinSumDecoder(25, 0.75, early_exit=ee, device=dev, schedule=LAY, lanes_per_frame=L, precision=A.PREC_F16)),
                         ("layered sum-product 25 L=%-4d   %s" % (L, mode),
                          lambda dev, ee=ee, L=L: A.BeliefPropagationDecoder(25, early_exit=ee, device=dev, schedule=LAY, lanes_per_frame=L))]
    for tag, ctor in legs:
        r = bench.decode_leg(rig, batch, ctor, args.snr, args.steps, args.warmup)
        print("5000x10000 %+.1f dB  %s  %8.3f M frames/s  kernel %8.2f ms  FER %.5f  mean iters %5.2f  [%s]"
              % (args.snr, tag, r["value"] / 1e6, r["kernel_ms"], r["fer"], r["mean_iters"], r["instance"]), flush=True)


if __name__ == "__main__":
    main()
