#!/usr/bin/env python3
"""What ordered-statistics decoding costs and buys as the second stage behind the fixed-point layered min-sum engine, whose
posteriors it takes over (acg_ldpc_cascade_*, handover=posteriors).  Device-resident batches of float symbols (acg_ldpc_awgn_dev),
the device entry points, for the points

    H05        2^20 frames at -2 dB and -1 dB (codewords of data/G05.txt)
    qc4x24z27  2^18 frames at 2.5 dB (tests/layered_wide_cases.py, 108 x 648, check degree 22-23; the all-zero word)

Legs, alternating, `--runs` rounds (default 3) in one session, each `--steps` timed calls behind one warm-up call, timed by the
host clock around calls that end in a device synchronise:

    OSD-1           alone, on the channel symbols
    QMS-25          alone (default quantiser)
    QMS-25+OSD-0    cascade, posteriors handed over
    QMS-25+OSD-1    cascade, posteriors handed over
    BP-50+QP-ADMM   the cascade BP-50 -> QP-ADMM(1.2, 0.55, 1000): the yardstick for speed (H05 only: the other code's checks are
                    too wide for these two engines)

For every leg: M frames/s of each run; then, from the Monte-Carlo calls on the same frames (same seed, device noise): FER, the
pseudo-codewords (undetected errors) among the frames, and for a cascade the frames handed over and the share of them repaired
(second_correct / second_frames).

    python3 tools/osd_rate.py [--points H05:-2,H05:-1,qc4x24z27:2.5] [--frames N] [--runs 3] [--steps 2]"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DATA = os.path.join(ROOT, "data")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="H05:-2,H05:-1,qc4x24z27:2.5")
    ap.add_argument("--frames", type=int, default=0, help="frames of every point (default: 2^20 for H05, 2^18 for qc4x24z27)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import torch
    import acg_alp_ldpc_amd as A
    from acg_alp_ldpc_amd import _lib
    from acg_alp_ldpc_amd._lib import check, lib
    if not A.device_available():
        raise SystemExit("osd_rate.py measures on a GPU: no HIP device here, nothing measured")

    def timed(step, steps):
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    for point in args.points.split(","):
        name, snr = point.split(":")
        snr = float(snr)
        if name == "H05":
            H = A.read_pcm(os.path.join(DATA, "H05.txt"))
            cws = A.gen_random_codewords(A.read_pcm(os.path.join(DATA, "G05.txt")).dense(), 8192, 239239239)
            F = args.frames or 1 << 20
        else:
            import layered_wide_cases as W
            H = A.ParityCheckMatrix(np.array(W.matrix(name)))
            cws = None
            F = args.frames or 1 << 18
        n, nw = H.n, (H.n + 31) // 32
        y = torch.empty((F, n), dtype=torch.float32, device="cuda")
        bits = torch.empty((F, nw), dtype=torch.int32, device="cuda")
        ok = torch.empty(F, dtype=torch.uint8, device="cuda")
        its = torch.empty(F, dtype=torch.int32, device="cuda")
        outs = (bits.data_ptr(), ok.data_ptr(), its.data_ptr())
        qms = lambda: A.QuantizedMinSumDecoder(25)
        made = [("OSD-1", A.OSDDecoder(1)), ("QMS-25", qms()),
                ("QMS-25+OSD-0", A.CascadeDecoder(qms(), A.OSDDecoder(0))), ("QMS-25+OSD-1", A.CascadeDecoder(qms(), A.OSDDecoder(1))),
                ("BP-50+QP-ADMM", A.CascadeDecoder(A.BeliefPropagationDecoder(50), A.QPADMMDecoder(1.2, 0.55, 1000)))]
        legs = []
        for tag, d in made:
            try:
                d.handle(H)
                legs.append((tag, d))
            except A.LdpcError as e:
                print("%s %+.1f dB: leg %s left out: %s" % (name, snr, tag, e))
                d.close()
        cfg = _lib.McCfg()
        cfg.frames, cfg.first_frame, cfg.snr, cfg.seed, cfg.noise = F, 0, snr, args.seed, _lib.NOISE_DEVICE_PHILOX
        if cws is not None:
            cfg.codewords, cfg.n_codewords = cws.ctypes.data, cws.shape[0]
        check(lib().acg_ldpc_awgn_dev(legs[0][1].handle(H)[0], C.byref(cfg), y.data_ptr(), None))
        legs[0][1].sync(H)
        t = {tag: [] for tag, _ in legs}
        for _ in range(args.runs):
            for tag, d in legs:
                t[tag].append(timed(lambda: d.decode_batch_dev(H, y.data_ptr(), False, F, snr, *outs), args.steps))
        print("%s (%d x %d) %+.1f dB, %d frames" % (name, H.m, n, snr, F))
        fps = {}
        for tag, d in legs:
            fps[tag] = [F / v for v in t[tag]]
            line = "    %-14s %s M frames/s" % (tag, " / ".join("%8.3f" % (v / 1e6) for v in fps[tag]))
            if isinstance(d, A.CascadeDecoder):
                total, first, ex = A.run_experiment_cascade(d, cws, H, snr, frames=F, noise="device", seed=args.seed)
                K = ex["second_frames"]
                line += "   FER %.6f (first alone %.6f)  pseudo %d (first %d)  handed over %d (%.2f %%)  repaired %d = %.1f %% of them" % (
                    total.FER(), first.FER(), total.pseudo, first.pseudo, K, 100.0 * K / F, ex["second_correct"],
                    100.0 * ex["second_correct"] / max(K, 1))
            else:
                r = A.run_experiment(d, cws, H, snr, frames=F, noise="device", seed=args.seed)
                line += "   FER %.6f  pseudo %d" % (r.FER(), r.pseudo)
            print(line, flush=True)
        if "BP-50+QP-ADMM" in fps:
            for tag in ("QMS-25+OSD-0", "QMS-25+OSD-1"):
                print("    %s against BP-50+QP-ADMM: x %s" % (tag, " / ".join("%.2f" % (a / b) for a, b in zip(fps[tag], fps["BP-50+QP-ADMM"]))))
        for _, d in legs:
            d.close()
        del y, bits, ok, its
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
