#!/usr/bin/env python3
"""What a two-stage decoder (acg_ldpc_cascade_*) costs and buys: H05, a device-resident batch of 2^20 frames of float symbols
(acg_ldpc_awgn_dev, codewords of data/G05.txt), the device entry points, -2 dB and -1 dB, for the pairs

    MS+BP       min-sum(0.75) 10 sweeps -> BP-50
    BP+QP-ADMM  BP-50 -> QP-ADMM(1.2, 0.55, 1000 sweeps)

Legs, alternating, `--runs` rounds (default 3) in one session, each `--steps` timed calls behind one warm-up call, timed by the
host clock around calls that end in a device synchronise (the cascade waits on the host once per chunk, so its wall time is the
figure): the first decoder alone, the second alone, the cascade, and the second alone on a resident compact batch of exactly the K
frames the first fails.  glue = cascade - first alone - second on K.  FER of first, second and cascade come from the Monte-Carlo
calls on the same frames (same seed and first_frame, device noise).

Bytes model of the glue per chunk of F frames (n symbols of elem bytes, nwords = (n+31)/32, K frames handed on):
    select   F in, 4K + 4 out (+ F when stage is asked for)
    gather   2 * K * n * elem
    scatter  2 * K * (4 * nwords + 5) (+ K for stage)
The kernels' own times come from a kernel trace of `--glue-only` (a few cascade calls and nothing else):
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python3 tools/cascade_rate.py --glue-only
whose *kernel_stats.csv lists cascade_select_kernel, cascade_gather_kernel and cascade_scatter_kernel.

    python3 tools/cascade_rate.py [--frames N] [--pairs MS+BP,BP+QP-ADMM] [--snrs -2,-1]"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DATA = os.path.join(ROOT, "data")
CHUNK = 65536


def glue_bytes(F, K_per_chunk, n, elem, stage):
    """bytes the three glue kernels move for chunks with K_per_chunk[c] failed frames -> (select, gather, scatter)"""
    nw = (n + 31) // 32
    sel = gat = sca = 0
    for c, K in enumerate(K_per_chunk):
        fc = min(CHUNK, F - c * CHUNK)
        sel += fc + 4 * K + 4 + (fc if stage else 0)
        if K:
            gat += 2 * K * n * elem
            sca += 2 * K * (4 * nw + 5) + (K if stage else 0)
    return sel, gat, sca


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--pairs", default="MS+BP,BP+QP-ADMM")
    ap.add_argument("--snrs", default="-2,-1")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--glue-only", action="store_true")
    args = ap.parse_args()
    import torch
    import acg_alp_ldpc_amd as A
    from acg_alp_ldpc_amd import _lib
    from acg_alp_ldpc_amd._lib import check, lib
    if not A.device_available():
        raise SystemExit("cascade_rate.py measures on a GPU: no HIP device here, nothing measured")
    H = A.read_pcm(os.path.join(DATA, "H05.txt"))
    G = A.read_pcm(os.path.join(DATA, "G05.txt")).dense()
    cws = A.gen_random_codewords(G, 8192, 239239239)
    F, n, nw = args.frames, H.n, (H.n + 31) // 32
    make = {"MS+BP": (lambda: A.MinSumDecoder(10, 0.75), lambda: A.BeliefPropagationDecoder(50)),
            "BP+QP-ADMM": (lambda: A.BeliefPropagationDecoder(50), lambda: A.QPADMMDecoder(1.2, 0.55, 1000))}
    y = torch.empty((F, n), dtype=torch.float32, device="cuda")
    bits = torch.empty((F, nw), dtype=torch.int32, device="cuda")
    ok = torch.empty(F, dtype=torch.uint8, device="cuda")
    its = torch.empty(F, dtype=torch.int32, device="cuda")
    stage = torch.empty(F, dtype=torch.uint8, device="cuda")
    outs = (bits.data_ptr(), ok.data_ptr(), its.data_ptr())

    def timed(step, steps):
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    for snr in [float(s) for s in args.snrs.split(",")]:
        for pair in args.pairs.split(","):
            d1, d2 = (f() for f in make[pair])
            cas = A.CascadeDecoder(*(f() for f in make[pair]))
            cfg = _lib.McCfg()
            cfg.frames, cfg.first_frame, cfg.snr, cfg.seed, cfg.noise = F, 0, snr, args.seed, _lib.NOISE_DEVICE_PHILOX
            cfg.codewords, cfg.n_codewords = cws.ctypes.data, cws.shape[0]
            check(lib().acg_ldpc_awgn_dev(d1.handle(H)[0], C.byref(cfg), y.data_ptr(), None))
            d1.sync(H)
            cas.decode_batch_dev(H, y.data_ptr(), False, F, snr, *outs, stage.data_ptr())
            torch.cuda.synchronize()
            K = cas.last_call(H)[0]
            Kc = [int((stage[c:c + CHUNK] == 2).sum()) for c in range(0, F, CHUNK)]
            assert sum(Kc) == K
            model = glue_bytes(F, Kc, n, 4, True)
            if args.glue_only:
                for _ in range(4):
                    cas.decode_batch_dev(H, y.data_ptr(), False, F, snr, *outs, stage.data_ptr())
                torch.cuda.synchronize()
                print("%s %+.1f dB: 5 cascade calls of %d frames, K = %d each; model bytes per call select %d gather %d scatter %d"
                      % (pair, snr, F, K, *model), flush=True)
                for d in (d1, d2, cas):
                    d.close()
                continue
            yK = y[torch.nonzero(stage == 2).flatten()].contiguous()
            assert yK.shape[0] == K
            legs = [("first alone", F, lambda: d1.decode_batch_dev(H, y.data_ptr(), False, F, snr, *outs)),
                    ("second alone", F, lambda: d2.decode_batch_dev(H, y.data_ptr(), False, F, snr, *outs)),
                    ("cascade", F, lambda: cas.decode_batch_dev(H, y.data_ptr(), False, F, snr, *outs, stage.data_ptr())),
                    ("second on K", K, lambda: d2.decode_batch_dev(H, yK.data_ptr(), False, K, snr, *outs))]
            t = {tag: [] for tag, _, _ in legs}
            for _ in range(args.runs):
                for tag, _, step in legs:
                    t[tag].append(timed(step, args.steps))
            print("%s %+.1f dB, %d frames, K = %d (%.2f %%)" % (pair, snr, F, K, 100.0 * K / F))
            for tag, frames, _ in legs:
                print("    %-13s %s ms   %s M frames/s" % (tag, " / ".join("%8.3f" % (1e3 * v) for v in t[tag]),
                                                          " / ".join("%7.2f" % (frames / v / 1e6) for v in t[tag])))
            glue = [c - a - b for c, a, b in zip(t["cascade"], t["first alone"], t["second on K"])]
            print("    glue = cascade - first alone - second on K: %s ms; model bytes select %d gather %d scatter %d (%d chunks)"
                  % (" / ".join("%7.3f" % (1e3 * g) for g in glue), *model, len(Kc)))
            print("    cascade against second alone: x %s" % " / ".join("%.2f" % (b / c) for c, b in zip(t["cascade"], t["second alone"])))
            total, first, ex = A.run_experiment_cascade(cas, cws, H, snr, frames=F, noise="device", seed=args.seed)
            r2 = A.run_experiment(d2, cws, H, snr, frames=F, noise="device", seed=args.seed)
            assert ex["second_frames"] == K
            print("    FER first %.6f  second %.6f  cascade %.6f   (Monte-Carlo call: first %.2f ms + second %.2f ms of decode kernels)"
                  % (first.FER(), r2.FER(), total.FER(), first.kernel_ms, ex["second_kernel_ms"]), flush=True)
            for d in (d1, d2, cas):
                d.close()


if __name__ == "__main__":
    main()
