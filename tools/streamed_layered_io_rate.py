#!/usr/bin/env python3
"""frames/s and kernel ms of the LLR entrance of the streamed float layered engine (acg_ldpc_decode_batch_llr_dev: fp32 LLRs in,
with and without fp32 posteriors out) next to the symbol entrance (acg_ldpc_decode_batch_dev, float symbols) on the SAME handle,
the same frames and in the same session: 25 iterations, fixed work, device-resident batch, sum-product and min-sum(0.75).

  c5     BASELINE configs[4], the (3,6)-regular 5000 x 10000, +2 dB, 196 608 frames
  big    regular_ldpc(2050, 41000, 2, 40, seed=1), 5.3 dB, 131 072 frames

The LLRs are the ones the symbol entrance forms from the batch's float symbols, (float) ((double) y * (2 / sigma^2)), so the three
legs decode the same frames and must return the same words, flags and iterations: the tool checks that, and that the posteriors'
sign bits are the words of the ok frames, before it prints.  The legs alternate, `--runs` rounds (default 3), each timing `--steps`
steps behind `--warmup` warm-up steps.  The handle is made before the LLRs and posteriors are allocated, so its workspace is the
one tools/streamed_layered_rate.py measures.

    python3 tools/streamed_layered_io_rate.py                    both codes, both algorithms
    python3 tools/streamed_layered_io_rate.py --legs symbols     the symbol leg alone: with ACG_LDPC_LIB naming the library of a
                                                                 commit without the LLR entrance, the A/B of that leg"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NEW_SYMBOLS = ("acg_ldpc_decode_batch_llr_dev", "acg_ldpc_decode_batch_llr")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--code", choices=("both", "c5", "big"), default="both")
    ap.add_argument("--algos", default="bp,minsum")
    ap.add_argument("--legs", choices=("all", "symbols"), default="all")
    ap.add_argument("--frames", type=int, default=196608)
    ap.add_argument("--big-frames", type=int, default=131072)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import numpy as np
    import torch
    import acg_alp_ldpc_amd as A
    if args.legs == "symbols":
        for name in NEW_SYMBOLS:          # (a library without the entrance can be loaded: nothing below calls it)
            A._lib.SYMBOLS.pop(name, None)
    import bench
    rig = bench.Rig(type("a", (), dict(inproc=0, gpus=1))())
    d0 = rig.devs[0]
    s = d0.shard
    ITERS, SCALE = 25, 0.75

    def run(name, snr, H, cws, F):
        n = H.n
        batch = bench.Batch(rig, H, cws, F)
        outs = (batch.bits[s].data_ptr(), batch.ok[s].data_ptr(), batch.its[s].data_ptr())
        dev = batch.y[s].device
        for k, algo in enumerate(args.algos.split(",")):
            # (one decoder at a time: a workspace is sized by the memory that is free when its handle is made)
            if algo == "bp":
                dec = A.StreamedLayeredBPDecoder(ITERS, early_exit=False, device=d0.idx)
            else:
                dec = A.StreamedLayeredMinSumDecoder(ITERS, SCALE, early_exit=False, device=d0.idx)
            dec.handle(H)
            if k == 0:
                batch.gen_noise({s: dec}, snr, 1)
                rig.sync_local()
            y = batch.y[s]
            legs = [("symbols (float32)", lambda d: dec.decode_batch_dev(H, y.data_ptr(), False, F, snr, *outs, d.stream.cuda_stream))]
            llr = post = None
            if args.legs == "all":
                # (allocated behind the handle and released with it: every handle sees the free memory the symbol leg alone would)
                llr = torch.empty((F, n), dtype=torch.float32, device=dev)
                post = torch.empty((F, n), dtype=torch.float32, device=dev)
                inv_var2 = 2.0 / (10.0 ** (-(snr / 10.0)) / 2.0)
                for f0 in range(0, F, 8192):     # (in pieces: the double intermediate of the whole batch is 8 bytes per symbol)
                    llr[f0:f0 + 8192] = (y[f0:f0 + 8192].double() * inv_var2).float()
                torch.cuda.synchronize()
                legs.append(("LLRs", lambda d: dec.decode_llr_batch_dev(H, llr.data_ptr(), F, *outs, None, d.stream.cuda_stream)))
                legs.append(("LLRs + posteriors", lambda d: dec.decode_llr_batch_dev(H, llr.data_ptr(), F, *outs, post.data_ptr(), d.stream.cuda_stream)))
            res = {tag: [] for tag, _ in legs}
            first = None
            for _ in range(args.runs):
                for tag, step_fn in legs:
                    dt, kms, _info = rig.timed(step_fn, args.steps, args.warmup)
                    res[tag].append((F * args.steps / dt, kms))
                    got = (batch.bits[s].clone(), batch.ok[s].clone(), batch.its[s].clone())
                    if first is None:
                        first = got
                    elif not all(bool((a == b).all()) for a, b in zip(got, first)):
                        raise SystemExit("%s %s: the leg '%s' returns other words, flags or iterations than the symbol entrance" % (name, algo, tag))
            if args.legs == "all":
                K = min(F, 2048)                                                 # (the sign check: on the first frames)
                ok = batch.ok[s][:K] == 1
                words = torch.signbit(post[:K])[ok].to(torch.int32)
                bits = ((batch.bits[s][:K][ok][:, :, None] >> torch.arange(32, device=dev, dtype=torch.int32)) & 1).reshape(int(ok.sum()), -1)[:, :n]
                if not bool((words == bits).all()):
                    raise SystemExit("%s %s: signbit(post) is not the word of every ok frame" % (name, algo))
            q = batch.quality(F)
            desc = dec.describe(H)
            for tag, _ in legs:
                print("%s %+.1f dB %d frames fixed %-6s %-18s  %s k frames/s  kernel %s ms  FER %.5f  [%s]"
                      % (name, snr, F, algo, tag, " / ".join("%7.1f" % (v / 1e3) for v, _ in res[tag]), " / ".join("%8.2f" % k for _, k in res[tag]),
                         q["fer"], desc), flush=True)
            dec.close()
            del llr, post
            torch.cuda.empty_cache()
        del batch
        torch.cuda.empty_cache()

    if args.code in ("both", "c5"):
        H, cws = bench.load_c5(A)
        run("5000x10000", 2.0, H, cws, args.frames)
    if args.code in ("both", "big"):
        Hm = A.regular_ldpc(2050, 41000, 2, 40, seed=1)
        run("2050x41000", 5.3, A.ParityCheckMatrix(Hm), np.zeros((1, 41000), dtype=np.uint8), args.big_frames)


if __name__ == "__main__":
    main()
