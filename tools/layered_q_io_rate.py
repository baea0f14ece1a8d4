#!/usr/bin/env python3
"""frames/s and kernel ms of the INTEGER entrance of the fixed-point layered min-sum engine (acg_ldpc_decode_batch_q_dev: int16
channel values in, with and without int16 posteriors out) next to the symbol entrance (acg_ldpc_decode_batch_dev, float symbols)
on the SAME handle, the same frames and in the same session: 25 iterations, fixed work, device-resident batch of 32 768 frames.

  c5         BASELINE configs[4], the (3,6)-regular 5000 x 10000, +2 dB, L = 512
  qc6x32z64  the (6,32)-regular quasi-cyclic 384 x 2048 of tests/layered_wide_cases.py, +2.5 dB, L = 0

The channel values are acg_ldpc_quantize_dev of the batch's symbols, so the three legs decode the same frames and must return the
same words, flags and iterations: the tool checks that before it prints.  The legs alternate, `--runs` rounds (default 3), each
timing `--steps` steps behind `--warmup` warm-up steps.

    python3 tools/layered_q_io_rate.py                 both codes
    python3 tools/layered_q_io_rate.py --code c5       one of them"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--code", choices=("both", "c5", "qc6x32z64"), default="both")
    ap.add_argument("--frames", type=int, default=32768)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import numpy as np
    import torch
    import acg_alp_ldpc_amd as A
    import bench
    import layered_wide_cases as W
    rig = bench.Rig(type("a", (), dict(inproc=0, gpus=1))())
    d0 = rig.devs[0]

    def run(name, snr, H, cws, L):
        F = args.frames
        batch = bench.Batch(rig, H, cws, F)
        dec = A.QuantizedMinSumDecoder(25, early_exit=False, device=d0.idx, lanes_per_frame=L)
        batch.gen_noise({d0.shard: dec}, snr, 1)
        s = d0.shard
        dev = batch.y[s].device
        c = torch.empty((F, batch.n), dtype=torch.int16, device=dev)
        post = torch.empty((F, batch.n), dtype=torch.int16, device=dev)
        dec.quantize_dev(H, batch.y[s].data_ptr(), False, F * batch.n, snr, c.data_ptr(), d0.stream.cuda_stream)
        rig.sync_local()
        outs = (batch.bits[s].data_ptr(), batch.ok[s].data_ptr(), batch.its[s].data_ptr())
        legs = [("symbols (float32)", lambda d: dec.decode_batch_dev(H, batch.y[s].data_ptr(), False, F, snr, *outs, d.stream.cuda_stream)),
                ("channel values", lambda d: dec.decode_llr_batch_dev(H, c.data_ptr(), F, *outs, None, d.stream.cuda_stream)),
                ("channel values + posteriors", lambda d: dec.decode_llr_batch_dev(H, c.data_ptr(), F, *outs, post.data_ptr(), d.stream.cuda_stream))]
        res = {tag: [] for tag, _ in legs}
        first = None
        for _ in range(args.runs):
            for tag, step in legs:
                dt, kms, _info = rig.timed(step, args.steps, args.warmup)
                res[tag].append((F * args.steps / dt, kms))
                got = (batch.bits[s].clone(), batch.ok[s].clone(), batch.its[s].clone())
                if first is None:
                    first = got
                elif not all(bool((a == b).all()) for a, b in zip(got, first)):
                    raise SystemExit("%s: the leg '%s' returns other words, flags or iterations than the symbol entrance" % (name, tag))
        K = min(F, 2048)                                                     # (the sign check: on the first frames)
        ok = batch.ok[s][:K] == 1
        words = (post[:K] < 0)[ok].to(torch.int32)
        bits = ((batch.bits[s][:K][ok][:, :, None] >> torch.arange(32, device=dev, dtype=torch.int32)) & 1).reshape(int(ok.sum()), -1)[:, :batch.n]
        if not bool((words == bits).all()):
            raise SystemExit("%s: (post < 0) is not the word of every ok frame" % name)
        q = batch.quality(F)
        desc = dec.describe(H)
        for tag, _ in legs:
            print("%s %+.1f dB fixed  %-28s  %s M frames/s  kernel %s ms  FER %.5f  [%s]"
                  % (name, snr, tag, " / ".join("%7.3f" % (v / 1e6) for v, _ in res[tag]), " / ".join("%8.2f" % k for _, k in res[tag]), q["fer"], desc), flush=True)
        dec.close()
        del batch

    if args.code in ("both", "c5"):
        H, cws = bench.load_c5(A)
        run("5000x10000", 2.0, H, cws, 512)
    if args.code in ("both", "qc6x32z64"):
        Hm = np.array(W.matrix("qc6x32z64"))
        run("384x2048", 2.5, A.ParityCheckMatrix(Hm), np.zeros((1, Hm.shape[1]), dtype=np.uint8), 0)


if __name__ == "__main__":
    main()
