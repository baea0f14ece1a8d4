#!/usr/bin/env python3
"""frames/s, kernel ms and achieved bytes/s of the streamed fixed-point layered min-sum engine
(acg_ldpc_decoder_create_quantized_streamed, bp_streamed_q_kernel) on device-resident inputs, the legs alternating in one
session, `--runs` rounds (default 3), each timing `--steps` steps behind `--warmup` warm-up steps.

  (a) c5     BASELINE configs[4], the (3,6)-regular 5000 x 10000, +2 dB, 25 iterations, fixed work, int16 channel values:
             the streamed engine against bp_layered_q_kernel at L = 512 on
             the same frames — the same algorithm, so words, flags and iterations are asserted equal — and against the float
             streamed min-sum (MinSumDecoder, engine = streamed, flooding) at 50 sweeps on the symbols those values came from.
  (a') c5    the two integer legs of (a) on channel values drawn uniformly from -20 ... 31: no frame latches, so every lane of
             the streamed engine stores in every iteration (the worst case of its traffic; the LDS engine's time does not
             depend on the data).
  (b) big    regular_ldpc(2050, 41000, 2, 40, seed=1), 5.3 dB, 25 iterations: rate and FER of the streamed engine, fixed work
             and early exit.  No other engine takes this code.

Bytes: the model of a frame is 6 E per iteration (P and R read, P and R written) + 4 n in (channel values read, P written) +
n read for the word + 4 ceil(n / 32) + 5 out; a check of more than 8 variables reads P and R twice, 9 E per iteration.  The model
is that of 25 full iterations for every leg: a lane whose frames have all latched writes nothing, and a tile with early exit
ends when its last frame latches, so the kernel moves fewer bytes than the model where frames latch.  The float streamed
engine's model is bench.bp_bytes_per_frame.

    python3 tools/streamed_q_rate.py                   both
    python3 tools/streamed_q_rate.py --code c5         one of them"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def model_bytes(n, E, iters, wide):
    return (9 if wide else 6) * E * iters + 4 * n + 2 * n + 4 * ((n + 31) // 32) + 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--code", choices=("both", "c5", "big"), default="both")
    ap.add_argument("--frames", type=int, default=196608)
    ap.add_argument("--big-frames", type=int, default=196608)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    import numpy as np
    import torch
    import acg_alp_ldpc_amd as A
    import bench
    rig = bench.Rig(type("a", (), dict(inproc=0, gpus=1))())
    d0 = rig.devs[0]
    s = d0.shard

    def streamed(H, iters, ee):
        return A.StreamedQuantizedMinSumDecoder(iters, early_exit=ee, device=d0.idx)

    def report(name, snr, tag, res, F, bpf, fer, desc):
        print("%s %6s  %-34s  %s k frames/s  kernel %s ms  model %.3f MB/frame -> %s GB/s  FER %.5f  [%s]"
              % (name, snr if isinstance(snr, str) else "%+.1f dB" % snr, tag, " / ".join("%8.1f" % (v / 1e3) for v, _ in res), " / ".join("%8.2f" % k for _, k in res), bpf / 1e6,
                 " / ".join("%7.1f" % (bpf * F / (k * 1e-3) / 1e9) for _, k in res), fer, desc), flush=True)

    def run_c5():
        H, cws = bench.load_c5(A)
        F, snr = args.frames, 2.0
        n, E = H.n, int(np.array(H.dense()).sum())
        batch = bench.Batch(rig, H, cws, F)
        lds = A.QuantizedMinSumDecoder(25, early_exit=False, device=d0.idx, lanes_per_frame=512)
        flo = A.MinSumDecoder(50, 0.75, early_exit=False, device=d0.idx, engine=A.ENGINE_STREAMED)
        sq = streamed(H, 25, False)
        batch.gen_noise({s: lds}, snr, 1)
        c = torch.empty((F, n), dtype=torch.int16, device=batch.y[s].device)
        lds.quantize_dev(H, batch.y[s].data_ptr(), False, F * n, snr, c.data_ptr(), d0.stream.cuda_stream)
        rig.sync_local()
        outs = (batch.bits[s].data_ptr(), batch.ok[s].data_ptr(), batch.its[s].data_ptr())
        legs = [("bp_layered_q_kernel L=512", lds, lambda d: lds.decode_llr_batch_dev(H, c.data_ptr(), F, *outs, None, d.stream.cuda_stream), None)]
        legs.append(("bp_streamed_q_kernel", sq, lambda d: sq.decode_llr_batch_dev(H, c.data_ptr(), F, *outs, None, d.stream.cuda_stream), model_bytes(n, E, 25, False)))
        legs.append(("float streamed min-sum, 50 sweeps", flo, lambda d: flo.decode_batch_dev(H, batch.y[s].data_ptr(), False, F, snr, *outs, d.stream.cuda_stream),
                     bench.bp_bytes_per_frame(n, E, 50)))
        res = {tag: [] for tag, _, _, _ in legs}
        fer = {}
        first = None
        for _ in range(args.runs):
            for tag, dec, step, bpf in legs:
                dt, kms, _info = rig.timed(step, args.steps, args.warmup)
                res[tag].append((F * args.steps / dt, kms))
                fer[tag] = batch.quality(F)["fer"]
                if dec is flo:
                    continue
                got = (batch.bits[s].clone(), batch.ok[s].clone(), batch.its[s].clone())
                if first is None:
                    first = got
                elif not all(bool((a == b).all()) for a, b in zip(got, first)):
                    raise SystemExit("c5: the leg '%s' returns other words, flags or iterations than bp_layered_q_kernel" % tag)
        for tag, dec, _, bpf in legs:
            report("5000x10000", snr, tag, res[tag], F, bpf or model_bytes(n, E, 25, False), fer[tag], dec.describe(H))
        # (a') the same two integer legs on channel values that are noise: no frame latches, so every lane stores in every iteration
        g = torch.Generator(device=c.device)
        g.manual_seed(1)
        c.copy_(torch.randint(-20, 32, (F, n), dtype=torch.int16, device=c.device, generator=g))
        rig.sync_local()
        res = {tag: [] for tag, _, _, _ in legs[:2]}
        first = None
        for _ in range(args.runs):
            for tag, dec, step, bpf in legs[:2]:
                dt, kms, _info = rig.timed(step, args.steps, args.warmup)
                res[tag].append((F * args.steps / dt, kms))
                got = (batch.bits[s].clone(), batch.ok[s].clone(), batch.its[s].clone())
                if first is None:
                    first = got
                elif not all(bool((a == b).all()) for a, b in zip(got, first)):
                    raise SystemExit("c5, noise: the leg '%s' returns other words, flags or iterations than bp_layered_q_kernel" % tag)
        latched = float(batch.ok[s].float().mean())
        for tag, dec, _, bpf in legs[:2]:
            report("5000x10000", "noise", tag + ", noise in", res[tag], F, model_bytes(n, E, 25, False), 1.0 - latched, "frames latched: %.5f" % latched)
        for dec in (lds, flo, sq):
            dec.close()

    def run_big():
        Hm = A.regular_ldpc(2050, 41000, 2, 40, seed=1)
        H = A.ParityCheckMatrix(Hm)
        F, snr = args.big_frames, 5.3
        n, E = H.n, int(Hm.sum())
        batch = bench.Batch(rig, H, np.zeros((1, n), dtype=np.uint8), F)
        decs = [("fixed work", streamed(H, 25, False)), ("early exit", streamed(H, 25, True))]
        batch.gen_noise({s: decs[0][1]}, snr, 1)
        c = torch.empty((F, n), dtype=torch.int16, device=batch.y[s].device)
        decs[0][1].quantize_dev(H, batch.y[s].data_ptr(), False, F * n, snr, c.data_ptr(), d0.stream.cuda_stream)
        rig.sync_local()
        outs = (batch.bits[s].data_ptr(), batch.ok[s].data_ptr(), batch.its[s].data_ptr())
        res = {tag: [] for tag, _ in decs}
        q = {}
        for _ in range(args.runs):
            for tag, dec in decs:
                dt, kms, _info = rig.timed(lambda d: dec.decode_llr_batch_dev(H, c.data_ptr(), F, *outs, None, d.stream.cuda_stream), args.steps, args.warmup)
                res[tag].append((F * args.steps / dt, kms))
                q[tag] = batch.quality(F)
        for tag, dec in decs:
            report("2050x41000", snr, "bp_streamed_q_kernel " + tag, res[tag], F, model_bytes(n, E, 25, True), q[tag]["fer"],
                   "mean iterations %.2f; %s" % (q[tag]["mean_iters"], dec.describe(H)))
            dec.close()

    if args.code in ("both", "c5"):
        run_c5()
    if args.code in ("both", "big"):
        run_big()


if __name__ == "__main__":
    main()
