#!/usr/bin/env python3
"""frames/s, kernel ms and achieved bytes/s of the streamed float layered engine (acg_ldpc_decoder_create_layered_streamed,
bp_streamed_layered_kernel) on device-resident symbols in one session, `--runs` rounds (default 3), each timing `--steps` steps
behind `--warmup` warm-up steps.  The legs of (a) alternate; those of (b) and (c) run one decoder at a time, because a
workspace is sized by the memory that is free when its handle is made.

  (a) c5     BASELINE configs[4], the (3,6)-regular 5000 x 10000, +2 dB, 25 iterations, fixed work: this engine, sum-product and
             min-sum(0.75), against bp_layered_block_kernel at lanes_per_frame = 1024 on the same frames — the same algorithm
             over the same sets, so words, flags and iterations are asserted equal — against the flooding streamed engine at
             50 sweeps, and against bp_streamed_q_kernel (default quantiser) on the channel values of those symbols.
  (b) big    regular_ldpc(2050, 41000, 2, 40, seed=1), 5.3 dB, 25 iterations, fixed work: rate and FER of both algorithms.  No
             other float engine takes this code.
  (c) caps   the resident tiles per CU (ACG_STREAML_PER_CU, developer switch read at creation) 4 / 8 / 12 / 16 on both codes,
             one round each.

Bytes: the model of a frame is 16 E per iteration for a check of up to 8 variables (P and R read, P and R written, fp32), 24 E
for a wider one (P and R read twice), + 8 E for a wide sum-product check with the stored magnitudes (written and read once) or
+ 0 with the recomputed ones, + 8 n in (symbols read, P written) + 4 n read for the word + 4 ceil(n / 32) + 5 out.  It is that
of 25 full iterations: a lane whose frame has latched writes nothing, so the kernel moves fewer bytes than the model where
frames latch.  The other engines' models: bench.bp_bytes_per_frame (flooding), tools/streamed_q_rate.model_bytes (integer).

    python3 tools/streamed_layered_rate.py                   all three
    python3 tools/streamed_layered_rate.py --code big --algos bp      one code, one algorithm (e.g. with ACG_LDPC_LIB naming a
                                                                     library built with -DACG_SL_STORE_MAG=1)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def model_bytes(n, E, iters, wide, spa_stored):
    per_edge = (24 if wide else 16) + (8 if wide and spa_stored else 0)
    return per_edge * E * iters + 8 * n + 4 * n + 4 * ((n + 31) // 32) + 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--code", choices=("all", "c5", "big", "caps"), default="all")
    ap.add_argument("--algos", default="bp,minsum")
    ap.add_argument("--frames", type=int, default=196608)
    ap.add_argument("--big-frames", type=int, default=131072)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    algos = args.algos.split(",")
    import numpy as np
    import torch
    import acg_alp_ldpc_amd as A
    import bench
    import streamed_q_rate
    rig = bench.Rig(type("a", (), dict(inproc=0, gpus=1))())
    d0 = rig.devs[0]
    s = d0.shard
    ITERS, SCALE = 25, 0.75

    def streamed(algo, ee=False):
        if algo == "bp":
            return A.StreamedLayeredBPDecoder(ITERS, early_exit=ee, device=d0.idx)
        return A.StreamedLayeredMinSumDecoder(ITERS, SCALE, early_exit=ee, device=d0.idx)

    def report(name, snr, F, tag, res, bpf, q, desc):
        print("%s %+.1f dB %d frames  %-44s  %s k frames/s  kernel %s ms  model %.3f MB/frame -> %s GB/s  FER %.5f  mean iterations %.2f  [%s]"
              % (name, snr, F, tag, " / ".join("%7.1f" % (v / 1e3) for v, _ in res), " / ".join("%8.2f" % k for _, k in res), bpf / 1e6,
                 " / ".join("%7.1f" % (bpf * F / (k * 1e-3) / 1e9) for _, k in res), q["fer"], q["mean_iters"], desc), flush=True)

    def stored(dec, H):
        return "wide_mag=stored" in dec.describe(H)

    def run_c5():
        H, cws = bench.load_c5(A)
        F, snr = args.frames, 2.0
        n, E = H.n, int(np.array(H.dense()).sum())
        batch = bench.Batch(rig, H, cws, F)
        outs = (batch.bits[s].data_ptr(), batch.ok[s].data_ptr(), batch.its[s].data_ptr())

        def sym(dec):
            return lambda d: dec.decode_batch_dev(H, batch.y[s].data_ptr(), False, F, snr, *outs, d.stream.cuda_stream)
        legs = []   # (tag, decoder, step, model bytes per frame, group whose outputs must be equal or None)
        kw = dict(early_exit=False, device=d0.idx)
        for algo in algos:
            sl = streamed(algo)
            lds = (A.BeliefPropagationDecoder(ITERS, schedule=A.SCHEDULE_LAYERED, lanes_per_frame=1024, **kw) if algo == "bp" else
                   A.MinSumDecoder(ITERS, SCALE, schedule=A.SCHEDULE_LAYERED, lanes_per_frame=1024, **kw))
            flo = (A.BeliefPropagationDecoder(50, engine=A.ENGINE_STREAMED, **kw) if algo == "bp" else
                   A.MinSumDecoder(50, SCALE, engine=A.ENGINE_STREAMED, **kw))
            legs.append(("bp_streamed_layered_kernel<%s>" % algo, sl, sym(sl), model_bytes(n, E, ITERS, False, False), algo))
            legs.append(("bp_layered_block_kernel L=1024 %s" % algo, lds, sym(lds), model_bytes(n, E, ITERS, False, False), algo))
            legs.append(("flooding streamed %s, 50 sweeps" % algo, flo, sym(flo), bench.bp_bytes_per_frame(n, E, 50), None))
        sq = A.StreamedQuantizedMinSumDecoder(ITERS, **kw)
        batch.gen_noise({s: legs[0][1]}, snr, 1)
        c = torch.empty((F, n), dtype=torch.int16, device=batch.y[s].device)
        sq.quantize_dev(H, batch.y[s].data_ptr(), False, F * n, snr, c.data_ptr(), d0.stream.cuda_stream)
        rig.sync_local()
        legs.append(("bp_streamed_q_kernel (int16 channel values)", sq, lambda d: sq.decode_llr_batch_dev(H, c.data_ptr(), F, *outs, None, d.stream.cuda_stream),
                     streamed_q_rate.model_bytes(n, E, ITERS, False), None))
        res = {tag: [] for tag, *_ in legs}
        q, first = {}, {}
        for _ in range(args.runs):
            for tag, dec, step, bpf, group in legs:
                dt, kms, _info = rig.timed(step, args.steps, args.warmup)
                res[tag].append((F * args.steps / dt, kms))
                q[tag] = batch.quality(F)
                if group is None:
                    continue
                got = (batch.bits[s].clone(), batch.ok[s].clone(), batch.its[s].clone())
                if group not in first:
                    first[group] = got
                elif not all(bool((a == b).all()) for a, b in zip(got, first[group])):
                    raise SystemExit("c5: the leg '%s' returns other words, flags or iterations than the other %s engine" % (tag, group))
        for tag, dec, _, bpf, _g in legs:
            report("5000x10000", snr, F, tag, res[tag], bpf, q[tag], dec.describe(H))
            dec.close()

    def big_code():
        Hm = A.regular_ldpc(2050, 41000, 2, 40, seed=1)
        return A.ParityCheckMatrix(Hm), int(Hm.sum())

    def run_big():
        H, E = big_code()
        F, snr, n = args.big_frames, 5.3, 41000
        batch = bench.Batch(rig, H, np.zeros((1, n), dtype=np.uint8), F)
        outs = (batch.bits[s].data_ptr(), batch.ok[s].data_ptr(), batch.its[s].data_ptr())
        # (one decoder at a time: each workspace is sized by the memory that is free when it is made)
        for k, algo in enumerate(algos):
            dec = streamed(algo)
            if k == 0:
                batch.gen_noise({s: dec}, snr, 1)
            res = []
            for _ in range(args.runs):
                dt, kms, _info = rig.timed(lambda d: dec.decode_batch_dev(H, batch.y[s].data_ptr(), False, F, snr, *outs, d.stream.cuda_stream), args.steps, args.warmup)
                res.append((F * args.steps / dt, kms))
            report("2050x41000", snr, F, "bp_streamed_layered_kernel<%s> fixed work" % algo, res, model_bytes(n, E, ITERS, True, algo == "bp" and stored(dec, H)),
                   batch.quality(F), dec.describe(H))
            dec.close()

    def run_caps():
        H5, cws5 = bench.load_c5(A)
        Hb, Eb = big_code()
        for name, H, cws, F, snr in (("5000x10000", H5, cws5, args.frames, 2.0), ("2050x41000", Hb, np.zeros((1, 41000), dtype=np.uint8), args.big_frames, 5.3)):
            batch = bench.Batch(rig, H, cws, F)
            outs = (batch.bits[s].data_ptr(), batch.ok[s].data_ptr(), batch.its[s].data_ptr())
            made = False
            for algo in algos:
                line = []
                for cap in (4, 8, 12, 16):
                    os.environ["ACG_STREAML_PER_CU"] = str(cap)
                    dec = streamed(algo)
                    dec.handle(H)
                    del os.environ["ACG_STREAML_PER_CU"]
                    if not made:
                        batch.gen_noise({s: dec}, snr, 1)
                        made = True
                    dt, kms, _info = rig.timed(lambda d: dec.decode_batch_dev(H, batch.y[s].data_ptr(), False, F, snr, *outs, d.stream.cuda_stream), args.steps, args.warmup)
                    line.append("%d per CU (tiles=%d): %.1f" % (cap, dec.layout(H)["grid_blocks"], F * args.steps / dt / 1e3))
                    dec.close()
                print("%s %+.1f dB %d frames  tile cap, %s, k frames/s:  %s" % (name, snr, F, algo, "   ".join(line)), flush=True)
            del batch
            torch.cuda.empty_cache()

    if args.code in ("all", "c5"):
        run_c5()
    if args.code in ("all", "big"):
        run_big()
    if args.code in ("all", "caps"):
        run_caps()


if __name__ == "__main__":
    main()
