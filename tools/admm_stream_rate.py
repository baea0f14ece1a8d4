"""Rate of the streamed QP-ADMM engine (csrc/admm_streamed.hip) against its HBM byte model.

    python tools/admm_stream_rate.py [--frames F] [--reps R] [--json FILE]

configs[4] (the (3,6)-regular 5000 x 10000 code) with QP-ADMM(1.2, 0.55, 100, 1e-5) in fp64 and fp32, fixed work
(early_exit = 0: 100 sweeps per frame) and residual exit, at -1 and +2 dB; then H05 with the streamed engine forced
beside the default LDS kernel.  Symbols are generated on the host and decoded from HBM (acg_ldpc_decode_batch_dev); the
time is the kernel's own event pair (median of R launches after one warm-up).

Byte model per frame and sweep: (nnz + n + n_var + sum of group sizes + 2C) * b.  A tile of 64 frames runs
until its slowest frame has exited, so with residual exit the sweeps counted are each tile's largest sweep count (fixed
work: 100).  Frames that have exited stop writing, so fixed work at a high SNR moves fewer bytes than the model says.
Printed: frames/s, modelled bytes per frame, modelled bandwidth and its fraction of 6.3 TB/s (the copy rate measured in
the microarchitecture guide).  The bandwidth is a model figure, not a counter reading.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import acg_alp_ldpc_amd as A  # noqa: E402

COPY_BW = 6.3e12


def model_words(Hm):
    """(nnz + n + n_var + sum of group sizes + 2C) of ConstructADMMProblem (qp_admm.h:13-102)"""
    deg = (np.asarray(Hm) != 0).sum(axis=1)
    n = Hm.shape[1]
    nnz = grp = C = aux = 0
    for d in deg.tolist():
        if d == 1:
            nnz, grp, C = nnz + 1, grp + 1, C + 1
        elif d == 2:
            nnz, grp, C = nnz + 4, grp + 2, C + 2
        elif d >= 3:
            g = d - 2
            nnz, grp, C, aux = nnz + 12 * g, grp + 3 * g, C + 4 * g, aux + d - 3
    return nnz + n + (n + aux) + grp + 2 * C


def leg(dec, H, y_dev, frames, snr, reps, words, b, fixed=False):
    import torch
    nw = (H.n + 31) // 32
    bits = torch.empty((frames, nw), dtype=torch.int32, device="cuda")
    ok = torch.empty(frames, dtype=torch.uint8, device="cuda")
    it = torch.empty(frames, dtype=torch.int32, device="cuda")
    ms = []
    for r in range(reps + 1):
        dec.decode_batch_dev(H, y_dev.data_ptr(), False, frames, snr, bits.data_ptr(), ok.data_ptr(), it.data_ptr())
        dec.sync(H)
        if r:
            ms.append(dec.last_kernel_ms(H))
    k = float(np.median(ms))
    iters = it.cpu().numpy()
    pad = (-frames) % 64
    tile_max = np.concatenate([iters, np.zeros(pad, iters.dtype)]).reshape(-1, 64).max(axis=1)
    sweeps = float(tile_max.sum()) * 64 / frames   # sweeps per frame the tiles actually ran
    if fixed:
        sweeps = float(dec.max_iter)                # fixed work: every tile runs max_iter sweeps
    bpf = words * b * sweeps
    fps = frames / (k * 1e-3)
    return dict(frames=frames, kernel_ms=round(k, 3), frames_per_s=round(fps, 1), mean_sweeps=round(float(iters.mean()), 2),
                tile_sweeps_per_frame=round(sweeps, 2), model_bytes_per_frame=int(bpf), model_TBps=round(fps * bpf / 1e12, 3),
                fraction_of_6p3=round(fps * bpf / COPY_BW, 3), describe=dec.describe(H))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=0, help="configs[4] frames per launch (0 = one tile per slab)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default="", help="also write every result row to this file")
    a = ap.parse_args()
    import torch
    out = []
    Hm = A.regular_ldpc(5000, 10000, 3, 6, seed=1)
    H = A.ParityCheckMatrix(Hm)
    G, _ = H.get_orthogonal()
    words = model_words(Hm)
    print("configs[4]: %d words per frame and sweep (%.2f MB fp64)" % (words, words * 8 / 1e6), flush=True)
    for prec, tag, b in ((A.PREC_F64, "fp64", 8), (A.PREC_F32, "fp32", 4)):
        for ee in (False, True):
            dec = A.QPADMMDecoder(1.2, 0.55, 100, 1e-5, precision=prec, early_exit=ee)
            frames = a.frames or dec.layout(H)["grid_blocks"] * 64
            for snr in (-1.0, 2.0):
                cws = A.gen_random_codewords(G, 256, 17)
                y = torch.from_numpy(A.transmit_frames(cws, snr, first_frame=0, frames=frames).astype(np.float32)).cuda()
                r = leg(dec, H, y, frames, snr, a.reps, words, b, fixed=not ee)
                r.update(code="configs[4]", precision=tag, mode="residual_exit" if ee else "fixed_100", snr=snr)
                out.append(r)
                print(json.dumps(r), flush=True)
                del y
            dec.close()
    Hm5 = A.read_pcm(os.path.join(ROOT, "data", "H05.txt"))
    G5, _ = Hm5.get_orthogonal()
    w5 = model_words(np.asarray(Hm5.dense()))
    frames = 1 << 17
    cws = A.gen_random_codewords(G5, 256, 17)
    y = torch.from_numpy(A.transmit_frames(cws, -1.0, first_frame=0, frames=frames).astype(np.float32)).cuda()
    for eng, tag in ((A.ENGINE_STREAMED, "streamed"), (A.ENGINE_AUTO, "lds")):
        dec = A.QPADMMDecoder(1.95, 0.5, 100, 1e-5, engine=eng)
        r = leg(dec, Hm5, y, frames, -1.0, a.reps, w5, 8)
        r.update(code="H05", precision="fp64", mode="residual_exit", snr=-1.0, engine=tag)
        if tag == "lds":
            for k in ("model_bytes_per_frame", "model_TBps", "fraction_of_6p3"):
                r.pop(k)   # the byte model is the streamed engine's; the LDS kernel moves only symbols and bits
        out.append(r)
        print(json.dumps(r), flush=True)
        dec.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
