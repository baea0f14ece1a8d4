"""What the Monte-Carlo GPU tests build their expectations from: the symbols of acg_ldpc_awgn_dev decoded through
decode_batch_dev on the decoder under test, to be classified by tests/mc_detail_ref.py — the decode path of the library,
never its classification."""
import ctypes as C

import numpy as np


def sent_words(cws, n, first, frames):
    if cws is None:
        return np.zeros((frames, n), dtype=np.uint8)
    return cws[(first + np.arange(frames, dtype=np.int64)) % len(cws)]


def mc_cfg(A, cws, snr, frames, first, seed, noise):
    from acg_alp_ldpc_amd import _lib
    cfg = _lib.McCfg()
    cfg.frames, cfg.first_frame, cfg.snr, cfg.seed = frames, first, snr, seed
    cfg.noise = _lib.NOISE_HOST_MT19937 if noise == "host" else _lib.NOISE_DEVICE_PHILOX
    if cws is not None:
        cfg.codewords, cfg.n_codewords = cws.ctypes.data, cws.shape[0]
    return cfg


def decode_device_noise(A, dec, H, cws, snr, frames, first, seed):
    """(y, packed words, ok, iters) of global frames [first, first + frames): awgn_dev + decode_batch_dev"""
    import torch
    from acg_alp_ldpc_amd._lib import check, lib
    h, _ = dec.handle(H)
    nw = (H.n + 31) // 32
    y = torch.empty((max(frames, 1), H.n), dtype=torch.float32, device="cuda")
    bits = torch.zeros((max(frames, 1), nw), dtype=torch.int32, device="cuda")
    ok = torch.zeros(max(frames, 1), dtype=torch.uint8, device="cuda")
    it = torch.zeros(max(frames, 1), dtype=torch.int32, device="cuda")
    if frames:
        cfg = mc_cfg(A, cws, snr, frames, first, seed, "device")
        check(lib().acg_ldpc_awgn_dev(h, C.byref(cfg), y.data_ptr(), None))
        dec.sync(H)
        dec.decode_batch_dev(H, y.data_ptr(), False, frames, snr, bits.data_ptr(), ok.data_ptr(), it.data_ptr())
        dec.sync(H)
    return (y.cpu().numpy()[:frames], bits.cpu().numpy().view(np.uint32)[:frames], ok.cpu().numpy()[:frames], it.cpu().numpy()[:frames])
