"""The three shapes the tests of the rate-matched Monte-Carlo run share (tests/test_rm_cabi.py on the CPU, tests/test_rm_gpu.py on
the device): the smallest at which each part of acg_ldpc_mc_run_rm can still go wrong.

  H05    data/H05.txt, 160 x 280, degree-1 variables; random words of data/G05.txt; -2.0 dB, 15 iterations, 300 frames; punctured
         v % 20 == 3 (14), shortened v % 20 == 11 (14): shortened bits that are 1, and the last packed word is partial
  deg40  regular_ldpc(30, 400, 3, 40, seed=3); the all-zero word; 4.0 dB, 10 iterations, 200 frames; punctured v % 100 == 7 (4),
         shortened v % 10 == 9 (40): wide checks, so the streamed handles only
  odd62  regular_ldpc(31, 62, 3, 6, seed=1); the all-zero word; 1.0 dB, 10 iterations, 200 frames; punctured v % 16 == 5,
         shortened v % 16 == 13; n % 4 == 2: a partial quad and a scalar-store tail

and the composition the device is held to, from public pieces that already exist: acg_ldpc_awgn_dev for the symbols, tests/rm_ref.py
for channel values and raw errors, the handle's own decode_llr_batch_dev for word, flag and iterations, rm_ref.counters."""
import ctypes as C
import os
import subprocess

import numpy as np

import awgn_ref
import layered_q_cases as Q
import rm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data")
MS_SCALE = 0.75
SEED = 2 ** 32 + 5

# name -> (SNR in dB, iterations, frames, punctured rule, shortened rule)
CASES = {
    "H05": (-2.0, 15, 300, lambda v: v % 20 == 3, lambda v: v % 20 == 11),
    "deg40": (4.0, 10, 200, lambda v: v % 100 == 7, lambda v: v % 10 == 9),
    "odd62": (1.0, 10, 200, lambda v: v % 16 == 5, lambda v: v % 16 == 13),
}

# engine -> which cases it takes (deg40: check degree 40 is beyond the LDS engine's 32)
ENGINES = {
    "float-bp": ("H05", "deg40", "odd62"),
    "float-ms": ("H05", "deg40", "odd62"),
    "q-lds": ("H05", "odd62"),
    "q-streamed": ("H05", "deg40", "odd62"),
}


def positions(name, n):
    """(punctured, shortened) index lists of a case"""
    _, _, _, pun, sho = CASES[name]
    return [v for v in range(n) if pun(v)], [v for v in range(n) if sho(v)]


class Case:
    def __init__(self, A, name):
        self.name = name
        self.snr, self.iters, self.frames = CASES[name][:3]
        self.cws = None
        if name == "H05":
            self.H = A.read_pcm(os.path.join(DATA, "H05.txt"))
            G = A.read_pcm(os.path.join(DATA, "G05.txt")).dense()
            self.cws = np.ascontiguousarray(A.gen_random_codewords(G, 37, 239239239), dtype=np.uint8)
        elif name == "deg40":
            self.H = A.ParityCheckMatrix(A.regular_ldpc(30, 400, 3, 40, seed=3))
        else:
            self.H = A.ParityCheckMatrix(A.regular_ldpc(31, 62, 3, 6, seed=1))
        self.n = self.H.n
        self.punctured, self.shortened = positions(name, self.n)
        self.pattern = A.rate_match_pattern(self.n, self.punctured, self.shortened)

    def sent(self, first, frames):
        return awgn_ref.sent_words(first, frames, self.n, self.cws)


_made = {}


def case(A, name):
    if name not in _made:
        _made[name] = Case(A, name)
    return _made[name]


def decoder(A, engine, it, quant="default", ee=True):
    if engine == "float-bp":
        return A.StreamedLayeredBPDecoder(it, early_exit=ee)
    if engine == "float-ms":
        return A.StreamedLayeredMinSumDecoder(it, MS_SCALE, early_exit=ee)
    cls = A.QuantizedMinSumDecoder if engine == "q-lds" else A.StreamedQuantizedMinSumDecoder
    return cls(it, quant=A.QuantConfig(*Q.QUANTS[quant]), early_exit=ee)


def quant_of(engine, quant="default"):
    """the 7-tuple rm_ref takes, None for the float engines"""
    return None if engine.startswith("float") else Q.QUANTS[quant]


def mc_cfg(c, first, frames, snr=None, seed=SEED, noise=0):
    """-> (McCfg, keep-alive): device noise unless noise says otherwise"""
    from acg_alp_ldpc_amd._lib import McCfg
    cfg = McCfg()
    cfg.frames, cfg.first_frame, cfg.snr, cfg.seed, cfg.noise = int(frames), int(first), float(c.snr if snr is None else snr), int(seed), int(noise)
    if c.cws is not None:
        cfg.codewords, cfg.n_codewords = c.cws.ctypes.data, c.cws.shape[0]
    return cfg


def awgn(dec, c, first, frames, snr=None, seed=SEED):
    """acg_ldpc_awgn_dev on the decoder's handle -> float32 [frames, n] on the host"""
    import torch
    from acg_alp_ldpc_amd._lib import check, lib
    h, _ = dec.handle(c.H)
    cfg = mc_cfg(c, first, frames, snr, seed)
    yd = torch.empty((frames, c.n), dtype=torch.float32, device="cuda")
    check(lib().acg_ldpc_awgn_dev(h, C.byref(cfg), yd.data_ptr(), None))
    dec.sync(c.H)
    return yd.cpu().numpy()


def rm_channel(dec, engine, c, pattern, first, frames, snr=None, seed=SEED, raw=True):
    """rm_channel_dev -> (values [frames, n] float32 or int16, raw [frames] int32 or None) on the host"""
    import torch
    cfg = mc_cfg(c, first, frames, snr, seed)
    out = torch.full((frames, c.n), 77, dtype=torch.float32 if engine.startswith("float") else torch.int16, device="cuda")
    rw = torch.full((frames,), -5, dtype=torch.int32, device="cuda") if raw else None
    dec.rm_channel_dev(c.H, cfg, pattern, out.data_ptr(), rw.data_ptr() if raw else None)
    dec.sync(c.H)
    return out.cpu().numpy(), (rw.cpu().numpy() if raw else None)


def unpack(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")[:, :n]


def composition(dec, engine, c, pattern, first, frames, quant="default", snr=None, seed=SEED):
    """the expectation of acg_ldpc_mc_run_rm: awgn_dev's symbols -> rm_ref's channel values and raw errors -> the handle's own
    decode_llr_batch_dev -> rm_ref.counters.  -> (the seven counters, ok [frames])"""
    import torch
    snr = c.snr if snr is None else snr
    y = awgn(dec, c, first, frames, snr, seed)
    sent = c.sent(first, frames)
    vals = rm_ref.channel_values(y, sent, snr, pattern, quant_of(engine, quant))
    raw = rm_ref.raw_errors(y, sent, pattern)
    vd = torch.from_numpy(np.ascontiguousarray(vals)).cuda()
    nw = (c.n + 31) // 32
    bits = torch.zeros((frames, nw), dtype=torch.int32, device="cuda")
    ok = torch.zeros(frames, dtype=torch.uint8, device="cuda")
    it = torch.zeros(frames, dtype=torch.int32, device="cuda")
    dec.decode_llr_batch_dev(c.H, vd.data_ptr(), frames, bits.data_ptr(), ok.data_ptr(), it.data_ptr())
    dec.sync(c.H)
    okh = ok.cpu().numpy()
    return rm_ref.counters(raw, unpack(bits.cpu().numpy(), c.n), okh, it.cpu().numpy(), sent), okh


def as_dict(r):
    return {f: getattr(r, f) for f in rm_ref.FIELDS}


def build_cxx_check(tmp_path):
    """tests/cxx_rm_check.cpp compiled with plain g++ against include/ and linked to the library -> the executable"""
    exe = str(tmp_path / "cxx_rm_check")
    libdir = os.path.join(ROOT, "acg_alp_ldpc_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx_rm_check.cpp"),
                           "-o", exe, "-L" + libdir, "-lacg_ldpc_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe
