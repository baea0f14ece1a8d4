#!/usr/bin/env python3
"""Rate of acg_ldpc_mc_run_detail beside acg_ldpc_mc_run, and of acg_ldpc_mc_run before and after the detail run was added.

    python tools/mc_detail_rate.py --parent-lib /path/to/parent/libacg_ldpc_hip.so [--frames 1000000] [--reps 3]

H05 at -2 dB, device noise, the same frames in every leg.  In ONE process and one session, per decoder, `reps` rounds of
    parent acg_ldpc_mc_run | new acg_ldpc_mc_run | detail cap 0 | detail cap 4096 + words
taken alternately (so drift hits every leg alike), after one untimed round.  Reports median and range of the wall-clock
rate (frames / time_sec of the call) per leg, the parent's own run-to-run range, and whether the new library's median lies
inside it.  --parent-lib: the library of the parent commit, built from a checkout of that commit (make -C
acg_alp_ldpc_amd/csrc); without it the comparison legs are skipped.
Decoders: BP-50 with early exit (acg_ldpc_mc_run is ONE fused Monte-Carlo kernel there, so the detail run pays the separate
noise and classification stages) and the layered min-sum engine with one workgroup per frame (noise kernel -> decode ->
classification in both calls, so the difference is the extra classification work alone)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bind(path):
    """the few entry points the comparison needs, from a library that may predate the detail run"""
    from acg_alp_ldpc_amd import _lib
    L = C.CDLL(path)
    for name in ("acg_ldpc_params_default", "acg_ldpc_last_error", "acg_ldpc_code_from_dense", "acg_ldpc_decoder_create",
                 "acg_ldpc_decoder_destroy", "acg_ldpc_mc_run"):
        f = getattr(L, name)
        f.restype, f.argtypes = _lib.SYMBOLS[name]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--frames", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--snr", type=float, default=-2.0)
    args = ap.parse_args()
    import numpy as np
    import acg_alp_ldpc_amd as A
    from acg_alp_ldpc_amd import _lib
    new = A.lib()
    old = bind(args.parent_lib) if args.parent_lib else None
    H = A.read_pcm(os.path.join(ROOT, "data", "H05.txt"))
    Hd = np.ascontiguousarray(H.dense(), dtype=np.uint8)
    G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 8192, 239239239)
    nwords = (H.n + 31) // 32

    def params(L, kind):
        p = _lib.Params()
        L.acg_ldpc_params_default(C.byref(p))
        p.max_iter = 50
        if kind == "layered_block":
            p.algo, p.max_iter, p.ms_scale, p.schedule, p.lanes_per_frame = _lib.ALGO_MINSUM, 25, 0.75, _lib.SCHEDULE_LAYERED, 256
        return p

    def handle(L, kind):
        code, dec = C.c_void_p(), C.c_void_p()
        assert L.acg_ldpc_code_from_dense(Hd.ctypes.data, H.m, H.n, C.byref(code)) == 0
        p = params(L, kind)
        assert L.acg_ldpc_decoder_create(code, C.byref(p), C.byref(dec)) == 0, L.acg_ldpc_last_error()
        return dec

    cfg = _lib.McCfg()
    cfg.frames, cfg.first_frame, cfg.snr, cfg.seed, cfg.noise = args.frames, 0, args.snr, 1, _lib.NOISE_DEVICE_PHILOX
    cfg.codewords, cfg.n_codewords = cws.ctypes.data, cws.shape[0]
    ev = np.zeros(4096, dtype=A.experiment.EVENT_DTYPE)
    wd = np.zeros((4096, nwords), dtype=np.uint32)
    report = {"frames": args.frames, "snr": args.snr, "reps": args.reps, "decoders": {}}
    for kind in ("bp50_early_exit", "layered_block"):
        legs = {}

        def mc_run(L, dec):
            r = _lib.McResult()
            assert L.acg_ldpc_mc_run(dec, C.byref(cfg), C.byref(r)) == 0, L.acg_ldpc_last_error()
            return r.time_sec, (r.correct, r.pseudo, r.total, r.sum_hamming, r.sum_iters)

        def detail(dec, cap, words):
            d = _lib.McDetail()
            assert new.acg_ldpc_mc_run_detail(dec, C.byref(cfg), C.byref(d), ev.ctypes.data if cap else None,
                                              wd.ctypes.data if words else None, cap) == 0, new.acg_ldpc_last_error()
            b = d.base
            return b.time_sec, (b.correct, b.pseudo, b.total, b.sum_hamming, b.sum_iters)

        dn = handle(new, kind)
        if old:
            do = handle(old, kind)
            legs["parent_mc_run"] = lambda: mc_run(old, do)
        legs["new_mc_run"] = lambda: mc_run(new, dn)
        legs["detail_cap0"] = lambda: detail(dn, 0, False)
        legs["detail_cap4096_words"] = lambda: detail(dn, 4096, True)
        times = {k: [] for k in legs}
        counts = {}
        for rep in range(args.reps + 1):            # round 0 is the warm-up (first-use allocations, clocks)
            for k, fn in legs.items():
                t, c = fn()
                counts.setdefault(k, c)
                assert counts[k] == c
                if rep:
                    times[k].append(args.frames / t)
        assert len(set(counts.values())) == 1, counts           # every leg counted the same frames the same way
        out = {k: {"median_frames_per_s": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}
        base = out["new_mc_run"]["median_frames_per_s"]
        for k in ("detail_cap0", "detail_cap4096_words"):
            out[k]["mc_run_over_detail"] = base / out[k]["median_frames_per_s"]
        if old:
            p = out["parent_mc_run"]
            out["new_mc_run"]["within_parent_range"] = bool(p["min"] <= base <= p["max"])
            out["new_mc_run"]["over_parent_median"] = base / p["median_frames_per_s"]
        report["decoders"][kind] = out
        for L, d in ((new, dn),) + (((old, do),) if old else ()):
            L.acg_ldpc_decoder_destroy(d)
        for k, v in out.items():
            print("%-16s %-22s median %8.2f M frames/s  range [%8.2f, %8.2f]  %s" % (
                kind, k, v["median_frames_per_s"] / 1e6, v["min"] / 1e6, v["max"] / 1e6,
                "  ".join("%s=%s" % (a, ("%.3f" % b) if isinstance(b, float) else b) for a, b in v.items()
                          if a not in ("median_frames_per_s", "min", "max"))), flush=True)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
