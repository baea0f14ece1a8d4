#!/usr/bin/env python3
"""Rate of acg_ldpc_mc_run_detail beside acg_ldpc_mc_run, and of acg_ldpc_mc_run before and after the detail run was added.

    python tools/mc_detail_rate.py --parent-lib /path/to/parent/libacg_ldpc_hip.so [--frames 1000000] [--reps 3]

H05 at -2 dB, device noise, the same frames in every leg.  In ONE process and one session, per decoder, `reps` rounds of
    parent acg_ldpc_mc_run | new acg_ldpc_mc_run | detail cap 0 | detail cap 4096 + words
taken alternately (so drift hits every leg alike), after one untimed round.  Reports median and range of the wall-clock
rate (frames / time_sec of the call) per leg, the parent's own run-to-run range, and whether the new library's median lies
inside it and whether it is not below the parent's minimum (the pass criterion of a change that must not slow anything:
the parent's own range is the only margin).  --parent-lib: the library of the parent commit, built from a checkout of that
commit (make -C acg_alp_ldpc_amd/csrc); without it the comparison legs are skipped.  A parent that exports
acg_ldpc_mc_run_detail also runs its own detail cap 0 leg, and one that exports acg_ldpc_mc_run_grid the grid leg.
Decoders: BP-50 with early exit (acg_ldpc_mc_run is ONE fused Monte-Carlo kernel there, so the detail run pays the separate
noise and classification stages) and the layered min-sum engine with one workgroup per frame (noise kernel -> decode ->
classification in both calls, so the difference is the extra classification work alone), and QP-ADMM with 100 sweeps (the
benchmark's qpadmm100 Monte-Carlo leg: noise kernel -> decode -> classification).  Last, one 36-point x 1000-frame
acg_ldpc_mc_run_grid leg on the QP-ADMM decoder (rate in virtual frames = points x frames per second)."""
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
                 "acg_ldpc_decoder_destroy", "acg_ldpc_mc_run", "acg_ldpc_mc_run_detail", "acg_ldpc_mc_run_grid"):
        f = getattr(L, name, None)
        if f is not None:
            f.restype, f.argtypes = _lib.SYMBOLS[name]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--frames", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--snr", type=float, default=-2.0)
    ap.add_argument("--new-first", action="store_true", help="every new leg before its parent leg (tells an order effect from a real one)")
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
        if kind == "qpadmm100":
            p.algo, p.max_iter = _lib.ALGO_QPADMM, 100      # (alpha 1.95, mu 0.5, eps_stop 1e-5: the defaults)
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
    report = {"frames": args.frames, "snr": args.snr, "reps": args.reps, "new_first": args.new_first, "decoders": {}}

    def compare(out, new_leg, parent_leg):
        p, med = out[parent_leg], out[new_leg]["median_frames_per_s"]
        out[new_leg]["within_parent_range"] = bool(p["min"] <= med <= p["max"])
        out[new_leg]["not_below_parent_min"] = bool(med >= p["min"])
        out[new_leg]["over_parent_median"] = med / p["median_frames_per_s"]

    def show(kind, out):
        for k, v in out.items():
            print("%-16s %-22s median %8.2f M frames/s  range [%8.2f, %8.2f]  %s" % (
                kind, k, v["median_frames_per_s"] / 1e6, v["min"] / 1e6, v["max"] / 1e6,
                "  ".join("%s=%s" % (a, ("%.3f" % b) if isinstance(b, float) else b) for a, b in v.items()
                          if a not in ("median_frames_per_s", "min", "max"))), flush=True)

    def rounds(legs, frames):
        """reps timed rounds of every leg in turn behind one untimed round -> leg -> rates; every leg must count alike"""
        if args.new_first:
            legs = dict(sorted(legs.items(), key=lambda kv: kv[0].startswith("parent_")))
        times = {k: [] for k in legs}
        counts = {}
        for rep in range(args.reps + 1):            # round 0 is the warm-up (first-use allocations, clocks)
            for k, fn in legs.items():
                t, c = fn()
                counts.setdefault(k, c)
                assert counts[k] == c
                if rep:
                    times[k].append(frames / t)
        assert len(set(counts.values())) == 1, counts           # every leg counted the same frames the same way
        return {k: {"median_frames_per_s": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}

    for kind in ("bp50_early_exit", "layered_block", "qpadmm100"):
        legs = {}

        def mc_run(L, dec):
            r = _lib.McResult()
            assert L.acg_ldpc_mc_run(dec, C.byref(cfg), C.byref(r)) == 0, L.acg_ldpc_last_error()
            return r.time_sec, (r.correct, r.pseudo, r.total, r.sum_hamming, r.sum_iters)

        def detail(dec, cap, words, L=new):
            d = _lib.McDetail()
            assert L.acg_ldpc_mc_run_detail(dec, C.byref(cfg), C.byref(d), ev.ctypes.data if cap else None,
                                            wd.ctypes.data if words else None, cap) == 0, L.acg_ldpc_last_error()
            b = d.base
            return b.time_sec, (b.correct, b.pseudo, b.total, b.sum_hamming, b.sum_iters)

        dn = handle(new, kind)
        if old:
            do = handle(old, kind)
            legs["parent_mc_run"] = lambda: mc_run(old, do)
        legs["new_mc_run"] = lambda: mc_run(new, dn)
        if old and hasattr(old, "acg_ldpc_mc_run_detail"):
            legs["parent_detail_cap0"] = lambda: detail(do, 0, False, old)
        legs["detail_cap0"] = lambda: detail(dn, 0, False)
        legs["detail_cap4096_words"] = lambda: detail(dn, 4096, True)
        out = rounds(legs, args.frames)
        base = out["new_mc_run"]["median_frames_per_s"]
        for k in ("detail_cap0", "detail_cap4096_words"):
            out[k]["mc_run_over_detail"] = base / out[k]["median_frames_per_s"]
        if old:
            compare(out, "new_mc_run", "parent_mc_run")
        if "parent_detail_cap0" in out:
            compare(out, "detail_cap0", "parent_detail_cap0")
        report["decoders"][kind] = out
        show(kind, out)
        if kind == "qpadmm100":
            # 6 x 6 points around the decoder's own, 1000 frames each, in one call
            al = np.ascontiguousarray([a for a in np.linspace(0.6, 1.95, 6) for _ in range(6)], dtype=np.float64)
            mu = np.ascontiguousarray([m for _ in range(6) for m in np.linspace(0.3, 0.9, 6)], dtype=np.float64)
            gcfg = _lib.McCfg()
            gcfg.frames, gcfg.first_frame, gcfg.snr, gcfg.seed, gcfg.noise = 1000, 0, args.snr, 1, _lib.NOISE_DEVICE_PHILOX
            gcfg.codewords, gcfg.n_codewords = cws.ctypes.data, cws.shape[0]

            def grid(L, dec):
                res = (_lib.McResult * 36)()
                assert L.acg_ldpc_mc_run_grid(dec, C.byref(gcfg), al.ctypes.data, mu.ctypes.data, 36, res) == 0, L.acg_ldpc_last_error()
                return res[0].time_sec, tuple((r.correct, r.pseudo, r.total, r.sum_hamming, r.sum_iters) for r in res)

            glegs = {}
            if old and hasattr(old, "acg_ldpc_mc_run_grid"):
                glegs["parent_mc_run_grid"] = lambda: grid(old, do)
            glegs["new_mc_run_grid"] = lambda: grid(new, dn)
            gout = rounds(glegs, 36 * 1000)
            if "parent_mc_run_grid" in gout:
                compare(gout, "new_mc_run_grid", "parent_mc_run_grid")
            report["decoders"]["qpadmm100_grid36x1000"] = gout
            show("qpadmm100_grid", gout)
        for L, d in ((new, dn),) + (((old, do),) if old else ()):
            L.acg_ldpc_decoder_destroy(d)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
