#!/usr/bin/env python3
"""Rate of acg_ldpc_mc_run_rm (Monte-Carlo runs for punctured / shortened codes) beside acg_ldpc_mc_run on the same handle.

    python tools/mc_rm_rate.py [--reps 3] [--out profiles/mc_rm_rate.txt]

One handle per engine kind, 25 iterations fixed (no early exit), device noise, the all-zero word, in ONE process and session:
  (3,6) 5000 x 10 000 at +2 dB            float streamed (sum-product) and quantized at L = 512
  regular_ldpc(2050, 41000, 2, 40) at 5.3 dB   float streamed (sum-product) and quantized streamed
Per handle, behind one untimed round, `reps` rounds of  acg_ldpc_mc_run | acg_ldpc_mc_run_rm with an all-sent pattern  taken
alternately (so drift hits both alike); their seven counters must be equal.  Yardstick: the slowest _rm run against the fastest
acg_ldpc_mc_run run of the same session (>= 0.97 expected: the new path writes and reads fewer bytes per frame than noise ->
symbols -> decode -> classification on symbols).  Then `reps` runs with 10 % of the positions punctured (v % 10 == 3): FER and
rate.  Rates are frames / time_sec of the call (wall clock around work that ends in a device synchronisation)."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="rehearsal: tiny codes and frame counts")
    args = ap.parse_args()
    import numpy as np
    import acg_alp_ldpc_amd as A
    from acg_alp_ldpc_amd import _lib
    if not A.device_available():
        raise SystemExit("mc_rm_rate needs a HIP device")
    L = A.lib()
    ITERS = 25
    if args.small:
        codes = [("300x600", A.regular_ldpc(300, 600, 3, 6, seed=1), 2.0, 4096), ("30x400", A.regular_ldpc(30, 400, 3, 40, seed=3), 4.0, 4096)]
    else:
        codes = [("5000x10000", A.regular_ldpc(5000, 10000, 3, 6, seed=1), 2.0, 196608),
                 ("2050x41000", A.regular_ldpc(2050, 41000, 2, 40, seed=1), 5.3, 65536)]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    worst = None
    for ci, (cname, Hm, snr, frames) in enumerate(codes):
        H = A.ParityCheckMatrix(Hm)
        decs = [("float streamed", A.StreamedLayeredBPDecoder(ITERS, early_exit=False)),
                ("quantized L=512", A.QuantizedMinSumDecoder(ITERS, early_exit=False, lanes_per_frame=512)) if ci == 0 else
                ("quantized streamed", A.StreamedQuantizedMinSumDecoder(ITERS, early_exit=False))]
        all_sent = np.zeros(H.n, dtype=np.uint8)
        punctured = A.rate_match_pattern(H.n, punctured=range(3, H.n, 10))
        for dname, dec in decs:
            h, _ = dec.handle(H)
            cfg = _lib.McCfg()
            cfg.frames, cfg.first_frame, cfg.snr, cfg.seed, cfg.noise = frames, 0, snr, 1, _lib.NOISE_DEVICE_PHILOX

            def run(pattern):
                r = _lib.McResult()
                rc = L.acg_ldpc_mc_run(h, C.byref(cfg), C.byref(r)) if pattern is None else L.acg_ldpc_mc_run_rm(h, C.byref(cfg), pattern.ctypes.data, C.byref(r))
                assert rc == 0, L.acg_ldpc_last_error()
                return r, (r.correct, r.pseudo, r.total, r.sum_hamming, r.sum_hamming_ok, r.sum_hamming_wrong, r.sum_iters)

            rates = {"mc_run": [], "mc_run_rm": [], "punctured": []}
            kms = {"mc_run": [], "mc_run_rm": [], "punctured": []}
            for rep in range(args.reps + 1):            # round 0 is the warm-up (first-use allocations, clocks)
                a, ca = run(None)
                b, cb = run(all_sent)
                assert ca == cb, (ca, cb)               # an all-sent pattern is the plain run, counter for counter
                if rep:
                    for k, r in (("mc_run", a), ("mc_run_rm", b)):
                        rates[k].append(frames / r.time_sec)
                        kms[k].append(r.kernel_ms)
            fer0 = (a.total - a.correct) / a.total
            for rep in range(args.reps + 1):
                p, _ = run(punctured)
                if rep:
                    rates["punctured"].append(frames / p.time_sec)
                    kms["punctured"].append(p.kernel_ms)
            ferp = (p.total - p.correct) / p.total
            ratio = min(rates["mc_run_rm"]) / max(rates["mc_run"])
            worst = ratio if worst is None else min(worst, ratio)
            desc = dec.describe(H)
            for k, fer in (("mc_run", fer0), ("mc_run_rm", fer0), ("punctured", ferp)):
                label = {"mc_run": "acg_ldpc_mc_run", "mc_run_rm": "acg_ldpc_mc_run_rm all sent", "punctured": "acg_ldpc_mc_run_rm 10% punctured"}[k]
                say("%-10s %+.1f dB %6d frames fixed-%d %-18s %-32s %s k frames/s  decode kernel %s ms  FER %.5f" % (
                    cname, snr, frames, ITERS, dname, label, " / ".join("%8.1f" % (x / 1e3) for x in rates[k]),
                    " / ".join("%8.2f" % x for x in kms[k]), fer))
            say("%-10s %-18s slowest _rm run over fastest acg_ldpc_mc_run run: %.4f (%s 0.97)  [%s]" % (
                cname, dname, ratio, ">=" if ratio >= 0.97 else "BELOW", desc))
            dec.close()
    say("worst ratio over the four handles: %.4f" % worst)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
