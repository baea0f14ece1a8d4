#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — writes tests/golden/ref_answers.npz: what the REAL reference (oracle/_ref/libacg_ref.so, built by
`make -C oracle ref` where the reference tree exists) answers to the questions tests/test_oracle_vs_ref.py asks the oracle —
parsing, generator matrices, codewords, channel words, the QP-ADMM matrix, decoded words and Monte-Carlo counts.

    python oracle/make_golden_vs_ref.py

The test holds the oracle to this file on every machine, and to the live reference as well where that is built.  Every
function below takes the implementation to ask (`Oracle()` or `Ref()`, same methods) and the oracle, which makes the inputs;
it returns {key: array}, so the file and the test are the same code.  Everything written is data, no reference source text.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data")
OUT = os.path.join(ROOT, "tests", "golden", "ref_answers.npz")

FILES = ("H.txt", "H05.txt", "optimalH.txt", "G05.txt")
FRESH_SNRS = (-3.0, -1.0, 4.0)
EXPERIMENT_KEYS = ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong")


def _reset(impl):
    """the reference's global BP node counter changes a summation order: start every decode from the same state"""
    if getattr(impl, "is_ref", False):
        impl.reset_node_counter()


def parse_and_generators(impl, oracle):
    out = {}
    for fn in FILES:
        out["pcm_" + fn[:-4]] = impl.read_pcm(os.path.join(DATA, fn))
    H = oracle.read_pcm(os.path.join(DATA, "optimalH.txt"))
    G, ok = impl.get_orthogonal(H)
    out["G_optimalH"], out["G_optimalH_ok"] = G, np.array(bool(ok))
    bad = H.copy()
    bad[5] = 0
    out["G_bad_ok"] = np.array(bool(impl.get_orthogonal(bad)[1]))
    for seed in (239, 239239239):
        out["codewords_%d" % seed] = impl.gen_codewords(G, seed, 40)
    cw = oracle.gen_codewords(oracle.get_orthogonal(H)[0], 1, 3)
    for seed in (1, 2, 12345):
        for snr in (-5.0, -0.5, 3.0):
            out["transmit_%d_%+.1f" % (seed, snr)] = impl.transmit(seed, snr, cw[1])
    out["is_codeword"] = np.array([bool(impl.is_codeword(H, c)) for c in cw])
    c = cw[0].copy()
    c[7] ^= 1
    out["is_codeword_flipped"] = np.array(bool(impl.is_codeword(H, c)))
    return out


def admm_matrices(impl, matrices):
    out = {}
    for name, H in matrices.items():
        for part, x in zip(("col_ptr", "con", "coef", "b"), impl.admm_matrix(H)):
            out["admm_%s_%s" % (name, part)] = x
    return out


def fresh_frames(impl, oracle, matrices, snr):
    """frames NOT in the golden set (seeds 5000+), incl. +4 dB where infinities appear"""
    H = matrices["H05"]
    G, _ = oracle.get_orthogonal(H)
    cws = oracle.gen_codewords(G, 77, 60)
    y = oracle.transmit_frames(cws, snr, first_seed=5000)
    tag = "%+.1f" % snr
    _reset(impl)
    bits, ok, _ = impl.bp_decode(H, y, snr, 30, threads=4)
    out = {"bp_bits_" + tag: bits, "bp_ok_" + tag: ok}
    bits, ok, _ = impl.qpadmm_decode(H, y, snr, 1.95, 0.5, 60, 1e-5, threads=4)
    out.update({"qpadmm_bits_" + tag: bits, "qpadmm_ok_" + tag: ok})
    return out


def experiment_counts(impl, oracle, matrices):
    H = matrices["optimalH"]
    G, _ = oracle.get_orthogonal(H)
    cws = oracle.gen_codewords(G, 239, 120)
    out = {}
    for kind, it, a, m in (("bp", 25, 0, 0), ("qpadmm", 80, 1.2, 0.55)):
        _reset(impl)
        r = impl.experiment(kind, H, cws, -2.5, it, a, m)
        out["experiment_" + kind] = np.array([r[k] for k in EXPERIMENT_KEYS], dtype=np.int64)
    return out


def answers(impl, oracle, matrices):
    out = parse_and_generators(impl, oracle)
    out.update(admm_matrices(impl, matrices))
    for snr in FRESH_SNRS:
        out.update(fresh_frames(impl, oracle, matrices, snr))
    out.update(experiment_counts(impl, oracle, matrices))
    return out


def load_matrices(oracle):
    return {name: oracle.read_pcm(os.path.join(DATA, name + ".txt")) for name in ("H", "H05", "optimalH")}


def main():
    sys.path.insert(0, ROOT)
    from oracle.pyoracle import Oracle, Ref
    o = Oracle()
    ans = answers(Ref(), o, load_matrices(o))
    np.savez_compressed(OUT, **ans)
    print("wrote %d arrays to %s" % (len(ans), os.path.relpath(OUT, ROOT)))


if __name__ == "__main__":
    main()
