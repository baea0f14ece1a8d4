"""CPU: oracle restatement vs the real reference.  The reference's answers are stored in tests/golden/ref_answers.npz
(written by oracle/make_golden_vs_ref.py from the reference compiled as-is, oracle/_ref); where that library is built,
the live reference is asked the same questions and must give the stored answers."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import make_golden_vs_ref as G  # noqa: E402


def _equal(got, want):
    assert set(got) <= set(want)
    for k, v in got.items():
        assert v.shape == want[k].shape and (v == want[k]).all(), k


@pytest.fixture(scope="module")
def ref_answers(oracle, matrices):
    from oracle.pyoracle import Ref, ref_available, build
    with np.load(G.OUT) as z:
        stored = {k: z[k] for k in z.files}
    build()
    if ref_available():
        live = G.answers(Ref(), oracle, matrices)
        assert set(live) == set(stored)
        _equal(live, stored)
    return stored


def test_parse_and_generators(oracle, ref_answers):
    got = G.parse_and_generators(oracle, oracle)
    _equal(got, ref_answers)
    assert got["G_optimalH_ok"] and not got["G_bad_ok"]
    assert got["is_codeword"].all() and not got["is_codeword_flipped"]


def test_admm_matrix_identical(oracle, ref_answers, matrices):
    _equal(G.admm_matrices(oracle, matrices), ref_answers)


@pytest.mark.parametrize("snr", G.FRESH_SNRS)
def test_decoders_fresh_frames(oracle, ref_answers, matrices, snr):
    _equal(G.fresh_frames(oracle, oracle, matrices, snr), ref_answers)


def test_experiment_counts(oracle, ref_answers, matrices):
    _equal(G.experiment_counts(oracle, oracle, matrices), ref_answers)
