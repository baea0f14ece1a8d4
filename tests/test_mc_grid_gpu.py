"""acg_ldpc_mc_run_grid / run_experiment_grid: the (alpha, mu) loop of qpadmm_params.cpp:64-77 on ONE decoder handle.

Every check is an equality of integer counters: with the per-point path (run_experiment on a decoder created with the
point's own alpha and mu), with the oracle's restatement of the reference's loop, between chunkings, between shardings."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data")

pytestmark = pytest.mark.gpu

INT_FIELDS = ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong", "sum_iters")
FRAMES = 333  # not a multiple of any workgroup, wavefront or tile size


def ints(r):
    return tuple(getattr(r, f) for f in INT_FIELDS)


def product(alphas, mus):
    """alpha-major, like the reference's double loop"""
    a = [x for x in alphas for _ in mus]
    m = [y for _ in alphas for y in mus]
    return a, m


@pytest.fixture(scope="module")
def setup():
    import acg_alp_ldpc_amd as A
    out = {}
    for name in ("H05", "optimalH"):
        H = A.read_pcm(os.path.join(DATA, name + ".txt"))
        G, ok = H.get_orthogonal()
        assert ok
        out[name] = (H, A.gen_random_codewords(G, 64, 239), H.admm_shape()["e_min"])
    return out


def is_guard(e_min, a, m):
    return e_min * m <= a  # qp_admm.h:108-114


def check_guard_point(r, frames, raw_hamming):
    """experiment.h:109-120 with (zeros, false) from every decode: nothing correct, every Hamming sum on the wrong side"""
    assert (r.correct, r.pseudo, r.total, r.sum_iters) == (0, 0, frames, 0)
    assert r.sum_hamming_ok == 0 and r.sum_hamming == r.sum_hamming_wrong
    if raw_hamming is not None:
        assert r.sum_hamming == raw_hamming


@pytest.mark.parametrize("early_exit", [True, False])
@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("name", ["optimalH", "H05"])
def test_grid_equals_per_point(setup, name, prec, early_exit):
    """4 x 4 grid with guard points (alpha = mu = 0, and mu = 0 < alpha among them), host and device noise: every
    non-guard point equals run_experiment on its own decoder in all seven integer fields"""
    import acg_alp_ldpc_amd as A
    H, cws, e_min = setup[name]
    precision = A.PREC_F64 if prec == "f64" else A.PREC_F32
    alphas, mus = product([0.0, 0.6, 1.2, 1.95], [0.0, 0.3, 0.5, 0.9])
    assert is_guard(e_min, 0.0, 0.0) and is_guard(e_min, 0.6, 0.0)
    kw = dict(early_exit=early_exit, precision=precision)
    grid_dec = A.QPADMMDecoder(0.0, 0.0, 60, 1e-5, **kw)  # (its own alpha, mu are ignored: here they are a guard point)
    assert "mc_grid=single-launch" in grid_dec.describe(H)
    for noise in ("host", "device"):
        got = A.run_experiment_grid(grid_dec, cws, H, -3.0, alphas, mus, frames=FRAMES, first_frame=5, noise=noise, seed=11)
        assert len(got) == 16
        raw = None
        n_guard = 0
        for a, m, r in zip(alphas, mus, got):
            if is_guard(e_min, a, m):
                n_guard += 1
                continue
            want = A.run_experiment(A.QPADMMDecoder(a, m, 60, 1e-5, **kw), cws, H, -3.0, frames=FRAMES, first_frame=5, noise=noise,
                                    seed=11)
            assert ints(r) == ints(want), (noise, a, m)
            assert r.total == FRAMES
            raw = want.sum_hamming
        assert 2 <= n_guard < 16
        for a, m, r in zip(alphas, mus, got):
            if is_guard(e_min, a, m):
                check_guard_point(r, FRAMES, raw)
        assert all(r.time_sec == got[0].time_sec and r.time_sec > 0 for r in got)  # the wall time of the whole call
    grid_dec.close()


@pytest.mark.parametrize("noise", ["host", "device"])
def test_chunked_grid_equals_single_chunk(setup, monkeypatch, noise):
    """ACG_MC_GRID_BUDGET (virtual frames per launch) lowered so that the 6 x 6 grid takes many launches — three points per
    launch, then one launch per block of 100 frames and point: the same counters as the single launch"""
    import acg_alp_ldpc_amd as A
    H, cws, e_min = setup["optimalH"]
    alphas, mus = product(np.linspace(0.0, 2.0, 6), np.linspace(0.1, 0.9, 6))
    dec = A.QPADMMDecoder(1.2, 0.55, 80, 1e-5)
    monkeypatch.delenv("ACG_MC_GRID_BUDGET", raising=False)
    one = A.run_experiment_grid(dec, cws, H, -3.0, alphas, mus, frames=FRAMES, noise=noise, seed=3)
    assert any(is_guard(e_min, a, m) for a, m in zip(alphas, mus))
    for budget in ("1000", "100"):
        monkeypatch.setenv("ACG_MC_GRID_BUDGET", budget)
        many = A.run_experiment_grid(dec, cws, H, -3.0, alphas, mus, frames=FRAMES, noise=noise, seed=3)
        assert [ints(r) for r in many] == [ints(r) for r in one], budget
    dec.close()


def test_grid_equals_reference_semantics(setup, oracle):
    """host noise, mt19937(239) codewords, the 3 x 3 sub-grid of test_drivers.py::test_grid_search_driver_matches_oracle at
    200 frames and max_iter 1000: all six counters of the reference's loop, guard points included"""
    import acg_alp_ldpc_amd as A
    Hm = oracle.read_pcm(os.path.join(DATA, "optimalH.txt"))
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 239, 200)
    H = A.ParityCheckMatrix(Hm)
    alphas, mus = product([0.8, 1.2, 1.6], [0.3, 0.5, 0.7])
    dec = A.QPADMMDecoder(1.2, 0.55, 1000, 1e-5)
    got = A.run_experiment_grid(dec, cws, H, -3.0, alphas, mus, noise="host")
    keys = ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong")
    n_guard = 0
    for a, m, r in zip(alphas, mus, got):
        want = oracle.experiment("qpadmm", Hm, cws, -3.0, 1000, a, m, 1e-5)
        assert tuple(getattr(r, k) for k in keys) == tuple(want[k] for k in keys), (a, m)
        n_guard += is_guard(4.0, a, m)
    assert n_guard == 2
    dec.close()


@pytest.mark.parametrize("variant", ["lanes64", "streamed", "budget0"])
def test_other_engines_run_the_points_in_turn(setup, variant):
    """decoders without a grid kernel: the same entry point, the same per-point results (2 x 3 grid, one guard point)"""
    import acg_alp_ldpc_amd as A
    H, cws, e_min = setup["optimalH"]
    kw, iters = {"lanes64": (dict(lanes_per_frame=64), 50), "streamed": (dict(engine=A.ENGINE_STREAMED), 50),
                 "budget0": ({}, 0)}[variant]
    alphas, mus = product([0.9, 1.6], [0.3, 0.5, 0.7])
    assert sum(is_guard(e_min, a, m) for a, m in zip(alphas, mus)) == 1
    dec = A.QPADMMDecoder(1.95, 0.5, iters, 1e-5, **kw)
    assert "mc_grid=per-point" in dec.describe(H)
    for noise in ("host", "device"):
        got = A.run_experiment_grid(dec, cws, H, -3.0, alphas, mus, frames=FRAMES, noise=noise, seed=5)
        for a, m, r in zip(alphas, mus, got):
            if is_guard(e_min, a, m):
                check_guard_point(r, FRAMES, got[0].sum_hamming)
                continue
            want = A.run_experiment(A.QPADMMDecoder(a, m, iters, 1e-5, **kw), cws, H, -3.0, frames=FRAMES, noise=noise, seed=5)
            assert ints(r) == ints(want), (noise, a, m)
        # the handle is its own again afterwards
        own = A.run_experiment(dec, cws, H, -3.0, frames=FRAMES, noise=noise, seed=5)
        want = A.run_experiment(A.QPADMMDecoder(1.95, 0.5, iters, 1e-5, **kw), cws, H, -3.0, frames=FRAMES, noise=noise, seed=5)
        assert ints(own) == ints(want)
    dec.close()


def test_sharded_grid_merges_to_the_unsharded_one(setup):
    import acg_alp_ldpc_amd as A
    H, cws, _ = setup["H05"]
    alphas, mus = product([0.5, 1.95, 2.5], [0.2, 0.5])
    dec = A.QPADMMDecoder(1.95, 0.5, 100, 1e-5)
    whole = A.run_experiment_grid(dec, cws, H, -2.0, alphas, mus, frames=1001, noise="device", seed=9)
    lo = A.run_experiment_grid(dec, cws, H, -2.0, alphas, mus, frames=400, first_frame=0, noise="device", seed=9)
    hi = A.run_experiment_grid(dec, cws, H, -2.0, alphas, mus, frames=601, first_frame=400, noise="device", seed=9)
    for w, a, b in zip(whole, lo, hi):
        A.merge_exp_results(a, b)
        assert ints(a) == ints(w)
    dec.close()


def test_refusals(setup):
    import acg_alp_ldpc_amd as A
    H, cws, _ = setup["H05"]
    with pytest.raises(A.LdpcError, match="QP-ADMM"):
        A.run_experiment_grid(A.BeliefPropagationDecoder(10), cws, H, -2.0, [1.0], [0.5], frames=10)
    dec = A.QPADMMDecoder(1.95, 0.5, 10, 1e-5)
    with pytest.raises(A.LdpcError, match="n_points"):
        A.run_experiment_grid(dec, cws, H, -2.0, [], [], frames=10)
    with pytest.raises(A.LdpcError, match="same length"):
        A.run_experiment_grid(dec, cws, H, -2.0, [1.0, 2.0], [0.5], frames=10)
    dec.close()
