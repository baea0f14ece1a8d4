"""acg_ldpc_mc_run_codes / run_experiment_codes: a batch of parity-check matrices scored in one call on one evaluator.

Every check is an equality of integer counters: with the per-code path (run_experiment on a QPADMMDecoder created for that
code with fast_setup), between chunkings, between shardings.  The codes are H05 as an 8 x 14 protograph of 20 x 20
circulants and single-block mutations of it — what one step of the check-matrix local search produces."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data")

pytestmark = pytest.mark.gpu

INT_FIELDS = ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong", "sum_iters")
FRAMES = 333  # not a multiple of any workgroup, wavefront or tile size
Z, R, C_ = 20, 8, 14
SNR, ITERS, MU = -3.0, 60, 0.5


def ints(r):
    return tuple(getattr(r, f) for f in INT_FIELDS)


def proto_of(H):
    """shift of every Z x Z block, -1 = zero block"""
    P = -np.ones((R, C_), dtype=int)
    for i in range(R):
        for j in range(C_):
            row = H[i * Z, j * Z:(j + 1) * Z]
            if row.any():
                P[i, j] = int(np.argmax(row))
    return P


def dense_of(P):
    H = np.zeros((R * Z, C_ * Z), dtype=np.uint8)
    for i in range(R):
        for j in range(C_):
            if P[i, j] >= 0:
                for k in range(Z):
                    H[i * Z + k, j * Z + (P[i, j] + k) % Z] = 1
    return H


def make_code(A, P):
    H = A.ParityCheckMatrix(dense_of(P))
    G, ok = H.get_orthogonal()
    assert ok, "no generator"
    return H, A.gen_random_codewords(G, 64, 239), H.admm_shape()["e_min"]


@pytest.fixture(scope="module")
def setup():
    """H05 and four mutations: one block removed, one added, one shift changed, one block moved from the heaviest column to
    the lightest"""
    import acg_alp_ldpc_amd as A
    P0 = proto_of(A.read_pcm(os.path.join(DATA, "H05.txt")).dense())
    assert (dense_of(P0) == A.read_pcm(os.path.join(DATA, "H05.txt")).dense()).all()
    present = np.argwhere(P0 >= 0)
    absent = np.argwhere(P0 < 0)
    muts = [P0]
    P = P0.copy()
    P[tuple(present[3])] = -1
    muts.append(P)
    P = P0.copy()
    P[tuple(absent[5])] = 7
    muts.append(P)
    P = P0.copy()
    P[tuple(present[10])] = (P[tuple(present[10])] + 3) % Z
    muts.append(P)
    P = P0.copy()
    weight = (P0 >= 0).sum(axis=0)
    light, heavy = int(np.argmin(weight)), int(np.argmax(weight))
    P[int(np.argmax(P0[:, heavy] >= 0)), heavy] = -1
    P[int(np.argmax(P0[:, light] < 0)), light] = 11
    muts.append(P)
    return [make_code(A, P) for P in muts]


def per_code(A, alpha, code, noise, frames=FRAMES, first_frame=5, seed=11, **kw):
    H, cws, _ = code
    dec = A.QPADMMDecoder(alpha, MU, ITERS, 1e-5, fast_setup=True, **kw)
    r = A.run_experiment(dec, cws, H, SNR, frames=frames, first_frame=first_frame, noise=noise, seed=seed)
    dec.close()
    return r


def safe_alpha(codes):
    """below every code's guard threshold e_min * mu (qp_admm.h:108-114), and the reference's 1.95 where that is"""
    return min(1.95, 0.9 * MU * min(c[2] for c in codes))


@pytest.mark.parametrize("noise", ["host", "device"])
@pytest.mark.parametrize("early_exit", [True, False])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_codes_equal_per_code(setup, prec, early_exit, noise):
    import acg_alp_ldpc_amd as A
    kw = dict(early_exit=early_exit, precision=A.PREC_F64 if prec == "f64" else A.PREC_F32)
    alpha = safe_alpha(setup)
    ev = A.CodesEvaluator(A.QPADMMDecoder(alpha, MU, ITERS, 1e-5, **kw))
    batch = [(H, cws) for H, cws, _ in setup] + [(setup[2][0], setup[2][1])]  # (code 2 twice)
    got = A.run_experiment_codes(ev, batch, SNR, frames=FRAMES, first_frame=5, noise=noise, seed=11)
    assert "mc_codes=single-launch" in ev.describe(), ev.describe()
    assert len(got) == 6
    for k, code in enumerate(setup):
        want = per_code(A, alpha, code, noise, **kw)
        assert ints(got[k]) == ints(want), (k, ints(got[k]), ints(want))
        assert got[k].total == FRAMES
    assert ints(got[5]) == ints(got[2])
    assert all(r.time_sec == got[0].time_sec and r.time_sec > 0 for r in got)
    ev.close()


def check_guard_point(r, frames, raw_hamming):
    """experiment.h:109-120 with (zeros, false) from every decode: nothing correct, every Hamming sum on the wrong side"""
    assert (r.correct, r.pseudo, r.total, r.sum_iters) == (0, 0, frames, 0)
    assert r.sum_hamming_ok == 0 and r.sum_hamming == r.sum_hamming_wrong
    if raw_hamming is not None:
        assert r.sum_hamming == raw_hamming


def test_guard_codes(setup):
    import acg_alp_ldpc_amd as A
    batch = [(H, cws) for H, cws, _ in setup]
    e = [c[2] for c in setup]
    if min(e) < max(e):
        alpha = MU * (min(e) + max(e)) / 2
        for noise in ("host", "device"):
            got = A.run_experiment_codes(A.QPADMMDecoder(alpha, MU, ITERS, 1e-5), batch, SNR, frames=FRAMES, first_frame=5, noise=noise,
                                         seed=11)
            n_guard = 0
            for k, code in enumerate(setup):
                if code[2] * MU <= alpha:
                    n_guard += 1
                    # the raw-channel Hamming sum does not depend on the decoder: the same code below its guard threshold
                    raw = per_code(A, safe_alpha(setup), code, noise).sum_hamming
                    check_guard_point(got[k], FRAMES, raw)
                else:
                    assert ints(got[k]) == ints(per_code(A, alpha, code, noise)), k
            assert 0 < n_guard < len(setup)
    else:  # one e_min for all five: every code is a guard code at mu = 0
        ev = A.CodesEvaluator(A.QPADMMDecoder(1.95, 0.0, ITERS, 1e-5))
        got = ev.run(batch, SNR, frames=FRAMES, first_frame=5, noise="host", seed=11)
        for k, code in enumerate(setup):
            check_guard_point(got[k], FRAMES, per_code(A, safe_alpha(setup), code, "host").sum_hamming)
        ev.close()


def sparsest():
    """one block per column, spread over the rows: block rows of one or two blocks"""
    P = -np.ones((R, C_), dtype=int)
    for j in range(C_):
        P[j % R, j] = (3 * j) % Z
    return P


def densest(A):
    """as many blocks as the workgroup-per-frame kernel still accepts (at most 1024 variables incl. the auxiliary ones of
    qp_admm.h:34-57: 280 + 20 * sum(blocks of a row - 3)), filled row by row"""
    for blocks in range(61, 30, -1):
        P = -np.ones((R, C_), dtype=int)
        for b in range(blocks):
            i, j = b % R, (b // R + b % R) % C_
            P[i, j] = (5 * i + 3 * j) % Z
        H = A.ParityCheckMatrix(dense_of(P))
        if not H.get_orthogonal()[1]:
            continue
        dec = A.QPADMMDecoder(0.1, MU, ITERS, 1e-5, fast_setup=True)
        try:
            d = dec.describe(H)
        except A.LdpcError:  # (refused by every QP-ADMM kernel)
            continue
        finally:
            dec.close()
        if "engine=lds" in d and any("lanes_per_frame=%d " % L in d for L in (128, 192, 256)):
            return P
    raise AssertionError("no dense protograph for the workgroup-per-frame kernel")


def test_launch_groups():
    """the sparsest protograph (160 constraint groups, one- and two-variable checks: the general instance, 2 passes) and the
    densest one (about 1000 variables: 4 passes) cannot share a launch shape: two groups"""
    import acg_alp_ldpc_amd as A
    codes = [make_code(A, sparsest()), make_code(A, densest(A))]
    alpha = min(0.5, safe_alpha(codes))
    ev = A.CodesEvaluator(A.QPADMMDecoder(alpha, MU, ITERS, 1e-5))
    batch = [(codes[0][0], codes[0][1]), (codes[1][0], codes[1][1]), (codes[0][0], codes[0][1])]
    for noise in ("host", "device"):
        got = ev.run(batch, SNR, frames=FRAMES, first_frame=5, noise=noise, seed=11)
        d = ev.describe()
        assert "mc_codes=single-launch" in d and "per_code=0" in d, d
        assert int(d.split("groups=")[1].split()[0]) >= 2, d
        for k, j in enumerate((0, 1, 0)):
            assert ints(got[k]) == ints(per_code(A, alpha, codes[j], noise)), (noise, k)
    ev.close()


def test_chunking(setup, tmp_path):
    """ACG_MC_GRID_BUDGET=500 in a fresh child process: one code per launch (333 frames each) instead of all five — more than
    one chunk, the same counters"""
    import acg_alp_ldpc_amd as A
    alpha = safe_alpha(setup)
    ev = A.CodesEvaluator(A.QPADMMDecoder(alpha, MU, ITERS, 1e-5))
    batch = [(H, cws) for H, cws, _ in setup]
    one = {noise: [ints(r) for r in ev.run(batch, SNR, frames=FRAMES, first_frame=5, noise=noise, seed=11)] for noise in ("host", "device")}
    assert "chunks=1 " in ev.describe(), ev.describe()
    ev.close()
    np.savez(tmp_path / "codes.npz", alpha=alpha, **{"H%d" % k: c[0].dense() for k, c in enumerate(setup)},
             **{"cw%d" % k: c[1] for k, c in enumerate(setup)})
    script = tmp_path / "child.py"
    script.write_text(
        "import json, sys\n"
        "import numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "import acg_alp_ldpc_amd as A\n"
        "z = np.load(sys.argv[1])\n"
        "batch = [(z['H%%d' %% k], z['cw%%d' %% k]) for k in range(5)]\n"
        "ev = A.CodesEvaluator(A.QPADMMDecoder(float(z['alpha']), %r, %r, 1e-5))\n"
        "out = {}\n"
        "for noise in ('host', 'device'):\n"
        "    got = ev.run(batch, %r, frames=%r, first_frame=5, noise=noise, seed=11)\n"
        "    out[noise] = [[getattr(r, f) for f in %r] for r in got]\n"
        "out['describe'] = ev.describe()\n"
        "print(json.dumps(out))\n" % (ROOT, MU, ITERS, SNR, FRAMES, INT_FIELDS))
    import json
    env = dict(os.environ, ACG_MC_GRID_BUDGET="500")
    p = subprocess.run([sys.executable, str(script), str(tmp_path / "codes.npz")], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert int(out["describe"].split("chunks=")[1].split()[0]) > 1, out["describe"]
    for noise in ("host", "device"):
        assert [tuple(r) for r in out[noise]] == one[noise], noise


def test_sharding(setup):
    import acg_alp_ldpc_amd as A
    alpha = safe_alpha(setup)
    ev = A.CodesEvaluator(A.QPADMMDecoder(alpha, MU, ITERS, 1e-5))
    batch = [(H, cws) for H, cws, _ in setup]
    whole = ev.run(batch, SNR, frames=FRAMES, first_frame=0, noise="device", seed=9)
    parts = [ev.run(batch, SNR, frames=f, first_frame=lo, noise="device", seed=9) for lo, f in ((0, 100), (100, 133), (233, 100))]
    for k in range(len(batch)):
        tot = parts[0][k]
        A.merge_exp_results(tot, parts[1][k])
        A.merge_exp_results(tot, parts[2][k])
        assert ints(tot) == ints(whole[k]), k
    ev.close()


def test_fallback_per_code(setup):
    import acg_alp_ldpc_amd as A
    alpha = safe_alpha(setup)
    ev = A.CodesEvaluator(A.QPADMMDecoder(alpha, MU, ITERS, 1e-5, lanes_per_frame=64))
    batch = [(H, cws) for H, cws, _ in setup[:3]]
    for noise in ("host", "device"):
        got = ev.run(batch, SNR, frames=FRAMES, first_frame=5, noise=noise, seed=11)
        assert "mc_codes=per-code" in ev.describe(), ev.describe()
        for k in range(3):
            assert ints(got[k]) == ints(per_code(A, alpha, setup[k], noise, lanes_per_frame=64)), (noise, k)
    ev.close()


def test_one_workgroup_many_codes(setup):
    """7 codes x 3 frames, first as they are (21 virtual frames: one per workgroup, only the first load of a structure), then
    the same 7 repeated until the launch has at least four times as many virtual frames as it can have workgroups
    (min(frames, grid_cap) of them): hand-outs are consecutive, so every workgroup is handed four or more frames that are
    a whole launch's worth of frames apart — each time another entry of the batch, in turn smaller and larger codes — and
    reloads tables, registers and LDS offsets inside its frame loop.  Every row equals the per-code result of its code."""
    import acg_alp_ldpc_amd as A
    alpha = safe_alpha(setup)
    order = (0, 1, 2, 3, 4, 1, 0)
    dec = A.QPADMMDecoder(alpha, MU, ITERS, 1e-5, fast_setup=True)
    grid_cap = max(int(dec.describe(H).split("grid_cap=")[1].split()[0]) for H, _, _ in setup)
    dec.close()
    reps = (4 * grid_cap + 3 * len(order) - 1) // (3 * len(order)) + 1
    assert 3 * len(order) * reps >= 4 * grid_cap and 3 * len(order) * reps <= 65536  # (one chunk: ACG_MC_GRID_BUDGET's default)
    ev = A.CodesEvaluator(A.QPADMMDecoder(alpha, MU, ITERS, 1e-5))
    for noise in ("host", "device"):
        want = {j: ints(per_code(A, alpha, setup[j], noise, frames=3)) for j in set(order)}
        for n_rep in (1, reps):
            batch = [(setup[j][0], setup[j][1]) for j in order] * n_rep
            got = ev.run(batch, SNR, frames=3, first_frame=5, noise=noise, seed=11)
            d = ev.describe()
            assert "mc_codes=single-launch" in d and "chunks=1 " in d and "per_code=0" in d, d
            bad = [k for k, r in enumerate(got) if ints(r) != want[order[k % len(order)]]]
            assert not bad, (noise, n_rep, bad[:10])
    ev.close()


def test_errors(setup):
    import ctypes as C
    import acg_alp_ldpc_amd as A
    from acg_alp_ldpc_amd import _lib
    with pytest.raises(A.LdpcError, match="QP-ADMM"):
        A.CodesEvaluator(A.BeliefPropagationDecoder(10))
    ev = A.CodesEvaluator(A.QPADMMDecoder(safe_alpha(setup), MU, ITERS, 1e-5))
    small = A.ParityCheckMatrix(dense_of(proto_of(setup[0][0].dense()))[:, :260])
    with pytest.raises(A.LdpcError, match="different m or n"):
        ev.run([(setup[0][0], setup[0][1]), (small, None)], SNR, frames=10)
    with pytest.raises(A.LdpcError, match="n_codes"):
        ev.run([], SNR, frames=10)
    # cfgs that disagree (the Python mirror cannot build them): straight through the C ABI
    cfgs = (_lib.McCfg * 2)()
    for k in range(2):
        cfgs[k].frames, cfgs[k].snr, cfgs[k].seed, cfgs[k].noise = 10 + k, SNR, 1, _lib.NOISE_DEVICE_PHILOX
    handles = (C.c_void_p * 2)(setup[0][0]._h.value, setup[1][0]._h.value)
    res = (_lib.McResult * 2)()
    res[0].total = res[1].total = -7
    assert A.lib().acg_ldpc_mc_run_codes(ev._h, handles, 2, cfgs, res) != 0
    assert b"equal in every cfg" in A.lib().acg_ldpc_last_error()
    assert res[0].total == -7 and res[1].total == -7  # nothing ran
    ev.close()
