"""GPU: the quantiser grid of the fixed-point layered min-sum engine — acg_ldpc_mc_run_quants / run_experiment_quants, frames of
different quantisers in one launch of bp_layered_q_kernel's grid form — against (1) the restatement alone
(quant_grid_cases.ref_counters: host-noise symbols, layered_q_ref, mc_detail_ref) and (2) the per-point path it replaces, one
QuantizedMinSumDecoder and one run_experiment per quantiser.  Every assertion is an integer equality.  Codes, SNRs and
iteration counts are those of tests/layered_q_cases.py, the points those of tests/quant_grid_cases.py (tests/test_quant_grid.py
asserts on the CPU that the restatement tells them apart).  The handle's own quantiser is `saturating` throughout: a kernel
that read it instead of the table decodes next to nothing."""
import os
import subprocess

import numpy as np
import pytest

import layered_q_cases as Q
import quant_grid_cases as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data")
OWN = Q.QUANTS["saturating"]

# frames of test 1 per case: 333 where nothing else decides; the restatement of the 3000-variable code costs a second per
# 25 frames and point on the CPU, so it gets 111 — still more virtual frames (888) than a launch at L = 1024 has workgroups
FRAMES_1 = {"H05": G.FRAMES, "qc4x24z27": G.FRAMES, "qc2x10z300": 111, "diag10": G.FRAMES}


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


def _dec(A, it, L=0, ee=True, quant=OWN):
    return A.QuantizedMinSumDecoder(it, quant=A.QuantConfig(*quant), lanes_per_frame=L, early_exit=ee)


def _grid(A, dec, c, quants, frames, first=G.FIRST, noise="host", seed=1, cws="case"):
    cws = G.case_words(c) if isinstance(cws, str) else cws
    return A.run_experiment_quants(dec, cws, c.H, c.snr, quants, frames=frames, first_frame=first, noise=noise, seed=seed)


# ----------------------------------------------------------------------------------------------- 1. grid = restatement
@pytest.mark.parametrize("name", ["H05", "qc4x24z27", "qc2x10z300", "diag10"])
def test_grid_equals_restatement(A, name):
    """host noise, first_frame 5, random codewords where the case has them; lanes_per_frame 0, 64 and 1024, early exit and fixed
    work: all seven counters of every point are the restatement's"""
    c = Q.case(A, name)
    F = FRAMES_1[name]
    cws = G.case_words(c)
    want = [G.ref_counters(c, q, G.FIRST, F, cws) for q in G.LIST]
    for L in (0, 64, 1024):
        for ee in (True, False):
            dec = _dec(A, c.iters, L, ee)
            try:
                got = [G.counters(r) for r in _grid(A, dec, c, G.LIST, F)]
            finally:
                dec.close()
            print(name, L, ee, got)
            assert got == want, (name, L, ee, [(k, g, w) for k, g, w in zip(G.NAMES, got, want) if g != w])


# ------------------------------------------------------------------------------------------- 2. grid = the per-point path
@pytest.mark.parametrize("name", ["H05", "qc2x10z300"])
def test_grid_equals_per_point_path(A, name):
    """device noise: every point equals run_experiment on a QuantizedMinSumDecoder created with that point's quantiser, same
    seed; time_sec is one value for all points, kernel_ms positive"""
    c = Q.case(A, name)
    first, seed = (1 << 33) + 5, 3
    cws = G.case_words(c)
    dec = _dec(A, c.iters)
    try:
        got = _grid(A, dec, c, G.LIST, G.FRAMES, first, "device", seed)
        assert "mc_quants=single-launch" in dec.describe(c.H)
    finally:
        dec.close()
    assert len(got) == len(G.LIST)
    for k, q in enumerate(G.LIST):
        one = _dec(A, c.iters, quant=q)
        try:
            want = A.run_experiment(one, cws, c.H, c.snr, frames=G.FRAMES, first_frame=first, noise="device", seed=seed)
        finally:
            one.close()
        assert G.counters(got[k]) == G.counters(want), (name, G.NAMES[k], got[k], want)
    assert len({r.time_sec for r in got}) == 1 and got[0].time_sec > 0
    assert all(r.kernel_ms > 0 for r in got)
    assert 0 < got[0].correct < G.FRAMES and len({r.correct for r in got}) >= 3


# ------------------------------------------------------------------------------------------------- 3. chunks and shards
@pytest.mark.parametrize("noise", ["host", "device"])
def test_grid_chunking_and_sharding(A, monkeypatch, noise):
    """ACG_MC_GRID_BUDGET = 1000: three points per launch; = 100: one point per block of 100 frames (100, 100, 100, 33) — the
    counters of the single launch.  Two shards of 200 + 133 frames merged per point are the whole."""
    c = Q.case(A, "H05")
    monkeypatch.delenv("ACG_MC_GRID_BUDGET", raising=False)
    dec = _dec(A, c.iters)
    try:
        whole = [G.counters(r) for r in _grid(A, dec, c, G.LIST, G.FRAMES, noise=noise, seed=5)]
        if noise == "host":
            assert whole == [G.ref_counters(c, q, G.FIRST, G.FRAMES, G.case_words(c)) for q in G.LIST]
        for budget in ("1000", "100"):
            monkeypatch.setenv("ACG_MC_GRID_BUDGET", budget)
            got = [G.counters(r) for r in _grid(A, dec, c, G.LIST, G.FRAMES, noise=noise, seed=5)]
            assert got == whole, (noise, budget)
        monkeypatch.delenv("ACG_MC_GRID_BUDGET")
        lo = _grid(A, dec, c, G.LIST, 200, G.FIRST, noise, 5)
        hi = _grid(A, dec, c, G.LIST, 133, G.FIRST + 200, noise, 5)
        merged = [G.counters(A.merge_exp_results(a, b)) for a, b in zip(lo, hi)]
        assert merged == whole, noise
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------------- 4. edge cases
def test_grid_edge_cases(A):
    """max_iter = 0 (every frame fails, 0 iterations, the same launch path); frames = 0; one point; 1 frame x 8 points — fewer
    virtual frames than workgroups"""
    c = Q.case(A, "H05")
    cws = G.case_words(c)
    dec0 = _dec(A, 0)
    try:
        got = _grid(A, dec0, c, G.LIST, G.FRAMES)
        for k, r in enumerate(got):
            assert (r.total, r.correct, r.pseudo, r.sum_iters) == (G.FRAMES, 0, 0, 0), (k, r)
            assert G.counters(r) == G.ref_counters(c, G.LIST[k], G.FIRST, G.FRAMES, cws, it=0)
            assert r.sum_hamming == r.sum_hamming_wrong > 0
    finally:
        dec0.close()
    dec = _dec(A, c.iters)
    try:
        none = _grid(A, dec, c, G.LIST, 0)
        assert len(none) == len(G.LIST) and all(G.counters(r) == (0,) * 7 and r.kernel_ms == 0 for r in none)
        one = _grid(A, dec, c, [G.POINTS["step 0.3"]], G.FRAMES)
        assert [G.counters(r) for r in one] == [G.ref_counters(c, G.POINTS["step 0.3"], G.FIRST, G.FRAMES, cws)]
        few = _grid(A, dec, c, G.LIST, 1, first=11)
        assert [G.counters(r) for r in few] == [G.ref_counters(c, q, 11, 1, cws) for q in G.LIST]
        assert dec.layout(c.H)["grid_blocks"] > len(G.LIST)
    finally:
        dec.close()


# ---------------------------------------------------------------------------------------------------------- 5. refusals
def test_grid_refusals(A):
    """a MinSumDecoder handle through the C ABI; an invalid quantiser at index 3 of 5 — the message names the index and the rule;
    res stays as it was; after each, a valid call on the same handle returns the right counters"""
    import ctypes as C
    c = Q.case(A, "H05")
    cws = G.case_words(c)
    L = A.lib()
    cfg = A._lib.McCfg()
    cfg.frames, cfg.first_frame, cfg.snr, cfg.seed, cfg.noise = 64, G.FIRST, c.snr, 1, A._lib.NOISE_HOST_MT19937
    ms = A.MinSumDecoder(c.iters)
    try:
        h, _ = ms.handle(c.H)
        res = (A._lib.McResult * 2)()
        res[0].total = res[1].total = -7
        rc = L.acg_ldpc_mc_run_quants(h, C.byref(cfg), A.quant_structs(G.LIST[:2]), 2, res)
        msg = L.acg_ldpc_last_error().decode()
        assert rc != 0 and "acg_ldpc_decoder_create_quantized" in msg, (rc, msg)
        assert (res[0].total, res[1].total) == (-7, -7)
        plain = A.run_experiment(ms, cws, c.H, c.snr, frames=64, first_frame=G.FIRST)      # the handle still works
        assert plain.total == 64 and plain.correct > 0
    finally:
        ms.close()
    dec = _dec(A, c.iters)
    try:
        want = [G.ref_counters(c, q, G.FIRST, G.FRAMES, cws) for q in G.LIST[:3]]
        assert [G.counters(r) for r in _grid(A, dec, c, G.LIST[:3], G.FRAMES)] == want
        bad = list(G.LIST[:5])
        bad[3] = (0.5, 6, 9, 12, 1, 0, 1)                                                 # msg_bits 9
        with pytest.raises(A.LdpcError, match=r"quants\[3\].*invalid quantiser: msg_bits"):
            _grid(A, dec, c, bad, G.FRAMES)
        h, _ = dec.handle(c.H)
        res = (A._lib.McResult * 5)()
        for r in res:
            r.total = -7
        assert L.acg_ldpc_mc_run_quants(h, C.byref(cfg), A.quant_structs(bad), 5, res) != 0
        assert "quants[3]" in L.acg_ldpc_last_error().decode() and all(r.total == -7 for r in res)
        cfg_bad = A._lib.McCfg()
        cfg_bad.frames = -1
        assert L.acg_ldpc_mc_run_quants(h, C.byref(cfg_bad), A.quant_structs(G.LIST), len(G.LIST), res) != 0
        assert "bad mc cfg" in L.acg_ldpc_last_error().decode() and all(r.total == -7 for r in res)
        with pytest.raises(A.LdpcError, match="QP-ADMM"):                                 # (the parameter grid still refuses it)
            A.run_experiment_grid(dec, None, c.H, c.snr, [1.0], [0.5], frames=64, noise="device")
        assert [G.counters(r) for r in _grid(A, dec, c, G.LIST[:3], G.FRAMES)] == want
        assert "mc_quants=single-launch" in dec.describe(c.H)
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------------------ 6. driver
def test_quant_sweep_driver(A):
    """acg_quant_sweep on H05 + G05: ch_bits {6, 9} x post_bits {8, 10} x offset {0, 1}; ch_bits 9 over post_bits 8 is invalid,
    so two of the eight points are dropped and counted on stderr; the six CSV rows are run_experiment_quants' figures"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "drivers")], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "tools", "drivers", "bin", "acg_quant_sweep")
    frames, iters, snr = 200, 15, -2.0
    r = subprocess.run([exe, "--H", os.path.join(DATA, "H05.txt"), "--G", os.path.join(DATA, "G05.txt"), "--snr", str(snr),
                        "--tests", str(frames), "--iters", str(iters), "--lanes", "64", "--noise", "host",
                        "--ch-bits", "6,9", "--post-bits", "8,10", "--offset", "0,1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "points=6 dropped=2" in r.stderr, r.stderr
    pts = [(0.5, ch, 6, po, 1, 0, of) for ch in (6, 9) for po in (8, 10) for of in (0, 1) if ch <= po]
    assert len(pts) == 6
    H = A.read_pcm(os.path.join(DATA, "H05.txt"))
    Gm = A.read_pcm(os.path.join(DATA, "G05.txt")).dense()
    cws = A.gen_random_codewords(Gm, frames, 239)
    dec = _dec(A, iters, 64)
    try:
        want = A.run_experiment_quants(dec, cws, H, snr, pts, frames=frames, noise="host", seed=1)
    finally:
        dec.close()
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "llr_step,ch_bits,msg_bits,post_bits,scale_num,scale_shift,offset,fer,pseudo_rate,mean_iters"
    assert len(lines) == 7
    for line, q, w in zip(lines[1:], pts, want):
        v = line.split(",")
        assert (float(v[0]),) + tuple(int(x) for x in v[1:7]) == q, line
        assert v[7:] == ["%.12f" % w.FER(), "%.12f" % (w.pseudo / w.total), "%.12f" % (w.sum_iters / w.total)], (line, w)
    assert len({l.split(",")[7] for l in lines[1:]}) >= 2                                  # (the points differ)
