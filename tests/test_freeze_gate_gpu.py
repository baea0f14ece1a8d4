"""The checksum gate in front of the freeze path's compare (bp_fused_body FREEZE): a detection loads its snapshot and compares only
when every lane's sum of its words equals the sum taken at the snapshot, and otherwise only writes the new one.  The gate is a
necessary condition for equality and the compare is unchanged, so a handle with the gate freezes every frame at the sweep at which
a handle created under ACG_BP_FREEZE_NO_GATE=1 (compare at every detection behind a group's first) freezes it.  The switches are
read when a handle is created; all handles live in this process.  H05, 50 sweeps, the two ragged batches of test_freeze_gpu.py.
Run with `-m gpu` on an MI355X."""
import contextlib
import os
import re

import numpy as np
import pytest

import acg_alp_ldpc_amd as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNRS = (-3.0, -2.0, 2.0)
FRAMES = (2003, 777)
MAX_ITER = 50
SWITCHES = ("ACG_BP_NO_FREEZE", "ACG_BP_FREEZE_NO_GATE", "ACG_BP_FREEZE_CADENCE")
# tools/freeze_census.cpp, 1000 frames per SNR at -3, -2 and +2 dB, every cadence of its grid: no detection that passed the gate
# failed its compare (0 collisions of the sum among 1118 ... 13181 rejected detections per cadence and SNR).  The allowance for
# compare passes beyond the frozen frames is that count scaled to the batch, times 4, plus 2:
#   (0 collisions / 1000 frames) * 2780 frames * 4 + 2 = 2
# tests/test_freeze_gate_census.py holds the census itself to the same bound.
CENSUS_COLLISIONS, CENSUS_FRAMES = 0, 1000


def allowance(frames):
    return int(np.ceil(CENSUS_COLLISIONS / CENSUS_FRAMES * frames * 4)) + 2


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update({k: v for k, v in kw.items() if v is not None})
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def decoder(H, L, max_iter=MAX_ITER, **switches):
    """(decoder, describe()) with its handle for H created under the switches"""
    d = A.BeliefPropagationDecoder(max_iter, early_exit=False, lanes_per_frame=L)
    with env(**switches):
        text = d.describe(H)
    return d, text


def cadence(text):
    m = re.search(r" freeze=1 freeze_cadence=(\d+),(\d+) freeze_gate=([01])", text)
    assert m, text
    return int(m.group(1)), int(m.group(2)), int(m.group(3))


def gate_pair(H, L, max_iter=MAX_ITER):
    """gate on and gate off with the built-in first snapshot and a compare every sweep: the detections of a frame are then
    the sweeps from latch + first to the sweep it freezes at (or the last but one), which the counters below are held to"""
    probe, text = decoder(H, L, max_iter)
    first, _, gate = cadence(text)
    assert gate == 1, text
    probe.close()
    cad = "%d,1" % first
    on, t_on = decoder(H, L, max_iter, ACG_BP_FREEZE_CADENCE=cad)
    off, t_off = decoder(H, L, max_iter, ACG_BP_FREEZE_CADENCE=cad, ACG_BP_FREEZE_NO_GATE="1")
    assert cadence(t_on) == (first, 1, 1) and cadence(t_off) == (first, 1, 0), (t_on, t_off)
    return on, off, first


@pytest.fixture(scope="module")
def code():
    from oracle.pyoracle import Oracle
    H = A.ParityCheckMatrix(Oracle().read_pcm(os.path.join(ROOT, "data", "H05.txt")))
    G, ok = H.get_orthogonal()
    assert ok
    return H, A.gen_random_codewords(G, 64, 4245)


@pytest.fixture(scope="module")
def symbols(code):
    """per SNR the symbols of the two batches, made once and left alone"""
    H, cws = code
    out = {}
    for snr in SNRS:
        y = A.transmit_frames(cws[np.arange(sum(FRAMES)) % len(cws)], snr)
        out[snr] = (y[:FRAMES[0]], y[FRAMES[0]:])
    return out


def same(a, b, what):
    for k, name in enumerate(("bits", "ok", "iters")):
        assert np.array_equal(a[k], b[k]), (what, name, int((a[k] != b[k]).sum()))


def detections(ok, iters, first, frozen, skipped):
    """every detection of a batch at period 1: a frame latched at sweep k is detected after the sweeps k + first ... 49, a frozen one
    only up to the sweep it froze at, s, and the counter holds the sum of 50 - s; the first of a frame only writes"""
    k = iters[ok == 1].astype(np.int64)
    firsts = int((k + first < MAX_ITER).sum())
    total = int(np.maximum(MAX_ITER - k - first, 0).sum()) - (skipped - frozen)
    return firsts, total


@pytest.mark.parametrize("L", [32, 64])
def test_gate_changes_nothing(code, symbols, L):
    H, _ = code
    on, off, first = gate_pair(H, L)
    assert on.freeze_stats(H) == (0, 0) and off.freeze_stats(H) == (0, 0)
    assert on.freeze_passes(H) == (0, 0) and off.freeze_passes(H) == (0, 0)
    for snr in SNRS:
        for y in symbols[snr]:
            a, b = on.decode_batch(H, y, snr), off.decode_batch(H, y, snr)
            same(a, b, (L, snr, len(y)))
            sa, sb = on.freeze_stats(H), off.freeze_stats(H)
            pa, pb = on.freeze_passes(H), off.freeze_passes(H)
            print("L=%d %+.0f dB %d frames: frozen, sweeps not run %s / %s; store, compare passes %s / %s (gate on / off)"
                  % (L, snr, len(y), sa, sb, pa, pb))
            assert sa == sb, (L, snr, len(y))
            frozen, skipped = sa
            firsts, total = detections(a[1], a[2], first, frozen, skipped)
            # gate off: the first detection of a frame writes, every later one loads and compares
            assert pb == (firsts, total - firsts), (L, snr, len(y))
            # gate on: the same detections; of those behind the first, only the ones that can freeze load and compare
            assert sum(pa) == total, (L, snr, len(y))
            assert frozen <= pa[1] <= frozen + allowance(sum(FRAMES)), (L, snr, len(y))
    on.close()
    off.close()


@pytest.mark.parametrize("snr", [-2.0, 2.0])
def test_gate_monte_carlo_counters(code, snr):
    H, cws = code
    on, off, _ = gate_pair(H, 32)
    a = A.run_experiment(on, cws, H, snr, frames=20011, noise="device", seed=14)
    b = A.run_experiment(off, cws, H, snr, frames=20011, noise="device", seed=14)
    va, vb = [int(x) for x in a.as_vector()], [int(x) for x in b.as_vector()]
    assert len(va) == 7 and va == vb and a.total == 20011
    on.close()
    off.close()


def test_gate_special_symbols(code, symbols):
    """0, +-inf, NaN and +-1e30 among the symbols (the mix of test_freeze_special_symbols).  The sum and the compare are of words:
    a NaN whose payload wanders changes its lane's sum or fails the compare, so its frame keeps sweeping; one that recurs bit for
    bit may freeze.  Either way the outputs are those of every sweep: gate on against the freeze off."""
    H, _ = code
    rng = np.random.default_rng(77)
    y = symbols[-2.0][0].astype(np.float64).copy()
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e30, -1e30])
    hit = rng.random(y.shape) < 0.01
    hit[:200] |= rng.random((200, y.shape[1])) < 0.2     # some frames with many of them
    y[hit] = special[rng.integers(0, len(special), int(hit.sum()))]
    y[200] = 0.0
    y[201] = np.inf
    y[202] = np.nan
    y[203] = 1e30
    y[204] = -1e30
    for L in (32, 64):
        on, t_on = decoder(H, L)
        off, t_off = decoder(H, L, ACG_BP_NO_FREEZE="1")
        assert cadence(t_on)[2] == 1 and " freeze=0" in t_off, (t_on, t_off)
        on.freeze_stats(H)
        for yy in (y, y.astype(np.float32)):
            same(on.decode_batch(H, yy, -2.0), off.decode_batch(H, yy, -2.0), ("special", L, yy.dtype))
            frozen, _ = on.freeze_stats(H)
            stores, compares = on.freeze_passes(H)
            assert 0 < frozen <= compares and stores > 0, (L, frozen, stores, compares)
        on.close()
        off.close()


@pytest.mark.parametrize("max_iter", [0, 1, 2])
def test_gate_counts_nothing_where_nothing_is_due(code, symbols, max_iter):
    H, _ = code
    for L in (32, 64):
        on, off, _ = gate_pair(H, L, max_iter)
        for d in (on, off):
            d.freeze_stats(H)
            for y in symbols[2.0]:
                d.decode_batch(H, y, 2.0)
            assert d.freeze_stats(H) == (0, 0) and d.freeze_passes(H) == (0, 0), (L, max_iter)
            d.close()


def test_gate_counts_only_while_counting(code, symbols):
    H, _ = code
    on, _ = decoder(H, 32)
    y = symbols[2.0][1]
    on.decode_batch(H, y, 2.0)                       # counting was never asked for
    assert on.freeze_passes(H) == (0, 0)
    on.freeze_stats(H)
    on.decode_batch(H, y, 2.0)
    stores, compares = on.freeze_passes(H)
    assert stores > 0 and compares > 0
    assert on.freeze_passes(H) == (0, 0)             # read and cleared
    on.freeze_stats(H, enable=False)
    on.decode_batch(H, y, 2.0)
    assert on.freeze_passes(H) == (0, 0)
    on.close()
