"""The freeze of the fixed-work fused sum-product kernels (bp_fused_body FREEZE: a latched frame whose message state recurs bit for
bit stops sweeping) changes no result.  Every comparison is between a decoder whose handle was created with the path on and one
created under ACG_BP_NO_FREEZE=1 (the switch is read when a handle is created), both in this process, both with early_exit=False:
bits, ok and iters of every frame and the seven Monte-Carlo counters are equal.  The debug counter shows that the path runs where
it should and only there.  Run with `-m gpu` on an MI355X."""
import contextlib
import os
import re

import numpy as np
import pytest

import acg_alp_ldpc_amd as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNRS = (-3.0, -2.0, 2.0)
ITERS = (0, 1, 2, 5, 50, 120)
FRAMES = (2003, 777)  # two ragged batches of different size on one handle: the groups' slots are reused across launches


@contextlib.contextmanager
def env_no_freeze(off):
    old = os.environ.pop("ACG_BP_NO_FREEZE", None)
    if off:
        os.environ["ACG_BP_NO_FREEZE"] = "1"
    try:
        yield
    finally:
        os.environ.pop("ACG_BP_NO_FREEZE", None)
        if old is not None:
            os.environ["ACG_BP_NO_FREEZE"] = old


def pair(H, max_iter, L):
    """(decoder with the path on, decoder without, describe() of the first); the handles for H exist when this returns"""
    on = A.BeliefPropagationDecoder(max_iter, early_exit=False, lanes_per_frame=L)
    off = A.BeliefPropagationDecoder(max_iter, early_exit=False, lanes_per_frame=L)
    with env_no_freeze(False):
        d_on = on.describe(H)
    with env_no_freeze(True):
        d_off = off.describe(H)
    assert " freeze=1" not in d_off, d_off
    if "kernel=bp_fused_kernel " in d_off:
        assert " freeze=0" in d_off, d_off
    return on, off, d_on


@pytest.fixture(scope="module")
def codes():
    from oracle.pyoracle import Oracle
    o = Oracle()
    out = {}
    for name in ("H05", "H", "optimalH"):
        H = A.ParityCheckMatrix(o.read_pcm(os.path.join(ROOT, "data", name + ".txt")))
        G, ok = H.get_orthogonal()
        assert ok
        cws = A.gen_random_codewords(G, 64, 4245)
        out[name] = (H, cws)
    return out


@pytest.fixture(scope="module")
def symbols(codes):
    """per (matrix, SNR): the symbols of the two batches, made once and left alone"""
    out = {}
    for name, (H, cws) in codes.items():
        for snr in SNRS:
            y = A.transmit_frames(cws[np.arange(sum(FRAMES)) % len(cws)], snr)
            out[name, snr] = (y[:FRAMES[0]], y[FRAMES[0]:])
    return out


def same(a, b, what):
    for k, name in enumerate(("bits", "ok", "iters")):
        assert np.array_equal(a[k], b[k]), (what, name, int((a[k] != b[k]).sum()))


@pytest.mark.parametrize("L", [16, 32, 64])
@pytest.mark.parametrize("name", ["H05", "H", "optimalH"])
def test_freeze_changes_no_result(codes, symbols, name, L):
    H, _ = codes[name]
    for max_iter in ITERS:
        on, off, d_on = pair(H, max_iter, L)
        if name == "H05" and L in (32, 64):
            assert "kernel=bp_fused_kernel " in d_on and " freeze=1 " in d_on, d_on  # the headline's instance and its 64-lane twin
        for snr in SNRS:
            for y in symbols[name, snr]:
                same(on.decode_batch(H, y, snr), off.decode_batch(H, y, snr), (name, L, max_iter, snr, len(y)))
        on.close()
        off.close()


@pytest.mark.parametrize("snr", [-2.0, 2.0])
def test_freeze_monte_carlo_counters(codes, snr):
    H, cws = codes["H05"]
    on, off, d_on = pair(H, 50, 32)
    assert " freeze=1 " in d_on, d_on
    a = A.run_experiment(on, cws, H, snr, frames=20011, noise="device", seed=14)
    b = A.run_experiment(off, cws, H, snr, frames=20011, noise="device", seed=14)
    va, vb = [int(x) for x in a.as_vector()], [int(x) for x in b.as_vector()]
    assert len(va) == 7 and va == vb and a.total == 20011


def test_freeze_knife_edge_frames(codes):
    H, _ = codes["H05"]
    k = np.load(os.path.join(ROOT, "tests", "golden", "bp_knife_edges.npz"))
    for L in (32, 64):
        on, off, d_on = pair(H, 50, L)
        assert " freeze=1 " in d_on, d_on
        for i in range(len(k["snr"])):
            y, snr = np.ascontiguousarray(k["y"][i:i + 1]), float(k["snr"][i])
            got = on.decode_batch(H, y, snr)
            same(got, off.decode_batch(H, y, snr), ("knife", L, i))
            assert got[1][0] == 1 and (got[0][0] == np.unpackbits(k["oracle_bits"][i])[:H.n]).all()


def test_freeze_special_symbols(codes, symbols):
    """0, +-inf, NaN and +-1e30 among the symbols: messages that are +0, +inf or NaN from the first sweep on.  The compare is of
    words, so a NaN state that recurs freezes like any other and one whose payload wanders does not; either way the outputs are
    those of every sweep."""
    H, _ = codes["H05"]
    rng = np.random.default_rng(77)
    y = symbols["H05", -2.0][0].astype(np.float64).copy()
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e30, -1e30])
    hit = rng.random(y.shape) < 0.01
    hit[:200] |= rng.random((200, y.shape[1])) < 0.2     # some frames with many of them
    y[hit] = special[rng.integers(0, len(special), int(hit.sum()))]
    y[200] = 0.0
    y[201] = np.inf
    y[202] = np.nan
    y[203] = 1e30
    y[204] = -1e30
    for L, max_iter in ((32, 50), (64, 50), (32, 120)):
        on, off, d_on = pair(H, max_iter, L)
        assert " freeze=1 " in d_on, d_on
        for yy in (y, y.astype(np.float32)):
            same(on.decode_batch(H, yy, -2.0), off.decode_batch(H, yy, -2.0), ("special", L, max_iter, yy.dtype))


def cadence(d):
    m = re.search(r" freeze_cadence=(\d+),(\d+)", d)
    assert m, d
    return int(m.group(1)), int(m.group(2))


def test_freeze_path_runs(codes, symbols):
    H, _ = codes["H05"]
    # +2 dB, 50 sweeps: every frame has converged by sweep 4 and its state stands still a few sweeps later
    on, off, d_on = pair(H, 50, 32)
    first, period = cadence(d_on)
    assert on.freeze_stats(H) == (0, 0)
    y = symbols["H05", 2.0][0]
    bits, ok, iters = on.decode_batch(H, y, 2.0)
    frozen, skipped = on.freeze_stats(H)
    print("+2 dB: %d of %d frames frozen, %d sweeps not run (%.1f per frame)" % (frozen, len(y), skipped, skipped / len(y)))
    assert frozen > 0.9 * len(y) and frozen <= int(ok.sum())
    # a frame that latched at sweep k is compared first at sweep k + first + period
    assert 0 < skipped <= int(np.maximum(50 - (iters[ok == 1] + first + period), 0).sum())
    # -2 dB: only frames that latched (ok = 1) can be counted, and none of them earlier than the cadence allows
    y = symbols["H05", -2.0][0]
    bits, ok, iters = on.decode_batch(H, y, -2.0)
    frozen, skipped = on.freeze_stats(H)
    print("-2 dB: %d of %d frames frozen (%d ok), %d sweeps not run" % (frozen, len(y), int(ok.sum()), skipped))
    assert 0 < frozen <= int(ok.sum()) < len(y)
    assert skipped <= int(np.maximum(50 - (iters[ok == 1] + first + period), 0).sum())
    # counting off again; the decoder without the path never counts
    assert on.freeze_stats(H, enable=False) == (0, 0)
    on.decode_batch(H, y, -2.0)
    assert on.freeze_stats(H, enable=False) == (0, 0)
    off.freeze_stats(H)
    off.decode_batch(H, y, 2.0)
    assert off.freeze_stats(H) == (0, 0)
    on.close()
    off.close()
    # max_iter <= 2: the first detection only writes, so nothing can freeze
    for max_iter in (0, 1, 2):
        on, off, d_on = pair(H, max_iter, 32)
        on.freeze_stats(H)
        on.decode_batch(H, symbols["H05", 2.0][0], 2.0)
        assert on.freeze_stats(H) == (0, 0), max_iter
        on.close()
        off.close()
