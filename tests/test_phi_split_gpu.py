"""The one-series phi of the fused fixed-work sum-product sweeps (bp_core.inc: Dom<float>::phi_small / phi_large, BpPass::word_c /
word_v with SPLIT; the split:: instances, which a fixed-work handle runs by default): a wavefront whose groups have all
latched and whose evaluating lanes all lie at or above 2 (variable side) or at or below 1 (check side) evaluates one of phi's two
series, the one max(ps, pl) would pick.  Nothing may change: the device compares the series with phi on every non-negative fp32
bit pattern, and every output and device counter of such a decoder equals that of one created under
ACG_BP_NO_PHISPLIT=1 (read when a handle is created), for the three build-time instances of the default SPEC_CODES and for the
generic instance (ACG_BP_NO_SPEC=1).  The threshold batches are tests/phi_split_cases.py's: units that are uniform but for one
lane, on either side.  The message words themselves are compared through acg_ldpc_debug_bp_trace, whose dump comes, under
ACG_BP_TRACE_SAT=1 / 2, from the debug twins of the fixed-work instance without and with the split.  (The Monte-Carlo launches of a
handle and the generic instance at 64 lanes have no split: there both sides run the same kernel.)  Run with `-m gpu` on an MI355X."""
import contextlib
import functools
import os

import numpy as np
import pytest

import acg_alp_ldpc_amd as A
from phi_split_cases import END_SNR, check_batch, variable_batch
from satrows_cases import end_case_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# instance -> (matrix, generic instance?)
ENTRIES = {"H05_L32": ("H05", False), "H_L64": ("H", False), "optimalH_L32": ("optimalH", False), "sat_H05": ("H05", True)}
SNRS = (-3.0, -2.0, 2.0)
FRAMES = (1, 7, 2003)      # 7: less than one chunk of 8 frames; 2003: odd, the last wavefront runs with one empty half
MAX_ITERS = (0, 1, 2, 50)


@contextlib.contextmanager
def switches(**sw):
    names = ("ACG_BP_NO_SPEC", "ACG_BP_NO_PHISPLIT", "ACG_BP_NO_FREEZE", "ACG_BP_NO_PHIMEMO")
    old = {k: os.environ.pop(k, None) for k in names}
    for k, on in sw.items():
        if on:
            os.environ[k] = "1"
    try:
        yield
    finally:
        for k in names:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def decoder(H, generic, split, max_iter=50, no_memo=False):
    d = A.BeliefPropagationDecoder(max_iter, early_exit=False)
    with switches(ACG_BP_NO_SPEC=generic, ACG_BP_NO_PHISPLIT=not split, ACG_BP_NO_PHIMEMO=no_memo):
        text = d.describe(H)
    return d, text


def pair(name, H, generic, max_iter=50, no_memo=False):
    on, t_on = decoder(H, generic, True, max_iter, no_memo)
    off, t_off = decoder(H, generic, False, max_iter, no_memo)
    spec = " spec=" + ("0" if generic else name)
    assert " phi_split=1 " in t_on and " phi_split=0 " in t_off and t_on.endswith(spec) and t_off.endswith(spec), (t_on, t_off)
    return on, off


@functools.lru_cache(maxsize=None)
def make_entry(name):
    """per instance: name, H, generic?, codewords, per SNR the symbols of the largest batch, the end-case batches; made once"""
    from oracle.pyoracle import Oracle
    matrix, generic = ENTRIES[name]
    Hm = Oracle().read_pcm(os.path.join(ROOT, "data", matrix + ".txt"))
    H = A.ParityCheckMatrix(Hm)
    G, ok = H.get_orthogonal()
    assert ok
    cws = A.gen_random_codewords(G, 64, 1717)
    y = {snr: A.transmit_frames(cws[np.arange(max(FRAMES)) % len(cws)], snr) for snr in SNRS}
    d = A.BeliefPropagationDecoder(50, early_exit=False)
    L = d.layout(H)["lanes_per_frame"]
    d.close()
    yv, s, values = variable_batch(Hm, L)
    cb = check_batch(Hm, device_phi)
    print("%s: %d lanes per frame; variable side: variable %d of pass 0 takes %s" % (name, L, s, [float(v) for v in values]))
    if cb is not None:
        print("%s: check side: degree-1 variable %d, (wanted sum, LLR, exact) = %s" % (name, cb[1], [(float(w), float(x), e) for w, x, e in cb[2]]))
        # the threshold itself and its neighbour above, which decide the compare's direction, are met to the bit
        assert cb[2][0][2] and cb[2][1][2], cb[2]
    return name, H, generic, cws, y, (yv, end_case_batch(Hm.shape[1])), (cb[0] if cb is not None else None), Hm


@pytest.fixture(scope="module", params=sorted(ENTRIES))
def entry(request):
    return make_entry(request.param)


def device_phi(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros(3 * x.size, dtype=np.uint32)
    assert A.lib().acg_ldpc_debug_phi_sat(x.ctypes.data, out.ctypes.data, x.size) == 0
    return out[0::3].copy().view(np.float32).reshape(x.shape)


def same(a, b, *what):
    for k, part in enumerate(("bits", "ok", "iters")):
        assert a[k].tobytes() == b[k].tobytes(), what + (part, int((a[k] != b[k]).sum()))


def test_series_equal_phi_on_every_bit_pattern():
    out = np.zeros(6, dtype=np.uint32)
    assert A.lib().acg_ldpc_debug_phi_split(out.ctypes.data) == 0
    top_small, low_large = out[2:3].view(np.float32)[0], out[3:4].view(np.float32)[0]
    print("one series against phi: %d mismatches (first pattern 0x%08x); largest x with ps >= pl %.9g (0x%08x), smallest x with "
          "pl >= ps %.9g (0x%08x); max(ps, pl) against phi: %d mismatches (first 0x%08x)"
          % (out[0], out[1], top_small, out[2], low_large, out[3], out[4], out[5]))
    assert out[0] == 0 and out[1] == 0xFFFFFFFF, "phi_large on [2, 66) / phi_small on (0, 1] gives other bits than phi"
    assert out[4] == 0 and out[5] == 0xFFFFFFFF, "the full path of a split row gives other bits than phi"
    # between the two either series is right: the thresholds lie outside, with room
    assert 1.0 < low_large <= top_small < 2.0, (low_large, top_small)


def test_the_switches(entry):
    name, H, generic = entry[:3]
    # (the split lives in the instances with the freeze path; without the freeze nothing says that a group has latched)
    for sw, want in ((dict(), 1), (dict(ACG_BP_NO_PHISPLIT=True), 0), (dict(ACG_BP_NO_FREEZE=True), 0)):
        d = A.BeliefPropagationDecoder(50, early_exit=False)
        with switches(ACG_BP_NO_SPEC=generic, **sw):
            assert " phi_split=%d " % want in d.describe(H), (sw, d.describe(H))
        d.close()
    d = A.BeliefPropagationDecoder(50, early_exit=True)   # early exit: the plain instances, which have no split
    with switches():
        assert "phi_split" not in d.describe(H)
    d.close()


def test_outputs_equal_without_the_split(entry):
    name, H, generic, _, y = entry[:5]
    for max_iter in MAX_ITERS:
        on, off = pair(name, H, generic, max_iter)
        for snr in SNRS:
            for frames in FRAMES:
                same(on.decode_batch(H, y[snr][:frames], snr), off.decode_batch(H, y[snr][:frames], snr), name, max_iter, snr, frames)
        on.close()
        off.close()


def test_end_cases_equal_without_the_split(entry):
    name, H, generic, _, _, ends, ycheck = entry[:7]
    for max_iter in MAX_ITERS:
        on, off = pair(name, H, generic, max_iter)
        for k, yend in enumerate(ends):
            for yy in (yend, yend.astype(np.float32)):
                same(on.decode_batch(H, yy, END_SNR), off.decode_batch(H, yy, END_SNR), name, max_iter, "end cases", k, yy.dtype)
        on.close()
        off.close()
        if ycheck is None:
            continue
        for no_memo in (False, True):   # without the memo the rows of the degree-1 variables' checks evaluate phi
            on, off = pair(name, H, generic, max_iter, no_memo)
            same(on.decode_batch(H, ycheck, END_SNR), off.decode_batch(H, ycheck, END_SNR), name, max_iter, "check side", no_memo)
            on.close()
            off.close()


def trace(H, y, snr, iters, sat):
    nf, E = len(y), H.E
    y = np.ascontiguousarray(y, dtype=np.float64)
    c2v, mag, sgn = (np.zeros((nf, E)) for _ in range(3))
    post = np.zeros((nf, H.n))
    old = os.environ.get("ACG_BP_TRACE_SAT")
    os.environ["ACG_BP_TRACE_SAT"] = str(sat)
    try:
        rc = A.lib().acg_ldpc_debug_bp_trace(H._h, y.ctypes.data, nf, float(snr), iters, 0, A.ENGINE_FUSED, 32, c2v.ctypes.data,
                                             mag.ctypes.data, sgn.ctypes.data, post.ctypes.data)
    finally:
        os.environ.pop("ACG_BP_TRACE_SAT", None)
        if old is not None:
            os.environ["ACG_BP_TRACE_SAT"] = old
    assert rc == 0, A.lib().acg_ldpc_last_error()
    return c2v, mag, sgn, post


def test_message_words_equal_without_the_split():
    """the message words after the last sweep, from the debug twins of the fixed-work instance with and without the split (generic
    pass structure, 32 lanes per frame): max_iter 1 has no latched sweep, 2 the first one, 3 and 6 more of them"""
    name, H, generic, _, y, ends, ycheck, _ = make_entry("sat_H05")
    batches = [(y[2.0][:64], 2.0), (y[-2.0][:64], -2.0), (ends[0][:64], END_SNR)] + ([(ycheck[:64], END_SNR)] if ycheck is not None else [])
    for k, (yy, snr) in enumerate(batches):
        for iters in (1, 2, 3, 6):
            a, b = trace(H, yy, snr, iters, 1), trace(H, yy, snr, iters, 2)
            for part, u, v in zip(("c2v", "v2c magnitude", "v2c sign", "posterior"), a, b):
                assert u.tobytes() == v.tobytes(), (k, iters, part, int((u != v).sum()))


def test_freeze_and_monte_carlo_counters_equal(entry):
    name, H, generic, cws, y = entry[:5]
    on, off = pair(name, H, generic)
    assert on.freeze_stats(H) == (0, 0) and off.freeze_stats(H) == (0, 0)   # counting on from here
    for snr in SNRS:
        same(on.decode_batch(H, y[snr], snr), off.decode_batch(H, y[snr], snr), name, snr)
        # the state evolution is deterministic: frames frozen, sweeps not run, store and compare passes, to the unit
        sa, sb = on.freeze_stats(H), off.freeze_stats(H)
        pa, pb = on.freeze_passes(H), off.freeze_passes(H)
        print("%s %+.0f dB: frozen, sweeps not run %s / %s; store, compare passes %s / %s (split on / off)" % (name, snr, sa, sb, pa, pb))
        assert sa == sb and pa == pb, (name, snr)
    for snr in (-2.0, 2.0):
        a = A.run_experiment(on, cws, H, snr, frames=4096, noise="device", seed=17)
        b = A.run_experiment(off, cws, H, snr, frames=4096, noise="device", seed=17)
        va, vb = [int(x) for x in a.as_vector()], [int(x) for x in b.as_vector()]
        assert len(va) == 7 and va == vb and a.total == 4096, (name, snr, va, vb)
    on.close()
    off.close()
