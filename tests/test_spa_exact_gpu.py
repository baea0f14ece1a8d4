"""GPU: every flooding SUM-PRODUCT kernel against the numpy restatement of its own storage type (tests/spa_ref.py), EXACTLY.

test_gpu_parity.py ties these kernels to the reference (hard outputs against the 80-bit oracle, soft messages within a
tolerance); this file ties them to themselves: apart from phi every operation of a sweep is an IEEE add, a compare or a bit
operation in a fixed order, and phi is a pure function of its input bits that the library exports (acg_ldpc_debug_phi_sat for
Dom<float>::phi, acg_ldpc_debug_phi(f64 = 1) for phi_f).  The restatement is handed that device function, so there is
nothing left to tolerate:

  a. message words   acg_ldpc_debug_bp_trace after 1, 2, 3, 10 and 25 iterations, bit for bit, for the debug instances of four
                     engines (tests/test_spa_ref.py shows that one changed operation moves these words and no hard output)
  b. outputs         (bits, ok, iters) of every frame for the production instances: group sizes, fixed-work variants, the
                     workgroup-per-frame kernels, both streamed kernels, fp64
  c. knife edges     frames whose flag one message of the first iteration decides to the last bit, built with the device phi:
                     where a production instance that parts from its debug twin by an ulp shows — on a graph the variable
                     sweep decides and on one whose targeted variables are absorbed into their checks
  d. Monte-Carlo     the seven counters, device noise and host noise

Each instance is identified through describe() / layout(), so a silent fallback to another kernel fails the test."""
import contextlib
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from awgn_ref import classify, sent_words
from minsum_ref import Graph, channel_llr
from spa_cases import (SPA_SNR, SPA_SNR_SATURATED, SPA_TRACE_FRAMES, SPA_TRACE_SNRS, irregular, irregular_frames, noisy_zero, ragged,
                       ragged_frames, spa_frames, wide_code, wide_frames)
from spa_ref import KNIFE_SNR, LN2, flooding_sumproduct, fused_post, knife_edge_case

pytestmark = pytest.mark.gpu
MATS = ("H", "H05", "optimalH")
SPEC = {"H05": ("H05_L32", 32), "H": ("H_L64", 64), "optimalH": ("optimalH_L32", 32)}      # the build-time instances (csrc/Makefile)


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


@pytest.fixture(scope="module")
def phis(A):
    """{float32: Dom<float>::phi (log2(e)-scaled domain), float64: phi_f (natural domain)}, evaluated on the device"""
    def phi32(x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.zeros(3 * x.size, dtype=np.uint32)
        assert A.lib().acg_ldpc_debug_phi_sat(x.ctypes.data, out.ctypes.data, x.size) == 0
        return out[0::3].copy().view(np.float32).reshape(x.shape)

    def phi64(x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.zeros(x.size, dtype=np.float64)
        assert A.lib().acg_ldpc_debug_phi(x.ctypes.data, out.ctypes.data, x.size, 1) == 0
        return out.reshape(x.shape)
    return {np.dtype(np.float32): phi32, np.dtype(np.float64): phi64}


@contextlib.contextmanager
def _env(*names):
    """developer switches read when a decoder handle is created"""
    for k in names:
        os.environ[k] = "1"
    try:
        yield
    finally:
        for k in names:
            del os.environ[k]


class _Refs:
    """restatement results with the device phi, computed once per (graph, symbols — by content —, snr, sweeps, type) and left unchanged"""

    def __init__(self, phis):
        self.phis, self.graphs, self.memo = phis, {}, {}

    def graph(self, key, Hm):
        if key not in self.graphs:
            self.graphs[key] = Graph(Hm)
        return self.graphs[key]

    def __call__(self, key, Hm, y, snr, iters, dt=np.float32, trace_at=None):
        dt = np.dtype(dt)
        k = (key, y.dtype.str, y.shape, hashlib.sha1(np.ascontiguousarray(y).tobytes()).hexdigest(), float(snr), iters, dt.str, trace_at)
        if k not in self.memo:
            r = flooding_sumproduct(self.graph(key, Hm), y, snr, iters, self.phis[dt], dt, trace_at=trace_at)
            self.memo[k] = r[3] if trace_at else r
        return self.memo[k]


@pytest.fixture(scope="module")
def refs(phis):
    return _Refs(phis)


@pytest.fixture(scope="module")
def sets(A, oracle, matrices):
    """name -> (Hm, ParityCheckMatrix, {snr: symbols [192, n]}, sweeps)"""
    out = {}
    for n in MATS:
        Hm = matrices[n]
        out[n] = (Hm, A.ParityCheckMatrix(Hm), {snr: spa_frames(oracle, Hm, snr)[1] for snr in (SPA_SNR[n], SPA_SNR_SATURATED)}, 50)
    Hr, (yr, sr) = ragged(), ragged_frames()
    out["ragged"] = (Hr, A.ParityCheckMatrix(Hr), {sr: yr}, 12)
    Hi = irregular()
    yi, si = irregular_frames(Hi.shape[1])
    out["irregular"] = (Hi, A.ParityCheckMatrix(Hi), {si: yi}, 30)
    Hw, (yw, sw) = wide_code(), wide_frames()
    out["wide"] = (Hw, A.ParityCheckMatrix(Hw), {sw: yw}, 20)
    return out


@pytest.fixture(scope="module")
def big(A):
    """BASELINE configs[4]: (3,6)-regular 5000 x 10000, 64 frames at +2 dB (exits after a few sweeps) and at the threshold"""
    Hm = A.regular_ldpc(5000, 10000, 3, 6, seed=1)
    return Hm, A.ParityCheckMatrix(Hm), {snr: noisy_zero(10000, 64, snr, 7 + i) for i, snr in enumerate((2.0, -1.6))}


def _assert_same(got, want, ctx):
    """equality of bits, ok and iters for every frame; the message names the first differing frame and what differs there"""
    (bits, ok, iters), (rb, rok, rit) = got, want
    assert bits.shape == rb.shape and ok.shape == rok.shape and iters.shape == rit.shape, ctx
    d_flag, d_word, d_count = ok != rok, (bits != rb).any(axis=1), iters != rit
    bad = d_flag | d_word | d_count
    if bad.any():
        f = int(np.nonzero(bad)[0][0])
        what = ", ".join(n for n, d in (("flag", d_flag), ("word", d_word), ("count", d_count)) if d[f])
        pytest.fail("%s: %d of %d frames differ; first: frame %d, differing in %s (kernel ok=%d iters=%d, restatement ok=%d iters=%d, "
                    "%d word bits apart)" % (ctx, int(bad.sum()), len(bad), f, what, ok[f], iters[f], rok[f], rit[f],
                                             int((bits[f] != rb[f]).sum())))


# ------------------------------------------------------------------------------------------ the instances
# name -> (decoder arguments, switches, what describe() must contain / layout() must match, storage type)
def _instances(A):
    inst = {}
    for L in (16, 32, 64):
        inst["fused%d" % L] = (dict(lanes_per_frame=L), (), ["kernel=bp_fused_kernel ", " f64=0 ", dict(lanes_per_frame=L)], np.float32)
        inst["fused%d_f64" % L] = (dict(lanes_per_frame=L, precision=A.PREC_F64), (),
                                   ["kernel=bp_fused_kernel ", " f64=1 ", dict(lanes_per_frame=L)], np.float64)
    inst["block256"] = (dict(lanes_per_frame=256), (), ["kernel=bp_block_kernel ", " f64=0 ", dict(lanes_per_frame=256, frames_per_block=1)],
                        np.float32)
    inst["streamed_ring"] = (dict(engine=A.ENGINE_STREAMED), (), ["engine=streamed ", "kernel=bp_streamed_ring_kernel<", " f64=0 "], np.float32)
    inst["streamed_regs"] = (dict(engine=A.ENGINE_STREAMED), ("ACG_STREAM_NO_RING",), ["engine=streamed ", "kernel=bp_streamed_kernel ", " f64=0 "],
                             np.float32)
    inst["streamed_f64"] = (dict(engine=A.ENGINE_STREAMED, precision=A.PREC_F64), (), ["engine=streamed ", "kernel=bp_streamed_kernel ", " f64=1 "],
                            np.float64)
    return inst


FIXED_VARIANTS = (("ACG_BP_NO_SPEC",), ("ACG_BP_NO_SATSKIP",), ("ACG_BP_NO_PHIMEMO",), ("ACG_BP_NO_FREEZE",), ("ACG_BP_NO_ABSORB",))


def _decoder(A, H, iters, ee, kw, sw, want):
    """a sum-product decoder whose handle for H was created under the switches `sw` -> (decoder, describe()); `want`:
    substrings describe() must contain / layout() entries that must match"""
    dec = A.BeliefPropagationDecoder(iters, early_exit=ee, **kw)
    try:
        with _env(*sw):
            d, lay = dec.describe(H), dec.layout(H)
    except Exception:
        dec.close()
        raise
    assert d.startswith("sum-product ") and "schedule=flooding" in d, d
    for w in want:
        if isinstance(w, str):
            assert w in d + " ", (w, d)
        else:
            assert lay == dict(lay, **w), (w, lay)
    return dec, d


def _lds_bytes(A, H, kw, sw=()):
    """layout()['lds_bytes_per_frame'] of a fixed-work handle created under the switches `sw`"""
    dec, _ = _decoder(A, H, 50, False, kw, sw, ())
    try:
        return dec.layout(H)["lds_bytes_per_frame"]
    finally:
        dec.close()


def _absorbs(A, H, kw):
    """whether the handle takes the layout with absorbed degree-1 variables (BpLayout::n_apass > 0): an absorbed pass has one row
    of message words less, so the frame's LDS bytes differ from those under ACG_BP_NO_ABSORB"""
    return _lds_bytes(A, H, kw) != _lds_bytes(A, H, kw, ("ACG_BP_NO_ABSORB",))


def _decode(A, H, y, snr, iters, ee, kw, sw=(), want=()):
    dec, d = _decoder(A, H, iters, ee, kw, sw, want)
    try:
        return dec.decode_batch(H, y, snr), d
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------ a. message words
TRACE_ENGINES = {"fused": (0, "fused"), "fused32": (32, "fused"), "fused64": (64, "fused"), "fused_block256": (256, "fused"),
                 "streamed_ring": (0, "streamed"), "streamed_regs": (0, "streamed")}
TRACE_ITERS = (1, 2, 3, 10, 25)


def _trace(A, H, y, snr, it, f64, streamed, lpf):
    nf, E = len(y), H.E
    y = np.ascontiguousarray(y, dtype=np.float64)
    c2v, mag, sgn = (np.zeros((nf, E)) for _ in range(3))
    post = np.zeros((nf, H.n))
    rc = A.lib().acg_ldpc_debug_bp_trace(H._h, y.ctypes.data, nf, float(snr), it, f64, A.ENGINE_STREAMED if streamed else A.ENGINE_FUSED,
                                         lpf, c2v.ctypes.data, mag.ctypes.data, sgn.ctypes.data, post.ctypes.data)
    return rc, c2v, mag, sgn, post


def _words(x, dt):
    """the trace's doubles back as words of the kernel's type (tests/test_spa_ref.py: the float32 round trip is exact)"""
    if np.dtype(dt) == np.float64:
        return x.view(np.uint64)
    with np.errstate(invalid="ignore"):
        return (x / LN2).astype(np.float32).view(np.uint32)


def _first(diff):
    f, e = np.argwhere(diff)[0]
    return "%d differ; first: frame %d, index %d" % (int(diff.sum()), f, e)


def _compare_trace(g, llr, trace, got, dt, streamed, ctx):
    """NaN words are compared as NaN (x86 and the GPU generate quiet NaNs of opposite sign); no case set here forms one"""
    dt = np.dtype(dt)
    U = np.uint32 if dt == np.float32 else np.uint64
    c2v, v2c, post = trace
    _, gc, gm, gs, gp = got
    nan = np.isnan(c2v)
    d = (_words(gc, dt) != c2v.view(U)) & ~(nan & np.isnan(gc))
    assert not d.any(), (ctx, "c2v", _first(d))
    stripped = v2c.view(U) & ~U(1)
    d = (_words(gm, dt) != (stripped & ~U(1 << (dt.itemsize * 8 - 1)))) & ~(np.isnan(v2c) & np.isnan(gm))
    assert not d.any(), (ctx, "v2c magnitude", _first(d))
    d = gs != np.where(np.signbit(stripped.view(dt)), -1.0, 1.0)
    assert not d.any(), (ctx, "v2c sign", _first(d))
    if streamed:
        d = (_words(gp, dt) != post.view(U)) & ~(np.isnan(post) & np.isnan(gp))
    else:
        want = fused_post(g, llr, c2v, dt)
        d = (gp != want) & ~(np.isnan(want) & np.isnan(gp))
    assert not d.any(), (ctx, "post", _first(d))


# (graph, engine) pairs of a.: every graph on every engine, but the (4,16) code — check degree 16 — on the streamed ones only
TRACE_CASES = [(n, e) for n in MATS + ("ragged", "irregular", "wide") for e in sorted(TRACE_ENGINES)
               if n != "wide" or TRACE_ENGINES[e][1] == "streamed"]
# what the API must refuse (code 3, "no debug instance"): the fused debug instance is the headline variant — LLRs in registers,
# at most 12 variable passes — and the irregular graph has 584 variables: 19 passes of 32 lanes
TRACE_REFUSED = {("irregular", "fused32")}


@pytest.mark.parametrize("name,engine", TRACE_CASES)
def test_message_words(A, oracle, sets, refs, name, engine, monkeypatch):
    """c->v words, v->c words (LSB stripped, as the API strips it) and posteriors after 1, 2, 3, 10 and 25 iterations of 64 frames,
    fp32 and fp64 (the streamed ring is fp32 only: fp64 streams through bp_streamed_kernel, the streamed_regs case).  The
    streamed posterior is the kernel's own word llr + s; the fused one is a host-side double sum of the dumped words, formed
    here from the restatement's words in the same way.  Every case traces every leg — the count is asserted — except
    TRACE_REFUSED, where the refusal is asserted; `fused` (lanes left to the library) on the irregular graph is whichever of the
    two the library's choice of lanes makes it, and says which."""
    Hm, H, ys, _ = sets[name]
    lpf, kind = TRACE_ENGINES[engine]
    streamed = kind == "streamed"
    if engine == "streamed_regs":
        monkeypatch.setenv("ACG_STREAM_NO_RING", "1")
    refused = (name, engine) in TRACE_REFUSED
    if (name, engine) == ("irregular", "fused"):
        dec, _ = _decoder(A, H, 1, False, {}, (), ["kernel=bp_fused_kernel "])
        refused = dec.layout(H)["lanes_per_frame"] == 32
        print("irregular graph, lanes left open: %d lanes per frame" % dec.layout(H)["lanes_per_frame"])
        dec.close()
    g = refs.graph(name, Hm)
    traced = 0
    if name in MATS:
        ys = {snr: spa_frames(oracle, Hm, snr, SPA_TRACE_FRAMES)[1] for snr in SPA_TRACE_SNRS}
    legs = ((0, np.float32),) if engine == "streamed_ring" else ((0, np.float32), (1, np.float64))
    for snr, y in ys.items():
        y = y[:SPA_TRACE_FRAMES]
        for f64, dt in legs:
            llr = channel_llr(y, snr, dt)
            for it in TRACE_ITERS:
                got = _trace(A, H, y, snr, it, f64, streamed, lpf)
                if refused:
                    assert got[0] == 3 and b"no debug instance" in A.lib().acg_ldpc_last_error(), (name, engine, f64, it, got[0])
                    continue
                assert got[0] == 0, (name, engine, f64, it, A.lib().acg_ldpc_last_error())
                _compare_trace(g, llr, refs(name, Hm, y, snr, 0, dt, trace_at=it), got, dt, streamed, (name, engine, snr, "f64=%d" % f64, it))
                traced += 1
    assert traced == (0 if refused else len(ys) * len(legs) * len(TRACE_ITERS)), (name, engine, traced)


# ------------------------------------------------------------------------------------------ b. production instances
def _sweep(A, refs, key, Hm, H, y64, snr, its, kw, sw, want, dt, counts=(1, 63, 65)):
    """whole batch: double and float symbols x sweeps x early exit / fixed work; prefixes of 1, 63 and 65 frames at the first
    entry of `its` -> the restatement's results for the double symbols at its[0]"""
    for y in (y64, y64.astype(np.float32)):
        for it in its:
            ref = refs(key, Hm, y, snr, it, dt)
            for ee in (True, False):
                got, d = _decode(A, H, y, snr, it, ee, kw, sw, want)
                _assert_same(got, ref, (key, d.split(" kernel=")[1].split()[0], kw, sw, snr, y.dtype.name, it, "early exit" if ee else "fixed work"))
    ref = refs(key, Hm, y64, snr, its[0], dt)
    for n in counts:
        if n < len(y64):
            for ee in (True, False):
                got, _ = _decode(A, H, y64[:n], snr, its[0], ee, kw, sw, want)
                _assert_same(got, tuple(a[:n] for a in ref), (key, kw, sw, snr, "frames", n, ee))
    return ref


@pytest.mark.parametrize("lpf", [16, 32, 64])
@pytest.mark.parametrize("name", MATS)
def test_wave_group_fp32_exact(A, sets, refs, name, lpf):
    """bp_fused_kernel<float, ..., ALGO = 0> at 16 / 32 / 64 lanes per frame: 192 frames below the waterfall and 192 at +6 dB,
    50 / 3 / 1 / 0 sweeps; the fixed-work legs additionally one switch at a time: the generic instance instead of the
    build-time one, no phi fast path, no phi memo, no freeze, no absorbed variables.  (The freeze path needs the LLRs in
    registers, n <= 12 lanes: describe() says freeze=0 for the 280-variable codes at 16 lanes.)  describe() shows the spec, the
    fast path (through freeze) and the freeze switches; ACG_BP_NO_ABSORB shows in layout(): H05 at 32 and 64 lanes takes the
    absorbed layout (its trailing check passes hold only checks with one degree-1 variable in the last column) and nothing
    else among these nine does, so the switch is a no-op on the other eight; ACG_BP_NO_PHIMEMO changes an argument of the same kernel and shows nowhere."""
    Hm, H, ys, _ = sets[name]
    kw, sw, want, dt = _instances(A)["fused%d" % lpf]
    spec, spec_l = SPEC[name]
    absorbs = _absorbs(A, H, kw)
    print("%s at %d lanes: absorbed layout %s" % (name, lpf, "taken" if absorbs else "not taken"))
    assert absorbs == (name == "H05" and lpf >= 32), (name, lpf, absorbs)      # (optimalH's trailing passes hold non-candidates)
    for snr, y in ys.items():
        rb, rok, rit = _sweep(A, refs, name, Hm, H, y, snr, (50, 3, 1, 0), kw, sw, want, dt)
        if snr == SPA_SNR[name]:
            assert 0 < rok.sum() < len(rok) and rit[rok == 1].min() <= 5 and rit[rok == 1].max() > 20
        for it in (50, 3):
            ref = refs(name, Hm, y, snr, it, dt)
            got, d = _decode(A, H, y, snr, it, False, kw, (), want + [" freeze=%d " % (H.n <= 12 * lpf), " spec=%s " % (spec if lpf == spec_l else "0")])
            _assert_same(got, ref, (name, lpf, snr, it, "fixed work", d))
            for v in FIXED_VARIANTS:
                w = {"ACG_BP_NO_SPEC": [" spec=0 "], "ACG_BP_NO_SATSKIP": [" freeze=0 ", " spec=0 "], "ACG_BP_NO_FREEZE": [" freeze=0 "]}.get(v[0], [])
                got, d = _decode(A, H, y, snr, it, False, kw, v, want + w)
                _assert_same(got, ref, (name, lpf, snr, it, v))


@pytest.mark.parametrize("lpf", [16, 32, 64])
@pytest.mark.parametrize("name", MATS)
def test_wave_group_fp64_exact(A, sets, refs, name, lpf):
    """bp_fused_kernel<double, ...>: phi_f through the device math library, natural domain"""
    Hm, H, ys, _ = sets[name]
    kw, sw, want, dt = _instances(A)["fused%d_f64" % lpf]
    for snr, y in ys.items():
        _sweep(A, refs, name, Hm, H, y, snr, (50, 3, 1, 0), kw, sw, want, dt)


def test_block_fp32_exact_h05_256_lanes(A, sets, refs):
    Hm, H, ys, _ = sets["H05"]
    kw, sw, want, dt = _instances(A)["block256"]
    for snr, y in ys.items():
        _sweep(A, refs, "H05", Hm, H, y, snr, (50, 3, 1, 0), kw, sw, want, dt)


def test_block_and_streamed_exact_on_the_configs4_code(A, big, refs):
    """bp_block_kernel, 1024 threads per frame (index table in registers, regular instance) with its idx_reg switches, and both
    streamed kernels on a code whose state does not fit in LDS otherwise: 64 frames at +2 dB and at the threshold (-1.6 dB).
    One handle per instance serves both SNRs: creating one for this code (placement, the streamed workspace) costs more than
    decoding with it."""
    Hm, H, ys = big
    blk = ["kernel=bp_block_kernel ", " f64=0 ", dict(lanes_per_frame=1024, frames_per_block=1)]
    inst = _instances(A)
    runs = [(50, True, {}, (), blk + ["idx_reg=1 "], 64), (50, False, {}, (), blk + ["idx_reg=1 "], 64), (3, True, {}, (), blk + ["idx_reg=1 "], 64)]
    for sw, w in ((("ACG_BP_NO_IDXREG",), "idx_reg=0 "), (("ACG_BP_NO_PLACEMENT",), "idx_reg=1 "), (("ACG_BP_NO_REGULAR",), "idx_reg=1 "),
                  (("ACG_BP_NO_IDXREG", "ACG_BP_NO_PLACEMENT", "ACG_BP_NO_REGULAR"), "idx_reg=0 ")):
        runs.append((50, True, {}, sw, blk + [w], 64))
    for e, modes in (("streamed_ring", (True, False)), ("streamed_regs", (True,))):      # (61 frames: a tile that is not full)
        kw, sw, want, _ = inst[e]
        runs += [(50, ee, kw, sw, want, 61) for ee in modes]
    for it, ee, kw, sw, want, n in runs:
        dec, d = _decoder(A, H, it, ee, kw, sw, want)
        try:
            for snr, y in ys.items():
                _assert_same(dec.decode_batch(H, y[:n], snr), tuple(a[:n] for a in refs("big", Hm, y, snr, it)), ("big", snr, it, ee, sw, d))
        finally:
            dec.close()
    (_, k2, i2), (_, k16, i16) = refs("big", Hm, ys[2.0], 2.0, 50), refs("big", Hm, ys[-1.6], -1.6, 50)
    print("configs[4] code: +2 dB %d of 64 ok, exit iterations %d..%d; -1.6 dB %d of 64 ok, exit iterations %s"
          % (k2.sum(), i2.min(), i2.max(), k16.sum(), sorted(set(i16.tolist()))))
    assert k2.all() and i2.max() <= 12 and len(set(i16.tolist())) > 3 and i16.max() > 25
    assert not refs("big", Hm, ys[-1.6], -1.6, 3)[1].any()      # three sweeps at the threshold: the failing exit


@pytest.mark.parametrize("engine", ["streamed_ring", "streamed_regs", "streamed_f64"])
def test_streamed_exact(A, sets, refs, engine):
    """messages in HBM, one lane per frame: the LDS-DMA ring instance (default), the register-staged one and its fp64 instance;
    192 frames (three tiles) and prefixes that do not fill a tile"""
    kw, sw, want, dt = _instances(A)[engine]
    for name in MATS:
        Hm, H, ys, _ = sets[name]
        for snr, y in ys.items():
            _sweep(A, refs, name, Hm, H, y, snr, (50, 3, 1, 0) if name == "H05" else (50, 1), kw, sw, want, dt)
    Hm, H, ys, it = sets["wide"]
    if engine != "streamed_ring":                                # (whichever kernel the default picks for degree 16 runs in the regs case)
        for snr, y in ys.items():
            _sweep(A, refs, "wide", Hm, H, y, snr, (it, 1), kw, sw, want, dt)


def test_ragged_graphs_through_every_instance(A, sets, refs):
    """one-/two-variable checks (phi(+0) = +inf), an empty row, isolated and degree-1 variables through every instance that
    accepts the graph; the ones that must are named.  (Neither graph takes the absorbed layout — their trailing check pass
    holds checks that are no candidates —, so ACG_BP_NO_ABSORB is a no-op here; asserted, so that nobody reads these legs as
    covering check_abs: H05 and the absorbed knife-edge graph do.)"""
    inst = _instances(A)
    for name, must in (("ragged", set(inst)), ("irregular", {"fused64", "fused64_f64", "block256", "streamed_ring", "streamed_regs", "streamed_f64"})):
        Hm, H, ys, it = sets[name]
        (snr, y), = ys.items()
        ran = set()
        for e, (kw, sw, want, dt) in inst.items():
            try:
                dec, _ = _decoder(A, H, it, True, kw, sw, want)
                dec.close()
            except A.LdpcError:
                assert e not in must, (name, e)
                continue
            ref = _sweep(A, refs, name, Hm, H, y, snr, (it, 2), kw, sw, want, dt, counts=(63,))
            if e.startswith("fused") and dt == np.float32:
                assert not _absorbs(A, H, kw), (name, e)
                for v in FIXED_VARIANTS:
                    got, _ = _decode(A, H, y, snr, it, False, kw, v, want)
                    _assert_same(got, ref, (name, e, v))
            assert 0 < ref[1].sum() < len(y)
            ran.add(e)
        print("%s: %s" % (name, sorted(ran)))
        assert ran >= must, (name, must - ran)


def _extreme(oracle, Hm):
    """H05 at +1 dB, 192 frames; up to five random positions per frame replaced, cycling through zero, a denormal, 1e30 with the
    sent sign, infinity with the sent sign, -infinity whatever was sent, -1e30 whatever was sent and NaN"""
    cws, y = spa_frames(oracle, Hm, 1.0)
    y = y.copy()
    sent = 1.0 - 2.0 * cws.astype(np.float64)
    rng = np.random.default_rng(4)
    k = 0
    for f in range(len(y)):
        for v in rng.choice(y.shape[1], size=int(rng.integers(0, 6)), replace=False):
            y[f, v] = (0.0, 1e-310, 1e30 * sent[f, v], np.inf * sent[f, v], -np.inf, -1e30, np.nan)[k % 7]
            k += 1
    return y


def test_extreme_symbols(A, oracle, sets, refs):
    """0, a denormal, +-1e30, +-inf and NaN symbols, by the source's rules: `x <= 0` is false for a NaN, phi(NaN) and phi(inf)
    come from the device.  (A NaN's payload and sign never reach an output: every word is used through <=, phi and bit masks.)"""
    Hm, H, _, _ = sets["H05"]
    y = _extreme(oracle, Hm)
    assert np.isnan(y).any() and np.isinf(y).any() and (y == 0).any() and (np.abs(y) == 1e30).any() and (y == 1e-310).any()
    for e, (kw, sw, want, dt) in _instances(A).items():
        for yy in (y, y.astype(np.float32)):
            ref = refs("H05", Hm, yy, 1.0, 50, dt)
            for ee in (True, False):
                got, d = _decode(A, H, yy, 1.0, 50, ee, kw, sw, want)
                _assert_same(got, ref, ("extreme symbols", e, yy.dtype.name, ee))
        assert 0 < ref[1].sum() < len(y)


# ------------------------------------------------------------------------------------------ c. one message, to the last bit
@pytest.mark.parametrize("absorbed", [False, True])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_knife_edges(A, phis, dt, absorbed):
    """spa_ref.knife_edge_case built with the DEVICE phi: one message of the first iteration meets an LLR of exactly minus its
    value (total +0: hard 1) or minus the next number towards zero (total > 0: hard 0), for checks of degree 1 ... 8.  max_iter = 1,
    every instance that accepts the graph, the fixed-work switches included.  Two graphs:
      absorbed=False   eight disjoint checks.  Every variable has degree 1, but a check with several of them is no candidate for
                       absorption: all instances decide the targeted variable in the variable sweep (BpPass::var_at, StreamPass::var)
      absorbed=True    spa_ref.knife_edge_graph_absorbed: every check's last edge is its only degree-1 variable, and that edge
                       is the targeted one.  The fp32 wave-group kernels take the absorbed layout — asserted from layout(): the
                       frame's LDS bytes differ from those under ACG_BP_NO_ABSORB, at 16, 32 and 64 lanes — so the knife edge
                       is decided by BpPass::check_abs (`allr + R <= 0`), in the fixed-work instances behind the phi memo;
                       under ACG_BP_NO_ABSORB, in fp64 and in the other engines the variable sweep decides it.  The debug
                       instances at 32 and 64 lanes are traced on this graph as well, absorbed words included."""
    dt = np.dtype(dt)
    Hm, y, knife, kind_b, dropped = knife_edge_case(phis[dt], KNIFE_SNR, 320, 3, dt, absorbed)
    print("%s knife edges (device phi%s): %d of 320 frames kept; dropped per degree 1..8: %s"
          % (dt.name, ", absorbed graph" if absorbed else "", len(y), dropped.tolist()))
    assert (dropped <= 10).all(), dropped
    H = A.ParityCheckMatrix(Hm)
    g = Graph(Hm)
    rb, rok, rit, (_, _, post) = flooding_sumproduct(g, y, KNIFE_SNR, 1, phis[dt], dt, trace_at=1)
    pk = post[np.arange(len(y)), knife]
    assert (pk[~kind_b] == 0).all() and (pk[kind_b] > 0).all()
    want_res = flooding_sumproduct(g, y, KNIFE_SNR, 1, phis[dt], dt)
    assert 0 < want_res[1].sum() < len(y)
    ran = set()
    for e, (kw, sw, want, idt) in _instances(A).items():
        if np.dtype(idt) != dt:
            continue
        try:
            dec, _ = _decoder(A, H, 1, True, kw, sw, want)
            dec.close()
        except A.LdpcError:
            continue
        if e.startswith("fused"):
            assert _absorbs(A, H, kw) == (absorbed and dt == np.float32), (e, absorbed)
        for ee in (True, False):
            got, d = _decode(A, H, y, KNIFE_SNR, 1, ee, kw, sw, want)
            _assert_same(got, want_res, ("knife edges", e, "early exit" if ee else "fixed work"))
        if e.startswith("fused") and dt == np.float32:
            for v in FIXED_VARIANTS:
                got, _ = _decode(A, H, y, KNIFE_SNR, 1, False, kw, v, want)
                _assert_same(got, want_res, ("knife edges", e, v))
        ran.add(e)
    print("knife edges ran on: %s" % sorted(ran))
    assert ran >= ({"fused16", "fused32", "fused64", "block256", "streamed_ring", "streamed_regs"} if dt == np.float32
                   else {"fused16_f64", "fused32_f64", "fused64_f64", "streamed_f64"}), ran
    if absorbed:
        llr = channel_llr(y[:64], KNIFE_SNR, dt)
        for lpf in (32, 64):
            for it in (1, 2):
                got = _trace(A, H, y[:64], KNIFE_SNR, it, int(dt == np.float64), False, lpf)
                assert got[0] == 0, (lpf, it, A.lib().acg_ldpc_last_error())
                trace = flooding_sumproduct(g, y[:64], KNIFE_SNR, 0, phis[dt], dt, trace_at=it)[3]
                _compare_trace(g, llr, trace, got, dt, False, ("knife edges, absorbed graph", lpf, dt.name, it))


# ------------------------------------------------------------------------------------------ d. Monte-Carlo path
MC_FRAMES, MC_FIRST, MC_SEED, MC_SNR = 1027, 1000, 99, -2.0


@pytest.fixture(scope="module")
def mc(A, sets, refs):
    """the symbols the Monte-Carlo run decodes (acg_ldpc_awgn_dev: same Philox keys), decoded by the restatement through the
    float-symbol LLR path and classified on the host as experiment.h does -> the counters run_experiment must return"""
    import torch
    from acg_alp_ldpc_amd._lib import McCfg, check, lib
    Hm, H, _, _ = sets["H05"]
    G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 512, 1)
    dec = A.BeliefPropagationDecoder(50)
    h, _ = dec.handle(H)
    cfg = McCfg()
    cfg.frames, cfg.first_frame, cfg.snr, cfg.seed, cfg.noise = MC_FRAMES, MC_FIRST, MC_SNR, MC_SEED, 0
    cfg.codewords, cfg.n_codewords = cws.ctypes.data, cws.shape[0]
    yd = torch.empty((MC_FRAMES, H.n), dtype=torch.float32, device="cuda")
    check(lib().acg_ldpc_awgn_dev(h, C.byref(cfg), yd.data_ptr(), None))
    dec.sync(H)
    y = yd.cpu().numpy()
    dec.close()
    rb, rok, rit = refs("H05", Hm, y, MC_SNR, 50)
    sent = sent_words(MC_FIRST, MC_FRAMES, H.n, cws)
    return cws, y, sent, classify(y, rb, rok, rit, sent)


@pytest.mark.parametrize("engine", ["fused32", "fused64", "block256", "streamed_ring"])
def test_monte_carlo_counters_equal_the_restatement(A, sets, mc, engine):
    """device noise: all seven counters, early exit and fixed work, in one shard and in three"""
    _, H, _, _ = sets["H05"]
    cws, y, sent, want = mc
    assert 0 < want["correct"] < MC_FRAMES
    kw, sw, wd, _ = _instances(A)[engine]
    for ee in (True, False):
        dec, _ = _decoder(A, H, 50, ee, kw, sw, wd)
        try:
            r = A.run_experiment(dec, cws, H, MC_SNR, frames=MC_FRAMES, first_frame=MC_FIRST, noise="device", seed=MC_SEED)
            got = {k: getattr(r, k) for k in want}
            assert got == want, (engine, ee, got, want)
            tot = None
            for rank in range(3):
                lo, cnt = A.shard_range(MC_FRAMES, rank, 3)
                part = A.run_experiment(dec, cws, H, MC_SNR, frames=cnt, first_frame=MC_FIRST + lo, noise="device", seed=MC_SEED)
                tot = part if tot is None else A.merge_exp_results(tot, part)
            got = {k: getattr(tot, k) for k in want}
            assert got == want, (engine, ee, "three shards", got, want)
        finally:
            dec.close()


@pytest.mark.parametrize("engine", ["fused32", "fused64", "block256", "streamed_ring"])
def test_monte_carlo_host_noise_counters_equal_decode_batch(A, sets, refs, engine):
    """host noise (frame g <- mt19937(g + 1)): the counters are those of decode_batch on the same symbols, which b. holds to the
    restatement — and the restatement is asked here once more"""
    Hm, H, _, _ = sets["H05"]
    G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 64, 5)
    F, first = 259, 40
    y = A.transmit_frames(cws, MC_SNR, first_frame=first, frames=F)
    sent = cws[np.arange(first, first + F) % len(cws)]
    kw, sw, wd, _ = _instances(A)[engine]
    for ee in (True, False):
        dec, _ = _decoder(A, H, 50, ee, kw, sw, wd)
        try:
            bits, ok, iters = dec.decode_batch(H, y, MC_SNR)
            want = classify(y, bits, ok, iters, sent)
            r = A.run_experiment(dec, cws, H, MC_SNR, frames=F, first_frame=first, noise="host", seed=1)
            got = {k: getattr(r, k) for k in want}
            assert got == want, (engine, ee, got, want)
            _assert_same((bits, ok, iters), refs("H05", Hm, y, MC_SNR, 50), ("host noise", engine, ee))
        finally:
            dec.close()
