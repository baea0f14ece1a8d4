"""GPU: the STATE of the streamed layered engines — every posterior and every message a tile leaves in its slab, read through
acg_ldpc_debug_streamed_slab (Decoder.streamed_slab) — against the restatements' (tests/layered_ref.py with the device's own phi,
tests/streamed_q_ref.py), bit for bit, signed zeros included.  Word, flag and iteration count are compared in the same calls.
tests/test_streamed_state.py counts on the CPU what this sees and a comparison of the three hard outputs does not: the edge order of
a check, the order of the prefix and suffix sums across a chunk boundary, the subtraction of a STORED message, the store of R, the
rule that a latched lane writes nothing.

Everything here runs on handles of ONE tile (ACG_STREAML_TILES=1 / ACG_STREAMQ_TILES=1, set before the handle is made): one
workgroup takes the tiles of a launch in order, so slab 0 holds the last tile of the last decode."""
import ctypes as C

import numpy as np
import pytest

import layered_q_cases as Q
import streamed_state_cases as SS
from layered_ref import layered_minsum, layered_sumproduct_exact
from test_layered_q_io_gpu import _assert_same4
from test_layered_spa_exact_gpu import _assert_same, device_phi  # noqa: F401 (device_phi: a fixture)

pytestmark = pytest.mark.gpu

T = SS.T
TILES = {"first": (slice(0, 64), 64), "second": (slice(64, SS.FRAMES), SS.FRAMES)}      # frames of the tile, frames to decode


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


@pytest.fixture()
def one_tile(monkeypatch):
    monkeypatch.setenv("ACG_STREAML_TILES", "1")
    monkeypatch.setenv("ACG_STREAMQ_TILES", "1")


@pytest.fixture(scope="module")
def c(A):
    return SS.tails(A)


def _bits(a):
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def _assert_words(got, want, what, ctx):
    """got, want: [lanes, cells] of one type, compared as bit patterns"""
    assert got.shape == want.shape and got.dtype == want.dtype, (ctx, what, got.shape, want.shape, got.dtype, want.dtype)
    bad = _bits(got) != _bits(want)
    if bad.any():
        l, k = (int(x) for x in np.argwhere(bad)[0])
        pytest.fail("%s: %d of %d %s words differ in %d of %d lanes; first: lane %d, cell %d, kernel %r (0x%x), restatement %r (0x%x)"
                    % (ctx, int(bad.sum()), bad.size, what, int(bad.any(axis=1).sum()), len(bad), l, k, got[l, k], int(_bits(got)[l, k]),
                       want[l, k], int(_bits(want)[l, k])))


def _decode_and_read(dec, H, y, snr, want, frames, ctx, messages=True):
    """decode y on the one-tile handle, hold word, flag and count to want[0:3], read slab 0 and hold the lanes of its last tile to
    want[3] (and want[4]) of `frames`; lanes beyond the tile: P = +0 in every cell -> (P, R) of the tile's lanes"""
    _assert_same(dec.decode_batch(H, y, snr), tuple(a[:len(y)] for a in want[:3]), ctx)
    P, R = dec.streamed_slab(H)
    nf = frames.stop - frames.start
    assert P.shape[0] == T and R.shape[0] == T and P.dtype == np.float32 and R.dtype == np.float32
    _assert_words(P[:nf], want[3][frames], "posterior", ctx)
    if messages:
        _assert_words(R[:nf], want[4][frames], "message", ctx)
    assert not _bits(P[nf:]).any(), (ctx, "a lane beyond the tile's frames holds a posterior other than +0")
    return P[:nf], R[:nf]


# ------------------------------------------------------------------------------------------------ 1. float engine, `tails`
@pytest.mark.parametrize("it", [0, 1, 2, 3, 10, 25])
@pytest.mark.parametrize("algo", SS.ALGOS)
def test_tails_state_equals_restatement(A, c, device_phi, one_tile, algo, it):
    """frames 0 ... 63 decoded alone, then all 101 on the same handle — the second tile of 37 frames is the slab's next occupant,
    so anything it took over from the one before shows — with early exit and with fixed work: every posterior and message word
    of the tile's lanes equals the restatement's, lanes 37 ... 63 of the short tile hold P = +0 (their R is unspecified and is
    not looked at), and the state with early exit is the state with fixed work: a latched lane wrote nothing.  max_iter = 0
    compares P alone (R is unspecified there): the channel LLR and, for sum-product, its log2(e) scaling; for 0 and 3
    iterations also with float symbols, the other rounding of the LLR."""
    for f32 in ((False, True) if it in (0, 3) else (False,)):
        want = c.ref(algo, it, device_phi, f32=f32)
        assert not np.isnan(want[3]).any() and not np.isnan(want[4]).any()
        y = c.y.astype(np.float32) if f32 else c.y
        state = {}
        for ee in (True, False):
            dec = SS.decoder(A, algo, it, ee)
            try:
                assert " tiles=1 " in dec.describe(c.H), dec.describe(c.H)
                for name, (frames, F) in TILES.items():
                    ctx = ("tails", algo, it, "float symbols" if f32 else "double symbols", "early exit" if ee else "fixed work", name + " tile")
                    state[ee, name] = _decode_and_read(dec, c.H, y[:F], c.snr, want, frames, ctx, messages=it > 0)
            finally:
                dec.close()
        for name in TILES:
            _assert_words(state[True, name][0], state[False, name][0], "posterior", (algo, it, name, "early exit against fixed work"))
            if it > 0:
                _assert_words(state[True, name][1], state[False, name][1], "message", (algo, it, name, "early exit against fixed work"))
    if it == 0:
        assert not want[1].any() and (want[2] == 0).all()


@pytest.mark.parametrize("algo", SS.ALGOS)
def test_compared_tiles_hold_every_kind_of_exit(c, device_phi, algo):
    """from the restatement with the device's phi: after 3 iterations each of the two compared tiles holds frames that latched
    before, frames that ran out of iterations and passed the final syndrome pass, and frames that failed; after 25, frames that
    latched early (a latched lane then computes on for up to 23 rounds and must write nothing) and frames that failed"""
    for name, (frames, _) in TILES.items():
        latched, passed, failed = (k[frames] for k in SS.exits(c.ref(algo, 3, device_phi), c.ref(algo, 4, device_phi), 3))
        assert latched.any() and passed.any() and failed.any(), (algo, name, int(latched.sum()), int(passed.sum()), int(failed.sum()))
        r = c.ref(algo, 25, device_phi)
        assert ((r[1][frames] == 1) & (r[2][frames] <= 3)).any() and (r[1][frames] == 0).any(), (algo, name)


# ------------------------------------------------------------------------------------------------------ 2. float engine, H05
@pytest.mark.parametrize("algo", SS.ALGOS)
def test_h05_state_equals_restatement(A, oracle, matrices, device_phi, one_tile, algo):
    """a real code with narrow checks only (degree 3 ... 6, several checks per set): 64 frames at -2 dB, 25 iterations"""
    Hm = matrices["H05"]
    H = A.ParityCheckMatrix(Hm)
    _, layers = H.layers_any()
    G, _ = oracle.get_orthogonal(Hm)
    y = oracle.transmit_frames(oracle.gen_codewords(G, 5, T), -2.0, first_seed=1)
    P, R = [], []
    if algo == "minsum":
        want = layered_minsum(Hm, layers, y, -2.0, 25, SS.MS_SCALE, posteriors=P, messages=R)
    else:
        want = layered_sumproduct_exact(Hm, layers, y, -2.0, 25, device_phi, posteriors=P, messages=R)
    want = tuple(want) + (P[0], R[0])
    assert want[4].shape == (T, H.E) and 0 < want[1].sum() < T and (want[2][want[1] == 1] < 25).any()
    for ee in (True, False):
        dec = SS.decoder(A, algo, 25, ee)
        try:
            _decode_and_read(dec, H, y, -2.0, want, slice(0, T), ("H05", algo, "early exit" if ee else "fixed work"))
        finally:
            dec.close()


# ------------------------------------------------------------------------------------------- 3. float engine, extreme symbols
EXTREME = {
    # sum-product: phi(0) = inf, phi(inf) = 0 and a message is at most 83.25, so no inf - inf forms
    "bp": (0.0, 1e-40, 1e30, -1e30, np.inf, -np.inf),
    # min-sum: an infinite symbol is left out.  The other variable of the two-variable check receives scale * inf = inf; where
    # its own posterior is -inf, or in the next round, where q = inf - inf, a NaN forms (the restatement's state shows it)
    "minsum": (0.0, 1e-40, 1e30, -1e30),
}


def _extreme_tails(c, kinds):
    """the first tile's frames with up to five random symbols per frame replaced, cycling through `kinds`"""
    y = c.y[:T].copy()
    rng = np.random.default_rng(11)
    k = 0
    for f in range(T):
        for v in rng.choice(c.n, size=int(rng.integers(1, 6)), replace=False):
            y[f, v] = kinds[k % len(kinds)]
            k += 1
    return y


@pytest.mark.parametrize("algo", SS.ALGOS)
def test_extreme_symbols_state_equals_restatement(A, c, device_phi, one_tile, algo):
    """zero, a symbol whose fp32 LLR is denormal (1e-40), +-1e30 and, for sum-product, +-infinity sprinkled over the first tile
    of `tails`: the state after 3 iterations.  The restatement's state has no NaN on them (asserted first).  Dropped for
    min-sum: +-infinity, which makes one (EXTREME above).  NaN symbols stay out of scope, as in test_layered_spa_exact_gpu.py:
    the sign of a generated NaN differs between the host and the device."""
    y = _extreme_tails(c, EXTREME[algo])
    for kind in EXTREME[algo]:
        assert (y == kind).any(), kind
    want = c.ref(algo, 3, device_phi, y=y, key="extreme")
    assert not np.isnan(want[3]).any() and not np.isnan(want[4]).any()
    assert np.isinf(want[3]).any() == (algo == "bp")
    for ee in (True, False):
        dec = SS.decoder(A, algo, 3, ee)
        try:
            _decode_and_read(dec, c.H, y, c.snr, want, slice(0, T), ("extreme symbols", algo, "early exit" if ee else "fixed work"))
        finally:
            dec.close()
    # the denormal LLR itself, before any iteration touches it
    w0 = c.ref(algo, 0, device_phi, y=y, key="extreme")
    tiny = np.abs(w0[3][y == 1e-40])
    assert (tiny > 0).all() and (tiny < np.finfo(np.float32).tiny).all()
    dec = SS.decoder(A, algo, 0)
    try:
        _decode_and_read(dec, c.H, y, c.snr, w0, slice(0, T), ("extreme symbols", algo, "max_iter 0"), messages=False)
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------------ 4. quantised engine
def _qdec(A, it, qname, ee=True):
    return A.StreamedQuantizedMinSumDecoder(it, quant=A.QuantConfig(*Q.QUANTS[qname]), early_exit=ee)


@pytest.mark.parametrize("it", [1, 3, 25])
@pytest.mark.parametrize("qname", ["default", "saturating"])
def test_quantised_tails_outputs_and_state(A, c, one_tile, qname, it):
    """`tails` through bp_streamed_q_kernel (a short last chunk of every length 1 ... 7): word, flag, iteration and every posterior
    against decode_int_sparse, as tests/test_streamed_q_gpu.py compares its cases; the slab's P is the returned posteriors and
    its R the restatement's messages, for the first tile alone and for the second as the slab's next occupant"""
    want = c.qref(qname, it)
    ch = c.channel(qname)
    if it == 25:
        assert 0 < want[1].sum() < c.frames
    for ee in (True, False):
        dec = _qdec(A, it, qname, ee)
        try:
            assert " tiles=1 " in dec.describe(c.H), dec.describe(c.H)
            for name, (frames, F) in TILES.items():
                ctx = ("tails", qname, it, "early exit" if ee else "fixed work", name + " tile")
                got = dec.decode_llr_batch(c.H, ch[:F])
                _assert_same4(got, tuple(a[:F] for a in want[:4]), ctx)
                P, R = dec.streamed_slab(c.H)
                nf = frames.stop - frames.start
                assert P.dtype == np.int16 and R.dtype == np.int8 and P.shape == (T, c.n) and R.shape == (T, c.E)
                _assert_words(P[:nf], got[3][frames], "posterior (against the returned ones)", ctx)
                _assert_words(R[:nf], want[4][frames], "message", ctx)
                assert not P[nf:].any(), ctx
        finally:
            dec.close()


# ------------------------------------------------------------------------------------------------------------- 5. the entry
def _slab_call(A, h, slab, out=None, cap=0):
    size = C.c_int64(-1)
    rc = A.lib().acg_ldpc_debug_streamed_slab(h, slab, out, cap, C.byref(size))
    return rc, A.lib().acg_ldpc_last_error().decode(), size.value


def test_entry_sizes_and_refusals(A, c, matrices, one_tile):
    """the size query and a short copy on both engines; refused with a message: a null handle, handles of the other create calls,
    a slab outside 0 ... tiles - 1, a negative capacity"""
    n, E = c.n, c.E
    for dec, size in ((SS.decoder(A, "bp", 2), 4 * (n + E + 5) * T), (SS.decoder(A, "minsum", 2), 4 * (n + E) * T),
                      (_qdec(A, 2, "default"), (2 * n + E) * T)):
        try:
            h, _ = dec.handle(c.H)
            rc, _, got = _slab_call(A, h, 0)
            assert size % 256 == 0 and rc == 0 and got == size, (rc, got, size)
            dec.decode_batch(c.H, c.y[:5], c.snr)
            buf = np.full(64, 0xA5, dtype=np.uint8)
            rc, _, got = _slab_call(A, h, 0, buf.ctypes.data, 16)
            assert rc == 0 and got == size and (buf[16:] == 0xA5).all() and (buf[:16] != 0xA5).any()
            whole = np.zeros(size + 32, dtype=np.uint8)
            whole[size:] = 0x5A
            rc, _, got = _slab_call(A, h, 0, whole.ctypes.data, size + 32)
            assert rc == 0 and got == size and (whole[size:] == 0x5A).all() and (whole[:16] == buf[:16]).all()
            for slab in (-1, 1, 1 << 20):
                rc, msg, got = _slab_call(A, h, slab, whole.ctypes.data, size)
                assert rc != 0 and "outside 0 ... 0" in msg and got == size, (slab, rc, msg)
            rc, msg, _ = _slab_call(A, h, 0, whole.ctypes.data, -1)
            assert rc != 0 and "negative cap_bytes" in msg
            with pytest.raises(A.LdpcError, match="outside"):
                dec.streamed_slab(c.H, 1)
        finally:
            dec.close()
    rc, msg, got = _slab_call(A, None, 0)
    assert rc != 0 and "null decoder" in msg and got == 0
    H05 = A.ParityCheckMatrix(matrices["H05"])
    for other in (A.BeliefPropagationDecoder(3), A.MinSumDecoder(3, 0.75, schedule=A.SCHEDULE_LAYERED, lanes_per_frame=256),
                  A.BeliefPropagationDecoder(3, engine=A.ENGINE_STREAMED, fast_setup=True), A.QuantizedMinSumDecoder(3), A.QPADMMDecoder(0.5, 1.0, 20),
                  A.OSDDecoder(1)):
        try:
            h, _ = other.handle(H05)
            rc, msg, got = _slab_call(A, h, 0)
            assert rc != 0 and got == 0 and "acg_ldpc_decoder_create_layered_streamed or acg_ldpc_decoder_create_quantized_streamed" in msg, msg
            with pytest.raises(A.LdpcError, match="acg_ldpc_decoder_create_layered_streamed"):
                other.streamed_slab(H05)
        finally:
            other.close()
