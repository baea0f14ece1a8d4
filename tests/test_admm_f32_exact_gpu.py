"""The fp32 QP-ADMM kernels against tests/admm_ref.py in float32: word, flag and sweep count IDENTICAL on every frame whose
residual never came within the band of eps (tests/admm_f32_sets.py, qualified on the CPU by tests/test_admm_ref.py), and on
every frame without exception where the stopping rule is off.  Every fp32 instance is reached through the C ABI / its Python
mirror: the workgroup-per-frame kernel (2-, 3- and 4-pass, lean and general, decode, grid and codes instances), the
wavefront-group kernels (16, 32 and 64 lanes, the register-resident variant, the fused Monte-Carlo instance) and the streamed
engine."""
import ctypes as C
import math

import numpy as np
import pytest

import admm_f32_sets as S
import mc_detail_ref

pytestmark = pytest.mark.gpu

BLOCK_SIZES = (128, 192, 256)
COUNTERS = ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong", "sum_iters")
MC_FRAMES = 256


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


@pytest.fixture(scope="module")
def sets(oracle, matrices):
    return S.FrameSets(oracle, matrices)


@pytest.fixture(scope="module")
def pcm(A, sets):
    return {k: A.ParityCheckMatrix(v) for k, v in sets.H.items()}


def decoder(A, s, **kw):
    return A.QPADMMDecoder(s.alpha, s.mu, s.budget, s.eps, precision=A.PREC_F32, **kw)


def hold(sets, s, got, want, what):
    """got = (bits, ok, iters) of a kernel, want = (bits, ok, iters, band) of the restatement, same frames"""
    bits, ok, iters = got
    rb, rok, rit, band = want
    assert bits.shape == rb.shape and len(band) == len(iters)
    clear = sets.clear(s, band)
    banded = int((~clear).sum())
    assert banded <= 0.02 * len(band), (what, s, banded)
    w = (bits != rb).any(axis=1) & clear
    i = (iters != rit) & clear
    k = (ok != rok) & clear
    print("%s %s: %d frames, %d banded; differing: %d words, %d flags, %d sweep counts"
          % (what, s, len(band), banded, int(w.sum()), int(k.sum()), int(i.sum())))
    assert not w.any() and not k.any() and not i.any(), (what, s, np.flatnonzero(w | i | k)[:8].tolist())


def run(A, sets, pcm, s, what, rows=slice(None), **kw):
    """one fresh decoder (the environment is read when its handle is made) on set s; -> its layout and description"""
    dec = decoder(A, s, **kw)
    H = pcm[s.code]
    y = sets.frames(s.code, s.snr)[1][rows]
    got = dec.decode_batch(H, y, s.snr)
    lay, text = dec.layout(H), dec.describe(H)
    dec.close()
    hold(sets, s, got, tuple(x[rows] for x in sets.ref(s)), what)
    return lay, text


def passes_of(sets, code, L):
    """passes the workgroup-per-frame kernel needs at L threads: one thread per constraint group (a zero slot included)
    and per variable, never fewer than two"""
    col_ptr, con, coef, b = sets.problem(code)
    H = sets.H[code]
    deg = (H != 0).sum(axis=1)
    groups = int(np.maximum(deg - 2, 1)[deg > 0].sum()) + 1
    return max(2, math.ceil(groups / L), math.ceil((len(col_ptr) - 1) / L))


# ---------------------------------------------------------------------------------------------- decode instances
@pytest.mark.parametrize("s", S.MAIN + [S.make("optimalH", -2.0, *S.HIGH_GAIN)], ids=lambda s: "%s%+g_a%g" % (s.code, s.snr, s.alpha))
def test_workgroup_per_frame_auto(A, sets, pcm, s):
    """the default route of the three matrices, stopping rule on (EE instance) and off (eps = 0: every frame exact)"""
    f64 = A.QPADMMDecoder(s.alpha, s.mu, s.budget, s.eps)
    lds64 = f64.layout(pcm[s.code])["lds_bytes_per_frame"]
    f64.close()
    for eps in (s.eps, 0.0):
        se = s._replace(eps=eps)
        lay, text = run(A, sets, pcm, se, "auto")
        assert lay["lanes_per_frame"] in BLOCK_SIZES and lay["frames_per_block"] == 1 and "engine=lds" in text, (lay, text)
        assert lay["lds_bytes_per_frame"] < lds64, (lay, lds64)      # float state: the fp32 instance
        if eps > 0:
            it = sets.ref(se)[2]
            assert (it < s.budget).any() and (it == s.budget).any()
        else:
            assert (sets.ref(se)[2] == s.budget).all()


@pytest.mark.parametrize("force_l", BLOCK_SIZES)
def test_pass_instances(A, sets, pcm, monkeypatch, force_l):
    """ACG_ADMM_BLOCK_L = 128 / 192 / 256: H.txt takes 4 / 3 / 2 passes, H05 4 / 3 at 192 / 256 (128 threads would need more
    than four passes: the size is not taken).  layout() does not expose the pass count; it follows from the workgroup size."""
    monkeypatch.setenv("ACG_ADMM_BLOCK_L", str(force_l))
    reached = {}
    for s in (S.make("H", -2.0), S.make("H05", -2.0)):
        for eps in (s.eps, 0.0):
            lay, _ = run(A, sets, pcm, s._replace(eps=eps), "L=%d" % force_l)
            assert lay["lanes_per_frame"] in BLOCK_SIZES, lay
        if lay["lanes_per_frame"] == force_l:
            reached[s.code] = passes_of(sets, s.code, force_l)
    assert reached == {128: {"H": 4}, 192: {"H": 3, "H05": 4}, 256: {"H": 2, "H05": 3}}[force_l], reached


@pytest.mark.parametrize("env", ["ACG_ADMM_NO_LEAN", "ACG_ADMM_NO_QC"])
def test_general_instance(A, sets, pcm, monkeypatch, env):
    """the instance with the general paths compiled in; with ACG_ADMM_NO_QC the annealed placement (V cell != thread slot)"""
    monkeypatch.setenv(env, "1")
    s = S.make("H05", -2.0)
    for eps in (s.eps, 0.0):
        lay, _ = run(A, sets, pcm, s._replace(eps=eps), env)
        assert lay["lanes_per_frame"] in BLOCK_SIZES, lay


@pytest.mark.parametrize("L", [16, 32, 64])
def test_wavefront_groups(A, sets, pcm, L):
    """admm_fused_kernel<float, L>; 64 lanes keep the row state in registers (NGP variant) on both codes"""
    for s in (S.make("H05", -2.0), S.make("optimalH", -2.0, *S.HIGH_GAIN), S.make("H05", 1.0, eps=0.0)):
        lay, text = run(A, sets, pcm, s, "lanes=%d" % L, lanes_per_frame=L)
        assert lay["lanes_per_frame"] == L and lay["frames_per_block"] % (64 // L) == 0 and "engine=lds" in text, (lay, text)


def test_wavefront_64_lanes_row_state_in_lds(A, sets, pcm):
    """more than 12 x 64 constraint groups: admm_fused_kernel<float, 64, 0>.  This set has a frame inside the band (tests/test_admm_ref.py
    prints the census), so the skip is exercised; the other routes run it too"""
    s = S.make("regular", 0.0)
    deg = (sets.H[s.code] != 0).sum(axis=1)
    assert int(np.maximum(deg - 2, 1).sum()) > 12 * 64
    assert not sets.clear(s, sets.ref(s)[3]).all()
    lay, _ = run(A, sets, pcm, s, "lanes=64 lds", lanes_per_frame=64)
    assert lay["lanes_per_frame"] == 64, lay
    lay, _ = run(A, sets, pcm, s, "auto")
    assert lay["lanes_per_frame"] in BLOCK_SIZES, lay
    run(A, sets, pcm, s, "streamed", engine=A.ENGINE_STREAMED)
    run(A, sets, pcm, s._replace(eps=0.0), "lanes=64 lds", lanes_per_frame=64)


def test_streamed(A, sets, pcm):
    for s in (S.make("H05", -2.0), S.make("H05", -2.0, eps=0.0), S.make("mixed", -2.0), S.make("optimalH", 1.0)):
        lay, text = run(A, sets, pcm, s, "streamed", engine=A.ENGINE_STREAMED)
        assert lay["lanes_per_frame"] == 1 and "engine=streamed" in text and "f64=0" in text and "<float>" in text, (lay, text)


def test_generic_groups_and_list_tails(A, sets, pcm):
    """one- and two-variable checks (GENERIC group instance) and lists beyond the register-resident entries, on the
    workgroup-per-frame kernel and on 64 lanes"""
    H = sets.H["mixed"]
    assert {1, 2} <= set((H != 0).sum(axis=1).tolist()) and np.diff(sets.problem("mixed")[0]).max() > 6 * 4
    for s in (S.make("mixed", -2.0), S.make("mixed", -2.0, eps=0.0), S.make("small", -2.0, eps=1e-6), S.make("small", -2.0, eps=0.0)):
        lay, text = run(A, sets, pcm, s, "generic auto")
        assert lay["lanes_per_frame"] in BLOCK_SIZES and "engine=lds" in text, (lay, text)
        lay, _ = run(A, sets, pcm, s, "generic 64", lanes_per_frame=64)
        assert lay["lanes_per_frame"] == 64, lay


def test_float_symbols(A, sets, pcm):
    """float32 symbols through acg_ldpc_decode_batch_f32: q = float(2 * double(y) / var)"""
    s = S.make("H05", -2.0)
    y32 = sets.frames(s.code, s.snr)[1].astype(np.float32)
    want = sets.ref(s, y=y32, tag="y32")
    assert not all((a == b).all() for a, b in zip(want[:3], sets.ref(s)[:3]))   # other symbols, other words
    for what, kw in (("block", {}), ("lanes=32", dict(lanes_per_frame=32)), ("streamed", dict(engine=A.ENGINE_STREAMED))):
        dec = decoder(A, s, **kw)
        got = dec.decode_batch(pcm[s.code], y32, s.snr)
        dec.close()
        hold(sets, s, got, want, "y32 " + what)


@pytest.mark.parametrize("F", [1, 63, 65, S.FRAMES])
def test_ragged_batches(A, sets, pcm, F):
    s = S.make("H05", -2.0)
    run(A, sets, pcm, s, "block F=%d" % F, rows=slice(0, F))
    run(A, sets, pcm, s, "streamed F=%d" % F, rows=slice(0, F), engine=A.ENGINE_STREAMED)
    run(A, sets, pcm, s, "lanes=16 F=%d" % F, rows=slice(0, F), lanes_per_frame=16)


def extreme_symbols(sets, s):
    y = sets.frames(s.code, s.snr)[1][:48].copy()
    n = y.shape[1]
    vals = [0.0, -0.0, 1e-320, 1e30, -1e30, 1e39, -1e39, np.inf, -np.inf, np.nan]
    for f, v in enumerate(vals):
        y[f, (7 * f + 3) % n] = v
        y[f, (11 * f + 100) % n] = v
    y[10, 5], y[10, 6] = 1e39, -1e39            # both infinities in one frame
    y[11, 5], y[11, 200] = np.nan, 1e30
    y[12, :4] = [0.0, -0.0, 1e-320, -1e-320]
    return y


def test_extreme_symbols(A, sets, pcm):
    """zeros of both signs, a denormal that underflows in the fp32 q, 1e30, 1e39 (an infinite fp32 q), infinities and NaN:
    the comparisons of qp_admm.h:140-141,156-157 pass a NaN on, and so do the kernels"""
    s = S.make("H05", -2.0)
    y = extreme_symbols(sets, s)
    want = sets.ref(s, y=y, tag="extreme")
    for what, kw in (("block", {}), ("lanes=32", dict(lanes_per_frame=32)), ("streamed", dict(engine=A.ENGINE_STREAMED))):
        dec = decoder(A, s, **kw)
        got = dec.decode_batch(pcm[s.code], y, s.snr)
        dec.close()
        hold(sets, s, got, want, "extreme " + what)


# ---------------------------------------------------------------------------------------------- Monte-Carlo counters
def counters_of(sets, s, y, sent, want):
    """classification of the restatement's output on the CPU (IsCodeword, then equality with the sent word)"""
    bits, ok, iters, band = want
    assert sets.clear(s, band).all(), "a counter cannot skip a frame: choose frames without a banded one"
    c, _, _ = mc_detail_ref.mc_detail(y, mc_detail_ref.pack_bits(bits), ok, iters, sent, sets.H[s.code])
    return tuple(c[k] for k in COUNTERS)


def ints(r):
    return tuple(getattr(r, k) for k in COUNTERS)


def host_frames(sets, code, snr, count=MC_FRAMES):
    """the frames run_experiment(noise="host") makes: frame g sends cws[g % len] through mt19937(g + 1)"""
    G, ok = sets.oracle.get_orthogonal(sets.H[code])
    assert ok
    cws = sets.oracle.gen_codewords(G, 239, 64)
    sent = cws[np.arange(count) % len(cws)]
    return cws, sent, sets.oracle.transmit_frames(sent, snr, first_seed=1)


MC_ROUTES = [("block", {}), ("lanes=32", dict(lanes_per_frame=32)), ("streamed", "streamed")]


def test_mc_host_noise(A, sets, pcm):
    s = S.make("H05", -2.0)
    cws, sent, y = host_frames(sets, s.code, s.snr)
    want = counters_of(sets, s, y, sent, sets.ref(s, y=y, tag="mc-host"))
    assert 0 < want[0] < MC_FRAMES and want[6] < MC_FRAMES * s.budget
    for what, kw in MC_ROUTES:
        dec = decoder(A, s, **(dict(engine=A.ENGINE_STREAMED) if kw == "streamed" else kw))
        r = A.run_experiment(dec, cws, pcm[s.code], s.snr, frames=MC_FRAMES, noise="host")
        dec.close()
        assert ints(r) == want, (what, r, want)


def test_mc_device_noise(A, sets, pcm):
    """the symbols of acg_ldpc_awgn_dev restated, against the fused Monte-Carlo instance (32 lanes: noise, decode and
    classification in one kernel) and the block route (AWGN kernel -> decode -> classify)"""
    import torch
    from acg_alp_ldpc_amd._lib import check, lib
    from mc_decode_path import mc_cfg, sent_words
    s = S.make("H05", -2.0)
    H = pcm[s.code]
    cws = host_frames(sets, s.code, s.snr)[0]
    first, seed = 1000, 99
    dec = decoder(A, s)
    h, _ = dec.handle(H)
    yd = torch.empty((MC_FRAMES, H.n), dtype=torch.float32, device="cuda")
    cfg = mc_cfg(A, cws, s.snr, MC_FRAMES, first, seed, "device")
    check(lib().acg_ldpc_awgn_dev(h, C.byref(cfg), yd.data_ptr(), None))
    dec.sync(H)
    y = yd.cpu().numpy()
    assert y.dtype == np.float32
    sent = sent_words(cws, H.n, first, MC_FRAMES)
    want = counters_of(sets, s, y, sent, sets.ref(s, y=y, tag="mc-device"))
    assert 0 < want[0] < MC_FRAMES
    r = A.run_experiment(dec, cws, H, s.snr, frames=MC_FRAMES, first_frame=first, noise="device", seed=seed)
    dec.close()
    assert ints(r) == want, ("block", r, want)
    dec = decoder(A, s, lanes_per_frame=32)
    r = A.run_experiment(dec, cws, H, s.snr, frames=MC_FRAMES, first_frame=first, noise="device", seed=seed)
    dec.close()
    assert ints(r) == want, ("lanes=32 fused", r, want)


def test_mc_grid(A, sets, pcm):
    """acg_ldpc_mc_run_grid: each point restated at float(alpha), float(mu) with its own inv table"""
    code, snr = "optimalH", -2.0
    cws, sent, y = host_frames(sets, code, snr)
    points = [S.PARAMS[code], S.HIGH_GAIN]
    dec = A.QPADMMDecoder(0.3, 0.9, S.BUDGET, 1e-5, precision=A.PREC_F32)      # (its own alpha, mu do not apply)
    assert "mc_grid=single-launch" in dec.describe(pcm[code])
    got = A.run_experiment_grid(dec, cws, pcm[code], snr, [p[0] for p in points], [p[1] for p in points], frames=MC_FRAMES,
                                noise="host")
    dec.close()
    seen = []
    for (alpha, mu), r in zip(points, got):
        s = S.make(code, snr, alpha, mu)
        want = counters_of(sets, s, y, sent, sets.ref(s, y=y, tag="mc-host"))
        assert ints(r) == want, (alpha, mu, r, want)
        seen.append(want)
    assert seen[0] != seen[1]


def test_mc_codes(A, sets, pcm):
    """acg_ldpc_mc_run_codes: two codes of one shape in one launch, each equal to its own restatement"""
    snr = -2.0
    alpha, mu = S.PARAMS["H05"]
    dec = A.QPADMMDecoder(alpha, mu, S.BUDGET, 1e-5, precision=A.PREC_F32)
    ev = A.CodesEvaluator(dec)
    frames = {code: host_frames(sets, code, snr) for code in ("H05", "optimalH")}
    got = ev.run([(pcm[code], frames[code][0]) for code in frames], snr, frames=MC_FRAMES, noise="host")
    text = ev.describe()
    ev.close()
    dec.close()
    assert "mc_codes=single-launch" in text and "per_code=0" in text, text
    for code, r in zip(frames, got):
        s = S.make(code, snr, alpha, mu)
        cws, sent, y = frames[code]
        want = counters_of(sets, s, y, sent, sets.ref(s, y=y, tag="mc-host"))
        assert ints(r) == want, (code, r, want)
