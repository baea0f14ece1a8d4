"""GPU: the fixed-point layered min-sum engine (bp_layered_q_kernel behind acg_ldpc_decoder_create_quantized /
QuantizedMinSumDecoder) against its numpy restatement tests/layered_q_ref.py over the sets of ParityCheckMatrix.layers_wide():
word, flag and exit iteration of EVERY frame identical, nothing tolerated — every value is an integer.  Codes, frames, SNRs and
quantisers are those of tests/layered_q_cases.py (tests/test_layered_q.py asserts on the CPU that the restatement decodes some
frames and fails others on each)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import layered_q_cases as Q
import mc_detail_ref as R
from layered_q_ref import layered_minsum_q, quantize
from mc_decode_path import decode_device_noise, sent_words
from test_layered_block_gpu import _assert_same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "bp_layered_q_kernel"


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


def _dec(A, it, qname="default", L=0, ee=True):
    return A.QuantizedMinSumDecoder(it, quant=A.QuantConfig(*Q.QUANTS[qname]), lanes_per_frame=L, early_exit=ee)


def _decode(A, c, y, it, qname="default", L=0, ee=True):
    dec = _dec(A, it, qname, L, ee)
    try:
        out = dec.decode_batch(c.H, y, c.snr)
        d = dec.describe(c.H)
        assert d.startswith("minsum") and "kernel=%s " % KERNEL in d and "schedule=layered" in d, d
        want_L = L if L else min(x for x in (64, 128, 256, 512, 1024) if x >= min(c.width, 1024))
        assert "lanes_per_frame=%d " % want_L in d, d
        return out
    finally:
        dec.close()


# ---------------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("qname", sorted(Q.QUANTS))
@pytest.mark.parametrize("name", sorted(Q.CASES))
def test_q_equals_restatement(A, name, qname):
    """every case x quantiser at lanes_per_frame 0, 64, 256 and 1024: identical to layered_minsum_q"""
    c = Q.case(A, name)
    want = c.ref(qname)
    for L in (0, 64, 256, 1024):
        _assert_same(_decode(A, c, c.y, c.iters, qname, L), want, (name, qname, L))
    if qname == "default":
        assert 0 < want[1].sum() < len(want[1]), (name, int(want[1].sum()))      # decoded and failed frames, both exits covered
    assert ((want[0][want[1] == 1] @ c.Hm.T.astype(np.int64)) % 2 == 0).all()


@pytest.mark.parametrize("name", sorted(Q.CASES))
def test_q_batch_shapes_and_float_symbols(A, name):
    """1 and 63 frames on one handle (fewer frames than workgroups), then float32 symbols — the (double) y * (2 / sigma^2) LLR
    path through acg_ldpc_decode_batch_f32 — and the layout report: (n + 1 padded to 8) * 2 + E padded to 4 + 4 * nwords"""
    c = Q.case(A, name)
    want = c.ref("default")
    dec = _dec(A, c.iters)
    try:
        for F in (1, 63):
            _assert_same(dec.decode_batch(c.H, c.y[:F], c.snr), tuple(a[:F] for a in want), (name, "frames", F))
        _assert_same(dec.decode_batch(c.H, c.y.astype(np.float32), c.snr), c.ref("default", symbols_f32=True), (name, "float32 symbols"))
        assert dec.live_handles() == 1 and dec.name() == "QMS"
        assert A.lib().acg_ldpc_decoder_name(dec.handle(c.H)[0]) == b"QMS"
        lay = dec.layout(c.H)
        E = int(c.Hm.sum())
        lds = ((c.n + 1 + 7) & ~7) * 2 + ((E + 3) & ~3) + 4 * ((c.n + 31) // 32)
        assert (lay["lds_bytes_per_frame"], lay["frames_per_block"]) == (lds, 1) and lay["grid_blocks"] >= 1, (lay, lds)
        d = dec.describe(c.H)
        assert "quant=llr_step:0.5,ch_bits:6,msg_bits:6,post_bits:8,scale_num:1,scale_shift:0,offset:1" in d, d
        assert "sets=%d " % len(c.layers) in d and "largest_set=%d " % c.width in d and "lds_block=%d " % lds in d, d
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------- 2. fixed work, 0 and 1 iterations
@pytest.mark.parametrize("name", sorted(Q.CASES))
def test_q_fixed_work_and_short_runs(A, name):
    """early_exit = 0 returns what early_exit = 1 returns; max_iter = 0: every frame fails with 0 iterations; max_iter = 1"""
    c = Q.case(A, name)
    _assert_same(_decode(A, c, c.y, c.iters, ee=False), c.ref("default"), (name, "fixed work"))
    for it in (0, 1):
        want = c.ref("default", it)
        for ee in (True, False):
            _assert_same(_decode(A, c, c.y, it, ee=ee), want, (name, it, "early exit" if ee else "fixed work"))
    b0, ok0, it0 = c.ref("default", 0)
    assert not ok0.any() and not b0.any() and (it0 == 0).all()


# --------------------------------------------------------------------------------------------------------- 3. extreme symbols
def test_q_extreme_symbols(A):
    """an all-zero frame: word 0, ok 1, 1 iteration.  +-1e30, +-inf and NaN among ordinary symbols: the restatement's answer,
    for double and for float symbols, for the default and the saturating quantiser"""
    c = Q.case(A, "H05")
    z = _decode(A, c, np.zeros((3, c.n)), c.iters)
    assert not z[0].any() and (z[1] == 1).all() and (z[2] == 1).all()
    rng = np.random.default_rng(11)
    y = c.y[:120].copy()
    special = np.array([1e30, -1e30, np.inf, -np.inf, np.nan])
    for f in range(len(y)):
        k = 1 + f % 9
        y[f, rng.choice(c.n, k, replace=False)] = rng.choice(special, k)
    y[0, :] = np.nan
    y[1, :] = -np.inf
    for qname in ("default", "saturating"):
        for f32 in (False, True):
            ys = y.astype(np.float32) if f32 else y
            want = layered_minsum_q(c.Hm, c.layers, ys, c.snr, c.iters, Q.QUANTS[qname], symbols_f32=f32)
            _assert_same(_decode(A, c, ys, c.iters, qname), want, ("extreme symbols", qname, "float32" if f32 else "float64"))
            if qname == "default" and not f32:
                assert 0 < want[1].sum() < len(y)
                assert want[1][0] == 1 and not want[0][0].any()          # all NaN = all zero


# ------------------------------------------------------------------------------------------------------------ 4. the quantiser
@pytest.mark.parametrize("f64", [True, False])
def test_q_debug_quantize_equals_numpy(A, f64):
    """4096 values at 0 dB (sigma^2 = 1/2: llr = 4 y exactly, t = 8 y for llr_step 0.5): every half-integer of t within and just
    beyond the range, +-Cmax +- 1, zeros of both signs, the specials, random values; then random values at -2 dB with a step
    whose inverse is not a binary fraction"""
    rng = np.random.default_rng(5)
    halves = (np.arange(-40, 40) + 0.5) / 8.0
    edges = np.array([30, 31, 32, -30, -31, -32, 30.5, 31.5, -30.5, -31.5, 0.0, -0.0]) / 8.0
    special = np.array([1e30, -1e30, np.inf, -np.inf, np.nan, 1e-30, -1e-30, 3.4e38, -3.4e38])
    y = np.concatenate([halves, edges, special])
    y = np.concatenate([y, rng.normal(0, 2.0, 4096 - len(y))]).astype(np.float64 if f64 else np.float32)
    assert len(y) == 4096
    for snr, quant in ((0.0, Q.QUANTS["default"]), (0.0, Q.QUANTS["saturating"]), (-2.0, (0.3, 7, 5, 10, 1, 0, 0))):
        out = np.full(len(y), -777, dtype=np.int16)
        q = A._lib.Quant(*quant)
        rc = A.lib().acg_ldpc_debug_quantize(y.ctypes.data, 1 if f64 else 0, len(y), snr, C.byref(q), out.ctypes.data)
        assert rc == 0, A.lib().acg_ldpc_last_error()
        want = quantize(y, snr, quant, symbols_f32=not f64)
        bad = np.nonzero(out != want)[0]
        assert len(bad) == 0, (snr, quant, [(float(y[i]), int(out[i]), int(want[i])) for i in bad[:8]])
        if snr == 0.0 and quant[0] == 0.5:
            t = 8.0 * halves                                                # exact: round half to even
            cm = (1 << (quant[1] - 1)) - 1
            assert (out[:len(halves)] == np.clip(np.rint(t), -cm, cm)).all()


# -------------------------------------------------------------------------------------------------------------- 5. Monte-Carlo
def test_q_monte_carlo_counters(A):
    """run_experiment and run_experiment_detail with device noise on 1024 frames of H05 = the counters tests/mc_detail_ref.py
    forms from acg_ldpc_awgn_dev's symbols decoded through this decoder's own decode_batch_dev"""
    c = Q.case(A, "H05")
    F, first, seed = 1024, (1 << 33) + 5, 2
    cws = c.cws[:7]
    dec = _dec(A, c.iters)
    try:
        y, words, ok, it = decode_device_noise(A, dec, c.H, cws, c.snr, F, first, seed)
        want, events, rows = R.mc_detail(y, words, ok, it, sent_words(cws, c.n, first, F), c.Hm, first_frame=first, cap=5)
        got = A.run_experiment(dec, cws, c.H, c.snr, frames=F, first_frame=first, noise="device", seed=seed)
        det = A.run_experiment_detail(dec, cws, c.H, c.snr, frames=F, first_frame=first, noise="device", seed=seed, cap=5)
        assert KERNEL in dec.describe(c.H)
    finally:
        dec.close()
    fields = ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong", "sum_iters")
    assert tuple(getattr(got, f) for f in fields) == tuple(want[f] for f in fields), (got, want)
    assert tuple(getattr(det, f) for f in fields) == tuple(want[f] for f in fields), (det, want)
    for f in ("word_frames", "bit_errors", "noncodeword_frames", "n_events", "n_stored"):
        assert getattr(det, f) == want[f], (f, getattr(det, f), want[f])
    assert list(det.events["frame"]) == list(events["frame"])
    assert 0 < want["correct"] < F


# ----------------------------------------------------------------------------------------------------------------- 6. refusals
def test_q_refusals_through_the_python_class(A):
    """each raises LdpcError with its message and leaves no handle"""
    c = Q.case(A, "H05")
    Hm33 = np.zeros((2, 40), dtype=np.uint8)
    Hm33[0, :33] = 1
    Hm33[1, 30:] = 1
    big = np.zeros((2, 82000), dtype=np.uint8)             # 164 KB of int16 posteriors alone
    big[0, :32] = 1
    big[1, -32:] = 1
    sum_product = A.QuantizedMinSumDecoder(10)
    sum_product._algo = A._lib.ALGO_BP
    for what, dec, H, word in (("flooding", A.QuantizedMinSumDecoder(10, schedule=A.SCHEDULE_FLOODING), c.H, "schedule"),
                               ("sum-product", sum_product, c.H, "algo"),
                               ("fp16", A.QuantizedMinSumDecoder(10, precision=A.PREC_F16), c.H, "precision"),
                               ("streamed", A.QuantizedMinSumDecoder(10, engine=A.ENGINE_STREAMED), c.H, "engine"),
                               ("32 lanes", A.QuantizedMinSumDecoder(10, lanes_per_frame=32), c.H, "lanes_per_frame"),
                               ("degree 33", A.QuantizedMinSumDecoder(10), Hm33, "degree above 32"),
                               ("frame beyond LDS", A.QuantizedMinSumDecoder(10), big, "does not fit in LDS"),
                               ("frame beyond LDS, 1024", A.QuantizedMinSumDecoder(10, lanes_per_frame=1024), big, "does not fit in LDS"),
                               ("msg_bits 9", A.QuantizedMinSumDecoder(10, quant=dict(msg_bits=9, post_bits=12)), c.H, "invalid quantiser"),
                               ("offset above Rmax", A.QuantizedMinSumDecoder(10, quant=dict(offset=32)), c.H, "invalid quantiser")):
        with pytest.raises(A.LdpcError, match=word):
            dec.handle(H)
        assert dec.live_handles() == 0, what
    dec = A.QuantizedMinSumDecoder(10)
    try:
        with pytest.raises(A.LdpcError, match="QP-ADMM"):
            A.run_experiment_grid(dec, None, c.H, c.snr, [1.0], [0.5], frames=64, noise="device")
        for L in (64, 128, 256, 512, 1024):                 # and what is accepted
            ok = A.QuantizedMinSumDecoder(10, lanes_per_frame=L)
            assert "lanes_per_frame=%d " % L in ok.describe(c.H)
            ok.close()
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------------------ 7. C++ mirror
def test_q_cxx_mirror_decodes(A, tmp_path):
    """tests/cxx_quant_check.cpp, built as tests/test_cxx_adaptor.py builds its program: one noiseless and one hopeless H05 frame
    through acg_ldpc::QuantizedMinSumDecoder"""
    exe = Q.build_cxx_check(tmp_path)
    out = subprocess.run([exe, os.path.join(ROOT, "data", "H05.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "m=160 n=280 E=860 quant=0.5,6,6,8,1,0,1 check=0 sizeof=32" in out.stdout
    assert "QMS noiseless ok=1 size=280 diff=0" in out.stdout and "QMS hopeless ok=0 size=0" in out.stdout
    assert "kernel=%s " % KERNEL in out.stdout
