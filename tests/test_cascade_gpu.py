"""GPU: two-stage decoding (acg_ldpc_cascade_*).  The cascade must equal the composition its header describes — stage 0 alone on
every frame (through the borrowed handle of acg_ldpc_cascade_stage), stage 1 alone on the numpy-compacted failed rows, the
results put back on the host — in word, flag, iteration count and stage of EVERY frame, nothing tolerated.  Then the edges
(K = 0, K = F, 0 and 1 frames, chunk boundaries), the host entries, the Monte-Carlo run in both noise modes, the refusals and
the driver's extra rows.  Codes and frames: tests/layered_q_cases.py (300-400 frames of host-noise symbols each)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import layered_q_cases as Q
from mc_decode_path import mc_cfg, sent_words
from mc_detail_ref import mc_detail, pack_bits, unpack_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data")
SEVEN = ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong", "sum_iters")


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


# name -> (case of layered_q_cases, SNR in dB or None = the case's own, first decoder, second decoder)
def _pairs(A):
    lay = A.SCHEDULE_LAYERED
    return {
        "ms10_bp50": ("H05", -2.0, lambda: A.MinSumDecoder(10, 0.75), lambda: A.BeliefPropagationDecoder(50)),
        "bp10_admm200": ("H05", -2.0, lambda: A.BeliefPropagationDecoder(10), lambda: A.QPADMMDecoder(1.2, 0.55, 200, fast_setup=True)),
        "qms5_layered_spa25": ("H05", -2.0, lambda: A.QuantizedMinSumDecoder(5), lambda: A.BeliefPropagationDecoder(25, schedule=lay)),
        "layered_ms_f16_streamed_bp50": ("H05", -2.0, lambda: A.MinSumDecoder(5, 0.75, schedule=lay, precision=A.PREC_F16),
                                         lambda: A.BeliefPropagationDecoder(50, engine=A.ENGINE_STREAMED)),
        "qc2x10z300_qms3_layered_ms25": ("qc2x10z300", 3.0, lambda: A.QuantizedMinSumDecoder(3, lanes_per_frame=256),
                                         lambda: A.MinSumDecoder(25, schedule=lay, lanes_per_frame=256)),
        "diag10_qms1_ms5": ("diag10", None, lambda: A.QuantizedMinSumDecoder(1), lambda: A.MinSumDecoder(5)),
        "H_ms3_bp20": ("H", 0.0, lambda: A.MinSumDecoder(3), lambda: A.BeliefPropagationDecoder(20)),
    }


def _symbols(A, case, snr):
    """the case's sent words at `snr` through the host generator (the case's own symbols where the SNR is the case's)"""
    c = Q.case(A, case)
    if snr is None or snr == c.snr:
        return c, c.snr, c.y
    return c, snr, A.transmit_frames(c.cws, snr)


def _decode_dev(fn, h, y, snr, n, want_iters=True, want_stage=None, stream=None, extra=1):
    """fn = acg_ldpc_decode_batch_dev (want_stage None) or acg_ldpc_cascade_decode_batch_dev on host symbols y [F, n] (float64 or
    float32) -> words [F, nw], ok, iters or None, stage or None.  The device outputs are `extra` rows longer than F and filled
    with sentinels: rows past F, and outputs handed over as NULL, must keep them."""
    import torch
    from acg_alp_ldpc_amd._lib import check
    F = y.shape[0]
    nw = (n + 31) // 32
    yd = torch.from_numpy(np.ascontiguousarray(y)).cuda() if F else torch.zeros(8, dtype=torch.float64, device="cuda")
    bits = torch.full((F + extra, nw), -1, dtype=torch.int32, device="cuda")
    ok = torch.full((F + extra,), 7, dtype=torch.uint8, device="cuda")
    it = torch.full((F + extra,), -7, dtype=torch.int32, device="cuda")
    st = torch.full((F + extra,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    args = [h, yd.data_ptr() if F else None, 1 if y.dtype == np.float64 else 0, F, float(snr), bits.data_ptr(), ok.data_ptr(),
            it.data_ptr() if want_iters else None]
    if want_stage is not None:
        args.append(st.data_ptr() if want_stage else None)
    check(fn(*args, stream))
    torch.cuda.synchronize()
    assert (bits[F:] == -1).all() and (ok[F:] == 7).all() and (it[F:] == -7).all() and (st[F:] == 9).all(), "a row past the batch was written"
    if not want_iters:
        assert (it == -7).all()
    if not want_stage:
        assert (st == 9).all()
    return (bits.cpu().numpy().view(np.uint32)[:F], ok.cpu().numpy()[:F], it.cpu().numpy()[:F] if want_iters else None,
            st.cpu().numpy()[:F] if want_stage else None)


def _stage_alone(A, cas, H, stage, y, snr):
    return _decode_dev(A.lib().acg_ldpc_decode_batch_dev, cas.stage_handle(H, stage), y, snr, H.n)[:3]


def _compose(A, cas, H, y, snr):
    """the header's semantics, by hand -> (words, ok, iters, stage), K"""
    w, ok, it = _stage_alone(A, cas, H, 0, y, snr)
    fail = np.flatnonzero(ok == 0)
    w, ok, it = w.copy(), ok.copy(), it.copy()
    stage = np.ones(len(ok), dtype=np.uint8)
    if len(fail):
        w2, ok2, it2 = _stage_alone(A, cas, H, 1, np.ascontiguousarray(y[fail]), snr)
        w[fail], ok[fail], it[fail], stage[fail] = w2, ok2, it2, 2
    return (w, ok, it, stage), len(fail)


def _cascade_dev(A, cas, H, y, snr, **kw):
    h, _ = cas.handle(H)
    kw.setdefault("want_stage", True)
    return _decode_dev(A.lib().acg_ldpc_cascade_decode_batch_dev, h, y, snr, H.n, **kw)


def _same(got, want, ctx):
    for k, what in enumerate(("words", "ok", "iters", "stage")):
        if want[k] is None or got[k] is None:
            continue
        bad = got[k] != want[k]
        bad = bad.any(axis=1) if bad.ndim == 2 else bad
        if bad.any():
            f = int(np.flatnonzero(bad)[0])
            pytest.fail("%s: %s of %d of %d frames differ; first: frame %d, cascade %s, composition %s (stage %s)"
                        % (ctx, what, int(bad.sum()), len(bad), f, got[k][f], want[k][f], want[3][f] if want[3] is not None else "?"))


# ---------------------------------------------------------------------------- 1. equality with the composition
@pytest.mark.parametrize("pair", ["ms10_bp50", "bp10_admm200", "qms5_layered_spa25", "layered_ms_f16_streamed_bp50",
                                  "qc2x10z300_qms3_layered_ms25", "diag10_qms1_ms5", "H_ms3_bp20"])
def test_cascade_equals_the_two_handles_run_by_hand(A, pair):
    import torch
    case, snr, first, second = _pairs(A)[pair]
    c, snr, y64 = _symbols(A, case, snr)
    cas = A.CascadeDecoder(first(), second())
    try:
        assert cas.name() == A.lib().acg_ldpc_cascade_name(cas.handle(c.H)[0]).decode()
        for y in (y64, y64.astype(np.float32)):
            want, K = _compose(A, cas, c.H, y, snr)
            print("%s %s: K = %d of %d frames" % (pair, y.dtype, K, len(y)))
            assert 0 < K < len(y), "the pair does not exercise both stages: K = %d of %d" % (K, len(y))
            _same(_cascade_dev(A, cas, c.H, y, snr), want, (pair, y.dtype))
            assert cas.last_call(c.H)[0] == K == int((want[3] == 2).sum())
            s = torch.cuda.Stream()
            _same(_cascade_dev(A, cas, c.H, y, snr, stream=s.cuda_stream), want, (pair, y.dtype, "caller's stream"))
            _same(_cascade_dev(A, cas, c.H, y, snr, want_iters=False, want_stage=False), want, (pair, y.dtype, "iters and stage NULL"))
            _same(_cascade_dev(A, cas, c.H, y, snr, want_iters=False), want, (pair, y.dtype, "iters NULL"))
        d = cas.describe(c.H)
        assert d.startswith("cascade " + cas.name() + " | first: ") and " | second: " in d and "last_second_frames=%d" % K in d
    finally:
        cas.close()


# ------------------------------------------------------------------------------------------------------ 2. edges
def test_no_frame_fails_the_first_stage(A):
    c, snr, y = _symbols(A, "H05", 6.0)
    cas = A.CascadeDecoder(A.BeliefPropagationDecoder(50), A.MinSumDecoder(5))
    try:
        alone = _stage_alone(A, cas, c.H, 0, y, snr)
        assert (alone[1] == 1).all()
        got = _cascade_dev(A, cas, c.H, y, snr)
        _same(got, alone + (np.ones(len(y), dtype=np.uint8),), "K = 0")
        k, ms0, ms1 = cas.last_call(c.H)
        assert k == 0 and ms0 > 0 and ms1 == 0
    finally:
        cas.close()


def test_every_frame_fails_the_first_stage(A):
    c, snr, y = _symbols(A, "H05", -2.0)
    cas = A.CascadeDecoder(A.BeliefPropagationDecoder(0), A.BeliefPropagationDecoder(50))
    try:
        assert (_stage_alone(A, cas, c.H, 0, y, snr)[1] == 0).all()
        alone = _stage_alone(A, cas, c.H, 1, y, snr)
        assert 0 < alone[1].sum() < len(y)
        got = _cascade_dev(A, cas, c.H, y, snr)
        _same(got, alone + (np.full(len(y), 2, dtype=np.uint8),), "K = F")
        k, _, ms1 = cas.last_call(c.H)
        assert k == len(y) and ms1 > 0
    finally:
        cas.close()


def test_zero_and_one_frame(A):
    c, snr, y = _symbols(A, "H05", -2.0)
    cas = A.CascadeDecoder(A.MinSumDecoder(10, 0.75), A.BeliefPropagationDecoder(50))
    try:
        want, _ = _compose(A, cas, c.H, y, snr)
        got = _cascade_dev(A, cas, c.H, y[:0], snr)     # nothing launched: every sentinel survives (checked inside)
        assert len(got[1]) == 0 and cas.last_call(c.H)[0] == 0
        one_of_each = [int(np.flatnonzero(want[3] == s)[0]) for s in (1, 2)]
        for f in one_of_each:
            _same(_cascade_dev(A, cas, c.H, y[f:f + 1], snr), tuple(x[f:f + 1] for x in want), ("one frame", f))
            assert cas.last_call(c.H)[0] == int(want[3][f] == 2)
    finally:
        cas.close()


def test_chunked_call_equals_the_unchunked_one(A, monkeypatch):
    c, snr, y = _symbols(A, "H05", -2.0)
    assert len(y) == 400
    cas = A.CascadeDecoder(A.MinSumDecoder(10, 0.75), A.BeliefPropagationDecoder(50))
    try:
        whole = _cascade_dev(A, cas, c.H, y, snr)
        assert "chunk=400 " in cas.describe(c.H)
        monkeypatch.setenv("ACG_CASCADE_CHUNK", "100")
        for yy in (y, y[:399], y.astype(np.float32)[:301]):   # four full chunks; a last chunk of 99; of one frame
            ref = whole if yy.dtype == np.float64 else _compose(A, cas, c.H, yy, snr)[0]
            _same(_cascade_dev(A, cas, c.H, yy, snr), tuple(x[:len(yy)] for x in ref), ("chunks of 100", len(yy)))
            assert "chunk=100 " in cas.describe(c.H)
            assert cas.last_call(c.H)[0] == int((ref[3][:len(yy)] == 2).sum())
    finally:
        cas.close()


# ------------------------------------------------------------------------------------------------ 3. host entries
@pytest.mark.parametrize("pair", ["ms10_bp50", "diag10_qms1_ms5"])
def test_host_entries_equal_the_device_entry(A, pair):
    case, snr, first, second = _pairs(A)[pair]
    c, snr, y64 = _symbols(A, case, snr)
    cas = A.CascadeDecoder(first(), second())
    try:
        for y in (y64, y64.astype(np.float32)):
            w, ok, it, st = _cascade_dev(A, cas, c.H, y, snr)
            bits, hok, hit, hst = cas.decode_batch(c.H, y, snr)
            assert bits.dtype == np.uint8 and (bits == unpack_bits(w, c.n)).all()
            assert (hok == ok).all() and (hit == it).all() and (hst == st).all()
            assert cas.last_call(c.H)[0] == int((st == 2).sum())
        w, ok, it, st = _cascade_dev(A, cas, c.H, y64, snr)
        for sel in (st == 1, (st == 2) & (ok == 1), (st == 2) & (ok == 0)):   # decode(): one frame of each kind there is
            for f in np.flatnonzero(sel)[:1]:
                word, good = cas.decode(c.H, y64[f], snr)
                assert good == bool(ok[f])
                assert (word == unpack_bits(w[f:f + 1], c.n)[0]).all() if good else len(word) == 0
    finally:
        cas.close()


# -------------------------------------------------------------------------------------------------- 4. Monte-Carlo
def _counters(r):
    return {f: int(getattr(r, f)) for f in SEVEN}


def _mc_pair(A):
    return A.CascadeDecoder(A.MinSumDecoder(10, 0.75), A.BeliefPropagationDecoder(50))


def test_mc_host_noise(A):
    from acg_alp_ldpc_amd._lib import McResult, check
    c, snr, y = _symbols(A, "H05", -2.0)
    F = len(y)
    cas = _mc_pair(A)
    alone = A.BeliefPropagationDecoder(50)
    try:
        total, first, ex = A.run_experiment_cascade(cas, c.cws, c.H, snr, noise="host")
        bits, ok, it, st = cas.decode_batch(c.H, y, snr)
        want, _, _ = mc_detail(y, pack_bits(bits), ok, it, c.cws, c.Hm)
        assert _counters(total) == {f: want[f] for f in SEVEN}
        # first = acg_ldpc_mc_run on the stage-0 handle
        cfg, r0 = mc_cfg(A, c.cws, snr, F, 0, 1, "host"), McResult()
        check(A.lib().acg_ldpc_mc_run(cas.stage_handle(c.H, 0), C.byref(cfg), C.byref(r0)))
        assert _counters(first) == _counters(r0)
        assert 0 < ex["second_frames"] < F and ex["second_frames"] == int((st == 2).sum())
        assert ex["second_frames"] == first.total - first.correct - first.pseudo
        assert total.correct == first.correct + ex["second_correct"] and total.pseudo == first.pseudo + ex["second_pseudo"]
        assert ex["second_sum_iters"] == int(it[st == 2].sum())
        assert total.correct > first.correct and ex["second_kernel_ms"] > 0 and first.kernel_ms > 0
        assert abs(total.kernel_ms - first.kernel_ms - ex["second_kernel_ms"]) < 1e-3
        # a frame is wrong in the cascade only if stage 0 returned a pseudo-codeword for it or stage 1 gets it wrong
        r1 = A.run_experiment(alone, c.cws, c.H, snr, noise="host")
        assert total.total - total.correct <= first.pseudo + (r1.total - r1.correct)
    finally:
        cas.close()
        alone.close()


def test_mc_device_noise(A, monkeypatch):
    import torch
    from acg_alp_ldpc_amd._lib import check
    c = Q.case(A, "H05")
    snr, F, seed, first_frame = -2.0, 400, 11, 1000
    cas = _mc_pair(A)
    try:
        whole = A.run_experiment_cascade(cas, c.cws, c.H, snr, frames=F, first_frame=first_frame, noise="device", seed=seed)
        key = lambda r: (_counters(r[0]), _counters(r[1]), {k: v for k, v in r[2].items() if k != "second_kernel_ms"})
        # two shards merged
        a = A.run_experiment_cascade(cas, c.cws, c.H, snr, frames=150, first_frame=first_frame, noise="device", seed=seed)
        b = A.run_experiment_cascade(cas, c.cws, c.H, snr, frames=F - 150, first_frame=first_frame + 150, noise="device", seed=seed)
        assert key(A.merge_cascade_results(a, b)) == key(whole)
        # the chunked run
        monkeypatch.setenv("ACG_CASCADE_CHUNK", "64")
        assert key(A.run_experiment_cascade(cas, c.cws, c.H, snr, frames=F, first_frame=first_frame, noise="device", seed=seed)) == key(whole)
        monkeypatch.delenv("ACG_CASCADE_CHUNK")
        # the classification of the device decode on acg_ldpc_awgn_dev's symbols
        yd = torch.empty((F, c.n), dtype=torch.float32, device="cuda")
        cfg = mc_cfg(A, c.cws, snr, F, first_frame, seed, "device")
        check(A.lib().acg_ldpc_awgn_dev(cas.stage_handle(c.H, 0), C.byref(cfg), yd.data_ptr(), None))
        torch.cuda.synchronize()
        y = yd.cpu().numpy()
        w, ok, it, st = _cascade_dev(A, cas, c.H, y, snr)
        want, _, _ = mc_detail(y, w, ok, it, sent_words(c.cws, c.n, first_frame, F), c.Hm)
        assert _counters(whole[0]) == {f: want[f] for f in SEVEN}
        assert whole[2]["second_frames"] == int((st == 2).sum()) and 0 < whole[2]["second_frames"] < F
        assert whole[2]["second_sum_iters"] == int(it[st == 2].sum())
        w0, ok0, it0 = _stage_alone(A, cas, c.H, 0, y, snr)
        want0, _, _ = mc_detail(y, w0, ok0, it0, sent_words(c.cws, c.n, first_frame, F), c.Hm)
        assert _counters(whole[1]) == {f: want0[f] for f in SEVEN}
    finally:
        cas.close()


def test_mc_with_qpadmm_as_second_stage(A):
    """QP-ADMM's flag is not the zero syndrome: the merged outputs are classified with the parity checks"""
    c, snr, y = _symbols(A, "H05", -2.0)
    cas = A.CascadeDecoder(A.BeliefPropagationDecoder(10), A.QPADMMDecoder(1.2, 0.55, 200, fast_setup=True))
    try:
        total, first, ex = A.run_experiment_cascade(cas, c.cws, c.H, snr, noise="host")
        bits, ok, it, st = cas.decode_batch(c.H, y, snr)
        assert (ok[st == 2] == 1).all()
        want, _, _ = mc_detail(y, pack_bits(bits), ok, it, c.cws, c.Hm)
        assert _counters(total) == {f: want[f] for f in SEVEN} and want["noncodeword_frames"] > 0
        assert total.correct == first.correct + ex["second_correct"] and ex["second_frames"] == int((st == 2).sum())
    finally:
        cas.close()


# ------------------------------------------------------------------------------------- 5. refusals, driver
def test_refusals_launch_nothing(A):
    import torch
    L = A.lib()
    c, snr, y = _symbols(A, "H05", -2.0)
    cas = _mc_pair(A)
    try:
        h, _ = cas.handle(c.H)
        nw = (c.n + 31) // 32
        yd = torch.from_numpy(y[:4]).cuda()
        bits = torch.full((4, nw), -1, dtype=torch.int32, device="cuda")
        ok = torch.full((4,), 7, dtype=torch.uint8, device="cuda")
        err = lambda: L.acg_ldpc_last_error().decode()
        assert L.acg_ldpc_cascade_decode_batch_dev(h, yd.data_ptr(), 1, -1, snr, bits.data_ptr(), ok.data_ptr(), None, None, None) != 0
        assert "frames < 0" in err()
        assert L.acg_ldpc_cascade_decode_batch_dev(h, None, 1, 4, snr, bits.data_ptr(), ok.data_ptr(), None, None, None) != 0
        assert "null y" in err()
        assert L.acg_ldpc_cascade_decode_batch_dev(h, yd.data_ptr(), 1, 4, snr, None, ok.data_ptr(), None, None, None) != 0
        assert "null bits or ok" in err()
        assert L.acg_ldpc_cascade_decode_batch_dev(h, yd.data_ptr(), 1, 4, snr, bits.data_ptr(), None, None, None, None) != 0
        assert "null bits or ok" in err()
        torch.cuda.synchronize()
        assert (bits == -1).all() and (ok == 7).all()
        hb, hk = np.zeros((4, c.n), dtype=np.uint8), np.zeros(4, dtype=np.uint8)
        assert L.acg_ldpc_cascade_decode_batch(h, y.ctypes.data, -1, snr, hb.ctypes.data, hk.ctypes.data, None, None) != 0
        assert L.acg_ldpc_cascade_decode_batch(h, None, 4, snr, hb.ctypes.data, hk.ctypes.data, None, None) != 0
        assert L.acg_ldpc_cascade_decode_batch_f32(h, y.ctypes.data, 4, snr, None, hk.ctypes.data, None, None) != 0
        assert L.acg_ldpc_cascade_decode_batch(h, y.ctypes.data, 0, snr, hb.ctypes.data, hk.ctypes.data, None, None) == 0
        assert not L.acg_ldpc_cascade_stage(h, 2) and not L.acg_ldpc_cascade_stage(h, -1)
        from acg_alp_ldpc_amd import _lib
        cfg, res = mc_cfg(A, c.cws, snr, -5, 0, 1, "host"), _lib.CascadeResult()
        assert L.acg_ldpc_cascade_mc_run(h, C.byref(cfg), C.byref(res)) != 0 and "bad mc cfg" in err()
        assert L.acg_ldpc_cascade_mc_run(h, None, C.byref(res)) != 0
    finally:
        cas.close()
    with pytest.raises(A.LdpcError, match="second: "):
        A.CascadeDecoder(A.BeliefPropagationDecoder(5), A.BeliefPropagationDecoder(-1)).handle(c.H)
    with pytest.raises(TypeError):
        A.CascadeDecoder(A.BeliefPropagationDecoder(5), "BP")


def test_eval_driver_adds_one_row_per_snr(A, tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "drivers")], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "tools", "drivers", "bin", "acg_eval")
    base = [exe, "--H", os.path.join(DATA, "H05.txt"), "--G", os.path.join(DATA, "G05.txt"), "--snrs", "-2,-1", "--tests", "400",
            "--bp-iters", "50", "--no-admm", "--minsum-iters", "10"]
    plain = subprocess.run(base + ["--out", str(tmp_path / "a.csv")], capture_output=True, text=True, timeout=120)
    casc = subprocess.run(base + ["--out", str(tmp_path / "b.csv"), "--cascade", "minsum,bp"], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and casc.returncode == 0, plain.stderr + casc.stderr
    strip = lambda text: [",".join(l.split(",")[:4] + l.split(",")[5:]) for l in text.strip().splitlines()]   # (the Time column)
    a, b = strip((tmp_path / "a.csv").read_text()), strip((tmp_path / "b.csv").read_text())
    assert len(a) == 1 + 2 * 2 and b[:len(a)] == a and len(b) == len(a) + 2
    c = Q.case(A, "H05")
    cas = _mc_pair(A)
    try:
        for row, snr in zip(b[len(a):], (-2.0, -1.0)):
            total, _, _ = A.run_experiment_cascade(cas, c.cws, c.H, snr, noise="host")
            f = row.split(",")
            assert f[0] == "MS+BP" and float(f[1]) == snr and abs(float(f[3]) - total.FER()) < 1e-9
    finally:
        cas.close()
    assert "Algo: MS+BP" in casc.stdout and "Algo: MS+BP" not in plain.stdout
    bad = subprocess.run(base + ["--cascade", "bp,turbo"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--cascade A,B" in bad.stderr
