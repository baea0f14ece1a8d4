"""GPU: the rate-matched Monte-Carlo run (acg_ldpc_mc_run_rm, acg_ldpc_rm_channel_dev) against a composition of public pieces
that already exist, never the code under test (tests/rm_cases.py): acg_ldpc_awgn_dev for the symbols, tests/rm_ref.py for channel
values and raw errors, the handle's own decode_llr_batch_dev for word, flag and iterations, rm_ref.counters.

1. channel values and raw errors, bit for bit, on the three shapes, the float and the quantized handles, two quantisers, and a
   run that crosses the high word of the frame counter
2. the seven counters on every engine a shape takes, at SNRs where frames both decode and fail
3. any chunking, any sharding: the same counters
4. degenerate patterns: none / all sent = acg_ldpc_mc_run; all shortened; max_iter = 0
5. refusals on a live handle, in the header's order, and the handle decodes afterwards
6. the C++ mirror and acg_eval --puncture / --shorten"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rm_cases as RM
import rm_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ------------------------------------------------------------------------------------------ 1. channel values
CHANNEL = [(name, engine, quant) for name in RM.CASES for engine in ("float-ms", "q-lds", "q-streamed") if name in RM.ENGINES[engine]
           for quant in (("default",) if engine == "float-ms" else ("default", "saturating"))]


@pytest.mark.parametrize("name,engine,quant", CHANNEL)
def test_channel_values_and_raw_errors_equal_the_restatement(A, name, engine, quant):
    """the case's frames from frame 0 and 8 frames from 2^32 - 3; floats compared as uint32; with the pattern, with none, and
    without the raw-error output"""
    c = RM.case(A, name)
    dec = RM.decoder(A, engine, c.iters, quant)
    try:
        for first, frames in ((0, c.frames), (2 ** 32 - 3, 8)):
            y = RM.awgn(dec, c, first, frames)
            sent = c.sent(first, frames)
            for pattern in (None, c.pattern):
                got, raw = RM.rm_channel(dec, engine, c, pattern, first, frames)
                want = rm_ref.channel_values(y, sent, c.snr, pattern, RM.quant_of(engine, quant))
                assert got.dtype == want.dtype and (_bits(got) == _bits(want)).all(), (name, engine, quant, first, pattern is None)
                assert (raw == rm_ref.raw_errors(y, sent, pattern)).all(), (name, engine, quant, first, pattern is None)
            again, none = RM.rm_channel(dec, engine, c, c.pattern, first, frames, raw=False)
            assert none is None and (_bits(again) == _bits(got)).all()
        # the pattern does what it says: erasures and known bits where it says, and a raw count that lost its share
        got, raw = RM.rm_channel(dec, engine, c, c.pattern, 0, c.frames)
        sent = c.sent(0, c.frames)
        assert not got[:, c.punctured].any() and (np.signbit(got[:, c.shortened].astype(np.float32)) == (sent[:, c.shortened] != 0)).all()
        assert 0 < raw.sum() < RM.rm_channel(dec, engine, c, None, 0, c.frames)[1].sum()
        if name == "H05":
            assert sent[:, c.shortened].any() and not sent[:, c.shortened].all()      # shortened bits that are 1, and 0
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------ 2. counters
COUNTERS = [("H05", "float-bp"), ("H05", "float-ms"), ("H05", "q-lds"), ("H05", "q-streamed"), ("deg40", "float-bp"), ("deg40", "q-streamed"),
            ("odd62", "float-ms"), ("odd62", "q-lds")]


@pytest.mark.parametrize("name,engine", COUNTERS)
def test_counters_equal_the_composition(A, name, engine):
    """H05: float sum-product, float min-sum, quantized LDS, quantized streamed; deg40: the two streamed engines; odd62"""
    c = RM.case(A, name)
    dec = RM.decoder(A, engine, c.iters)
    try:
        want, ok = RM.composition(dec, engine, c, c.pattern, 0, c.frames)
        rate = float(ok.mean())
        print("%s %s: ok rate of the composition %.3f; %r" % (name, engine, rate, want))
        if name in ("H05", "deg40"):
            assert 0.05 <= rate <= 0.95, (name, engine, rate)
        got = RM.as_dict(A.run_experiment_rm(dec, c.cws, c.H, c.snr, pattern=c.pattern, frames=c.frames, seed=RM.SEED))
        assert got == want, (got, want)
        assert got["total"] == c.frames and got["sum_hamming"] == got["sum_hamming_ok"] + got["sum_hamming_wrong"] > 0
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------ 3. chunks and shards
@pytest.mark.parametrize("engine", ["float-ms", "q-lds"])
def test_chunks_and_shards_give_the_same_counters(A, engine):
    """H05, 300 frames: ACG_MC_RM_CHUNK=64 makes five chunks, the last of 44 frames; [0, 130) and [130, 300) merged with
    acg_ldpc_mc_merge; both equal the run in one chunk, from a first frame that is no multiple of the codeword count"""
    from acg_alp_ldpc_amd._lib import McResult, lib
    c = RM.case(A, "H05")
    dec = RM.decoder(A, engine, c.iters)
    first = 1000
    try:
        whole = A.run_experiment_rm(dec, c.cws, c.H, c.snr, pattern=c.pattern, frames=c.frames, first_frame=first, seed=RM.SEED)
        os.environ["ACG_MC_RM_CHUNK"] = "64"
        try:
            chunked = A.run_experiment_rm(dec, c.cws, c.H, c.snr, pattern=c.pattern, frames=c.frames, first_frame=first, seed=RM.SEED)
        finally:
            del os.environ["ACG_MC_RM_CHUNK"]
        assert RM.as_dict(chunked) == RM.as_dict(whole) and 0 < whole.correct < c.frames
        h, _ = dec.handle(c.H)
        parts = []
        for lo, cnt in ((0, 130), (130, 170)):
            cfg = RM.mc_cfg(c, first + lo, cnt)
            r = McResult()
            assert lib().acg_ldpc_mc_run_rm(h, C.byref(cfg), c.pattern.ctypes.data, C.byref(r)) == 0, lib().acg_ldpc_last_error()
            parts.append(r)
        lib().acg_ldpc_mc_merge(C.byref(parts[0]), C.byref(parts[1]))
        assert RM.as_dict(parts[0]) == RM.as_dict(whole), (RM.as_dict(parts[0]), RM.as_dict(whole))
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------ 4. degenerate patterns
@pytest.mark.parametrize("engine", ["float-ms", "q-lds", "q-streamed"])
def test_no_pattern_and_all_sent_are_the_plain_run(A, engine):
    c = RM.case(A, "H05")
    dec = RM.decoder(A, engine, c.iters)
    try:
        plain = RM.as_dict(A.run_experiment(dec, c.cws, c.H, c.snr, frames=c.frames, first_frame=7, noise="device", seed=RM.SEED))
        for pattern in (None, np.zeros(c.n, dtype=np.uint8)):
            got = RM.as_dict(A.run_experiment_rm(dec, c.cws, c.H, c.snr, pattern=pattern, frames=c.frames, first_frame=7, seed=RM.SEED))
            assert got == plain, (engine, pattern is None, got, plain)
        assert 0 < plain["correct"] < c.frames
    finally:
        dec.close()


@pytest.mark.parametrize("engine", ["float-bp", "float-ms", "q-lds", "q-streamed"])
def test_all_shortened_and_no_iterations(A, engine):
    """all shortened: every frame correct in one iteration, no raw errors; max_iter = 0: every frame fails with no iteration and
    the raw errors are still counted"""
    c = RM.case(A, "H05")
    dec = RM.decoder(A, engine, c.iters)
    dec0 = RM.decoder(A, engine, 0)
    try:
        r = RM.as_dict(A.run_experiment_rm(dec, c.cws, c.H, c.snr, pattern=np.full(c.n, 2, dtype=np.uint8), frames=c.frames, seed=RM.SEED))
        assert r == {"correct": c.frames, "pseudo": 0, "total": c.frames, "sum_hamming": 0, "sum_hamming_ok": 0, "sum_hamming_wrong": 0,
                     "sum_iters": c.frames}, r
        y = RM.awgn(dec0, c, 0, c.frames)
        raw = int(rm_ref.raw_errors(y, c.sent(0, c.frames), c.pattern).sum())
        r0 = RM.as_dict(A.run_experiment_rm(dec0, c.cws, c.H, c.snr, pattern=c.pattern, frames=c.frames, seed=RM.SEED))
        assert raw > 0 and r0 == {"correct": 0, "pseudo": 0, "total": c.frames, "sum_hamming": raw, "sum_hamming_ok": 0, "sum_hamming_wrong": raw,
                                  "sum_iters": 0}, (r0, raw)
        none = RM.as_dict(A.run_experiment_rm(dec, c.cws, c.H, c.snr, pattern=c.pattern, frames=0, seed=RM.SEED))
        assert not any(none.values())
    finally:
        dec.close()
        dec0.close()


# ------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_on_a_live_handle_in_the_stated_order(A):
    from acg_alp_ldpc_amd._lib import McResult, lib
    import torch
    L = lib()
    c = RM.case(A, "H05")
    out = torch.zeros((4, c.n), dtype=torch.float32, device="cuda")
    bad_pat = c.pattern.copy()
    bad_pat[17] = 3
    bad_pat[40] = 200

    def both(h, cfg, pat):
        r = McResult()
        r.total = 77
        p = None if pat is None else pat.ctypes.data
        rc1, m1 = L.acg_ldpc_mc_run_rm(h, C.byref(cfg), p, C.byref(r)), L.acg_ldpc_last_error().decode()
        rc2, m2 = L.acg_ldpc_rm_channel_dev(h, C.byref(cfg), p, out.data_ptr(), None, None), L.acg_ldpc_last_error().decode()
        assert rc1 != 0 and rc2 != 0 and r.total == 77, (rc1, rc2, m1, m2)
        return m1, m2

    others = {"BP": A.BeliefPropagationDecoder(5), "QP-ADMM": A.QPADMMDecoder(1.95, 0.5, 20, 1e-5), "OSD": A.OSDDecoder(0),
              "layered LDS": A.MinSumDecoder(5, 0.75, schedule=A.SCHEDULE_LAYERED)}
    ours = RM.decoder(A, "float-ms", 5)
    try:
        # a handle of another create call: refused last, so each earlier reason wins over it
        for name, dec in others.items():
            h, _ = dec.handle(c.H)
            cfg = RM.mc_cfg(c, 0, 4)
            for m in both(h, cfg, c.pattern):
                assert all(w in m + " " for w in ("acg_ldpc_decoder_create_layered_streamed,", "acg_ldpc_decoder_create_quantized ",
                                                  "acg_ldpc_decoder_create_quantized_streamed ")), (name, m)
            for m in both(h, cfg, bad_pat):
                assert "pattern[17] = 3" in m, (name, m)
            cfg.noise = A._lib.NOISE_HOST_MT19937
            for m in both(h, cfg, bad_pat):
                assert "device noise only" in m, (name, m)
            cfg.frames = -1
            for m in both(h, cfg, bad_pat):
                assert "bad mc cfg" in m, (name, m)
            r = A.run_experiment(dec, c.cws, c.H, 1.0, frames=8, noise="device")      # the handle still decodes
            assert r.total == 8, name
        h, _ = ours.handle(c.H)
        cfg = RM.mc_cfg(c, 0, 4, noise=A._lib.NOISE_HOST_MT19937)
        for m in both(h, cfg, None):
            assert "device noise only" in m, m
        cfg = RM.mc_cfg(c, 0, 4)
        for m in both(h, cfg, bad_pat):
            assert "pattern[17] = 3" in m, m
        with pytest.raises(A.LdpcError, match="device noise only|null argument"):
            ours.rm_channel_dev(c.H, cfg, None, None)
        assert not out.cpu().numpy().any()       # nothing was launched
        good = A.run_experiment_rm(ours, c.cws, c.H, 1.0, pattern=c.pattern, frames=8)
        assert good.total == 8
    finally:
        ours.close()
        for dec in others.values():
            dec.close()


# ------------------------------------------------------------------------------------------ 6. C++ mirror and driver
def test_cxx_mirror_returns_the_c_calls_counters(A, tmp_path):
    A.lib()
    exe = RM.build_cxx_check(tmp_path)
    out = subprocess.run([exe, os.path.join(RM.DATA, "H05.txt")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(" same=1 ") == 3 and "MS frames=200" in out.stdout and out.stdout.count("QMS frames=200") == 2, out.stdout


def test_eval_driver_rows_are_run_experiment_rm(A, oracle, tmp_path):
    """acg_eval --puncture / --shorten on H05 with the case's positions written as indices and ranges: FER and the three Hamming
    columns of every block are run_experiment_rm's on the same words, frames and seed"""
    subprocess.check_call(["make", "-C", os.path.join(RM.ROOT, "tools", "drivers")], stdout=subprocess.DEVNULL)
    F, snr = 300, -2.0
    c = RM.case(A, "H05")
    csv = str(tmp_path / "r.csv")
    pun = ",".join(str(v) for v in c.punctured[:-2]) + ",%d-%d" % (c.punctured[-2], c.punctured[-2]) + ",%d" % c.punctured[-1]
    sho = ",".join(str(v) for v in c.shortened)
    r = subprocess.run([os.path.join(RM.ROOT, "tools", "drivers", "bin", "acg_eval"), "--H", os.path.join(RM.DATA, "H05.txt"), "--snrs", str(snr),
                        "--tests", str(F), "--noise", "device", "--seed", "9", "--puncture", pun, "--shorten", sho, "--qms-engine", "streamed",
                        "--qms-iters", "15", "--layered-streamed", "bp,minsum", "--bp-iters", "15", "--minsum-iters", "15", "--ms-scale", "0.75",
                        "--out", csv], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = open(csv).read().strip().split("\n")
    assert lines[0] == "Method,SNR,Sigma,FER,Time,AvgHamming,AvgHammingCorrect,AvgHammingWrong"
    rows = [l.split(",") for l in lines[1:]]
    assert [x[0] for x in rows] == ["QMS", "BP", "MS"] and r.stdout.count("Algo: ") == 3, r.stdout
    Hm = oracle.read_pcm(os.path.join(RM.DATA, "H05.txt"))
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 239239239, F)
    decs = [RM.decoder(A, "q-streamed", 15), RM.decoder(A, "float-bp", 15), RM.decoder(A, "float-ms", 15)]
    try:
        for row, dec in zip(rows, decs):
            e = A.run_experiment_rm(dec, cws, c.H, snr, pattern=c.pattern, frames=F, seed=9)
            want = (e.FER(), e.mean_hamming(), e.mean_hamming_ok(), e.mean_hamming_wrong())
            got = tuple(float(row[i]) for i in (3, 5, 6, 7))
            assert float(row[1]) == snr and got == pytest.approx(want, abs=1e-11), (row, want)
            assert 0 < e.correct < F
    finally:
        for dec in decs:
            dec.close()
