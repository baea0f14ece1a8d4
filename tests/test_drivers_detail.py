"""The detail flags of tools/drivers/acg_eval (--detail, --detail-out, --events-out, --events-cap).  CPU: the driver builds
and refuses inconsistent flags before it loads anything.  GPU: report.csv does not change, the two new files hold what
acg_ldpc_mc_run_detail returns, and shards merge to the single-handle result."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "drivers", "bin")
DATA = os.path.join(ROOT, "data")
DETAIL_HEADER = "Method,SNR,Frames,FER,BER,WordFrames,BitErrors,Pseudo,MinPseudoWeight,MinPseudoFrame,NonCodewordFrames,AvgSyndromeWeight"
EVENTS_HEADER = "Method,SNR,Frame,Kind,Iters,RawErrors,BitErrors,SyndromeWeight"


@pytest.fixture(scope="module")
def drivers():
    import acg_alp_ldpc_amd as A
    A.build()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "drivers")], stdout=subprocess.DEVNULL)
    return BIN


def test_inconsistent_event_flags_are_refused_before_anything_is_loaded(drivers, tmp_path):
    exe = os.path.join(drivers, "acg_eval")
    assert os.access(exe, os.X_OK)
    ev = str(tmp_path / "ev.csv")
    for flags in (["--events-out", ev], ["--events-cap", "5"], ["--events-out", ev, "--events-cap", "0"],
                  ["--events-out", ev, "--events-cap", "-3"]):
        # (--H names a file that does not exist: the flag check comes first, so its message is the one printed)
        r = subprocess.run([exe, "--H", str(tmp_path / "missing.txt"), "--out", str(tmp_path / "r.csv")] + flags, capture_output=True,
                           text=True, timeout=60, cwd=str(tmp_path))
        assert r.returncode == 2 and "--events-cap" in r.stderr, (flags, r.stderr)
        assert not os.path.exists(ev) and not os.path.exists(str(tmp_path / "r.csv"))
    # consistent flags get as far as reading H
    r = subprocess.run([exe, "--H", str(tmp_path / "missing.txt"), "--events-out", ev, "--events-cap", "5"], capture_output=True, text=True,
                       timeout=60, cwd=str(tmp_path))
    assert r.returncode == 1 and "read_pcm" in r.stderr


def test_driver_source_keeps_the_plain_path(drivers):
    """without the new flags the driver still calls acg_ldpc_mc_run (MultiGpu::run) and writes only --out"""
    src = open(os.path.join(ROOT, "tools", "drivers", "acg_eval.cpp")).read()
    assert "r = d.run(cws, n, snr, tests, noise" in src and "if (detail)" in src
    assert DETAIL_HEADER in src and EVENTS_HEADER in src


def run_eval(drivers, tmp_path, tag, extra, noise="device", tests="1000"):
    out = str(tmp_path / ("report_%s.csv" % tag))
    r = subprocess.run([os.path.join(drivers, "acg_eval"), "--H", os.path.join(DATA, "H05.txt"), "--snrs", "-2", "--tests", tests,
                        "--bp-iters", "50", "--alpha", "1.95", "--mu", "0.5", "--admm-iters", "100", "--noise", noise, "--out", out] + extra,
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    rows = [x.split(",") for x in open(out).read().strip().splitlines()]
    return r, rows


@pytest.mark.gpu
def test_eval_driver_detail_files(drivers, tmp_path):
    import numpy as np
    import acg_alp_ldpc_amd as A
    r0, plain = run_eval(drivers, tmp_path, "plain", [])
    assert sorted(os.listdir(str(tmp_path))) == ["report_plain.csv"]          # nothing new without the flags
    det, ev = str(tmp_path / "d.csv"), str(tmp_path / "e.csv")
    r1, full = run_eval(drivers, tmp_path, "full", ["--detail", "--detail-out", det, "--events-out", ev, "--events-cap", "6"])
    # report.csv: every column except Time; stdout: every line except its (time=...) part
    assert [[x[i] for i in (0, 1, 2, 3, 5, 6, 7)] for x in plain] == [[x[i] for i in (0, 1, 2, 3, 5, 6, 7)] for x in full]
    assert [l.split(", (time")[0] for l in r0.stdout.splitlines()] == [l.split(", (time")[0] for l in r1.stdout.splitlines()]
    rows = open(det).read().strip().splitlines()
    assert rows[0] == DETAIL_HEADER and [x.split(",")[0] for x in rows[1:]] == ["BP", "QP-ADMM"]
    evl = open(ev).read().strip().splitlines()
    assert evl[0] == EVENTS_HEADER
    # the same runs through the Python mirror
    H = A.read_pcm(os.path.join(DATA, "H05.txt"))
    G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 1000, 239239239)
    names = {1: "PSEUDO", 2: "NO_WORD", 3: "NONCODEWORD"}
    at = 1
    for row, dec in zip(rows[1:], (A.BeliefPropagationDecoder(50), A.QPADMMDecoder(1.95, 0.5, 100))):
        d = A.run_experiment_detail(dec, cws, H, -2.0, frames=1000, noise="device", seed=1, cap=6)
        f = row.split(",")
        assert (int(f[2]), int(f[5]), int(f[6]), int(f[7]), int(f[8]), int(f[9]), int(f[10])) == \
            (d.total, d.word_frames, d.bit_errors, d.pseudo, d.min_pseudo_weight, d.min_pseudo_frame, d.noncodeword_frames)
        assert float(f[3]) == pytest.approx(d.FER(), abs=1e-11) and float(f[4]) == pytest.approx(d.BER(), abs=1e-11)
        assert float(f[11]) == pytest.approx(d.mean_syndrome_weight(), abs=1e-11)
        assert d.n_stored == 6
        for e in d.events:
            g = evl[at].split(",")
            at += 1
            assert g[0] == dec.name() and float(g[1]) == -2.0
            assert (int(g[2]), g[3], int(g[4]), int(g[5]), int(g[6]), int(g[7])) == \
                (int(e["frame"]), names[int(e["kind"])], int(e["iters"]), int(e["raw_errors"]), int(e["bit_errors"]), int(e["syndrome_weight"]))
        assert np.all(np.diff(d.events["frame"]) > 0)
    assert at == len(evl)
    # --detail alone writes report_detail.csv next to the caller and no event log
    run_eval(drivers, tmp_path, "d2", ["--detail", "--no-admm"])
    assert open(str(tmp_path / "report_detail.csv")).read().splitlines()[0] == DETAIL_HEADER


@pytest.mark.gpu
def test_eval_driver_detail_shards_merge(drivers, tmp_path):
    """--gpus 3 folded onto one device, 1001 frames: the merged detail file and event log equal the single-handle ones"""
    got = {}
    for tag, extra in (("one", []), ("three", ["--gpus", "3", "--device-count", "1"])):
        det, ev = str(tmp_path / (tag + "_d.csv")), str(tmp_path / (tag + "_e.csv"))
        run_eval(drivers, tmp_path, tag, ["--detail-out", det, "--events-out", ev, "--events-cap", "40"] + extra, tests="1001")
        got[tag] = (open(det).read(), open(ev).read())
    assert got["one"] == got["three"]
    assert len(got["one"][1].splitlines()) == 1 + 2 * 40
