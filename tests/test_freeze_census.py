"""tools/freeze_census.cpp (host only): the census of the freeze path builds and runs on the library's layout, and the float model
has the property the kernel's freeze stands on: a frame stopped at its first exact repeat of the message state has, after the
last sweep, the hard decisions it latched."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = ("fer", "latched", "latch", "repeat_share", "lag", "run_first", "run_cadence", "frozen_share", "detections")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("census") / "freeze_census")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "freeze_census.cpp"),
                           os.path.join(ROOT, "acg_alp_ldpc_amd", "csrc", "code.cpp"), "-o", out])
    return out


def census(exe, frames, sweeps, first, period, *snr):
    r = subprocess.run([exe, os.path.join(ROOT, "data", "H05.txt"), str(frames), str(sweeps), "32", str(first), str(period)] +
                       [str(s) for s in snr], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = []
    for line in r.stdout.splitlines():
        if line.startswith("| ") and "dB" in line:
            cells = [c.strip() for c in line.strip("|").split("|")[1:]]
            assert len(cells) == len(COLS), line
            rows.append(dict(zip(COLS, cells)))
    assert len(rows) == len(snr), r.stdout
    differ = [line for line in r.stdout.splitlines() if line.startswith("stopped frames whose final decisions differ")]
    assert len(differ) == 1, r.stdout
    return r.stdout, rows, int(differ[0].rsplit(":", 1)[1])


def num(cell):
    return float(cell.split()[0])


def test_stopped_frames_keep_their_latched_decisions(exe):
    text, rows, differ = census(exe, 300, 50, 6, 2, -3, -2, 2)
    assert "5 check passes (2 absorbed), 7 variable passes" in text
    assert differ == 0, text
    lo, mid, hi = rows
    # the property is asked of frames that did reach a repeat: most latched frames do, all of them at +2 dB
    assert int(hi["latched"]) == 300 and num(hi["repeat_share"]) == 100 and num(hi["fer"]) == 0
    assert int(mid["latched"]) > 200 and num(mid["repeat_share"]) > 90
    assert 50 < int(lo["latched"]) < 250
    for r in rows:
        # a cadence stops a frame no earlier than its first repeat, and never costs a sweep
        assert num(r["run_first"]) <= num(r["run_cadence"]) <= 50
    assert num(hi["run_cadence"]) < 15 and num(hi["frozen_share"]) == 100
    assert num(lo["run_cadence"]) > num(mid["run_cadence"]) > num(hi["run_cadence"])


def test_nothing_freezes_within_two_sweeps(exe):
    # the first detection behind a latch only writes: with first = period = 1 the earliest stop is the latch + 2, never the last sweep
    for sweeps in (1, 2):
        text, rows, differ = census(exe, 40, sweeps, 1, 1, 2)
        assert num(rows[0]["frozen_share"]) == 0 and num(rows[0]["run_cadence"]) == sweeps and differ == 0, text
