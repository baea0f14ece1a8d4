"""tools/phi_census.cpp (host only): the census of the phi fast path builds and runs on the library's layout, the memo of the
absorbed passes only ever adds skipped check rows, and a code without absorbed passes gets nothing from it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("census") / "phi_census")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "phi_census.cpp"),
                           os.path.join(ROOT, "acg_alp_ldpc_amd", "csrc", "code.cpp"), "-o", out])
    return out


def rows(exe, name, *snr):
    r = subprocess.run([exe, os.path.join(ROOT, "data", name + ".txt"), "40", "20", "32"] + [str(s) for s in snr],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = []
    for line in r.stdout.splitlines():
        if line.startswith("| ") and "dB" in line:
            out.append([float(c.strip().rstrip("%").strip()) for c in line.strip("|").split("|")[1:]])
    assert len(out) == len(snr), r.stdout
    return r.stdout, out


def test_census_h05(exe):
    text, out = rows(exe, "H05", -2, 2)
    assert "5 check passes (2 absorbed), 7 variable passes" in text
    for today, memo, memo_all, var, all_today, all_memo, fer in out:
        assert 0 <= today <= memo <= memo_all <= 100 and all_today <= all_memo
    assert out[1][1] > out[1][0] + 5  # +2 dB: most frames have converged, the absorbed rows are memo hits
    assert out[1][6] == 0


def test_census_without_absorbed_passes(exe):
    text, out = rows(exe, "H", 2)
    assert "(0 absorbed)" in text
    today, memo, memo_all, var, all_today, all_memo, fer = out[0]
    assert memo == today and all_memo == all_today
