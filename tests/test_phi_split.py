"""The one-series phi of the fused fixed-work sum-product sweeps (bp_core.inc: Dom<float>::phi_small / phi_large), host side: the
census of the units that need one series only (csrc/bp_sat_census.hpp, tools/phi_census.cpp --split) and the order of the two
series in the float model with adverse rounding of the transcendentals.  tests/phi_split_check.cpp is the stand-alone program;
tests/test_phi_split_gpu.py compares the device's own series on every bit pattern.  Host only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = os.path.join(ROOT, "acg_alp_ldpc_amd", "csrc", "code.cpp")
H05 = os.path.join(ROOT, "data", "H05.txt")
# H05, L = 32, 300 frames at -2 dB stopped at their first state repeat, thresholds 1 and 2 (the +0 rule and the |x| >= 66 rule as the
# fast paths): (behind the latch, side) -> per cent of units skipped, all <= 1, all >= 2, mixed
TABLE = {(0, "c"): (0.0, 0.6, 0.0, 99.4), (0, "v"): (0.0, 0.0, 20.4, 79.6), (1, "c"): (8.1, 46.8, 0.0, 45.1), (1, "v"): (40.3, 0.0, 54.7, 5.1)}
# every STRIDE-th bit pattern in the suite; the full enumeration (1.1e9 patterns, about a minute) is `phi_split_check series 1`
STRIDE = 16


def build(out, src, *flags):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", *flags, "-I" + os.path.join(ROOT, "include"), src, CODE, "-o", out])
    return out


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("phisplit") / "phi_split_check"), os.path.join(ROOT, "tests", "phi_split_check.cpp"))


def census_rows(exe):
    r = subprocess.run([exe, "census", H05], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "sweeps":
            rows["sweeps"] = (float(w[1]), float(w[2]))
        else:
            rows[(int(w[0]), w[1])] = (int(w[2]),) + tuple(float(x) for x in w[3:7])
    return rows


def test_census_reproduces_the_table(check):
    rows = census_rows(check)
    print(rows)
    for key, want in TABLE.items():
        got = rows[key]
        assert got[0] > 90000, (key, got)
        for g, w in zip(got[1:], want):
            assert abs(g - w) <= 2.0, (key, got, want)
    total, behind = rows["sweeps"]
    assert abs(total - 26.66) < 0.5 and abs(behind - 14.81) < 0.5, rows["sweeps"]


def test_series_order_with_adverse_rounding(check):
    r = subprocess.run([check, "series", str(STRIDE)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    w = r.stdout.split()
    print("patterns %s, smallest relative gap: pl over ps on [2, 66) %s, ps over pl on (0, 1] %s" % (w[1], w[2], w[3]))
    assert int(w[1]) >= (0x42840000 - 0x40000000 + 0x3F800000) // STRIDE
    # more than a hundred fp32 ulps of room at either threshold, with the transcendentals already moved two ulps against it
    assert float(w[2]) > 100 * 2.0 ** -24 and float(w[3]) > 100 * 2.0 ** -24


def test_the_same_program_sanitized(tmp_path):
    """the stand-alone host program under AddressSanitizer and UBSan (runtimes linked statically: nothing is loaded into Python)"""
    exe = build(str(tmp_path / "phi_split_check_san"), os.path.join(ROOT, "tests", "phi_split_check.cpp"), "-g", "-fsanitize=address,undefined",
                "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")
    rows = census_rows(exe)
    assert set(TABLE) <= set(rows)
    r = subprocess.run([exe, "series", "1024"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
