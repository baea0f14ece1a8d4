"""Absorbed degree-1 variables (csrc/code.cpp bp_layout_build, BpLayout::n_apass): host-only layout checks."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("absorb") / "absorb_layout_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "absorb_layout_check.cpp"),
                           os.path.join(ROOT, "acg_alp_ldpc_amd", "csrc", "code.cpp"), "-o", out])
    return out


def run(exe, name, L):
    r = subprocess.run([exe, os.path.join(ROOT, "data", name + ".txt"), str(L)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return tuple(int(x) for x in r.stdout.split())


@pytest.mark.parametrize("L", [16, 32, 64])
@pytest.mark.parametrize("name", ["H05", "optimalH", "H"])
def test_absorbed_layout_partitions_the_code(exe, name, L):
    # the binary checks the partition, the edge order inside every check, the degree counts and the message array
    n = {"H": 128}.get(name, 280)
    absorbed, vpass, vpass0 = run(exe, name, L)
    assert vpass == (n - absorbed + L - 1) // L and vpass0 == (n + L - 1) // L


def test_h05_absorbs_two_trailing_passes(exe):
    # H05: 80 degree-1 variables (columns 200-279), each the last edge of its own degree-4 or degree-5 check.  At L = 32
    # the checks are 20 x 7, 60 x 6, 40 x 5, 40 x 4: the last two passes (24 x 5 + 8 x 4, 32 x 4) are all such checks,
    # the pass before them mixes 16 degree-6 checks in and stays as it is.  280 - 64 = 216 variables: 7 passes, not 9.
    assert run(exe, "H05", 32) == (64, 7, 9)
    assert run(exe, "H05", 64) == (32, 4, 5)


def test_nothing_to_absorb(exe):
    # data/H.txt has no degree-1 variable; optimalH's are not at the end of a run of whole check passes
    for L in (16, 32, 64):
        assert run(exe, "H", L)[0] == 0
        assert run(exe, "optimalH", L)[0] == 0
