"""acg_qpadmm_params: the default path (the whole grid through acg_ldpc_mc_run_grid on one handle) against --per-point
(one handle and one acg_ldpc_mc_run per grid point)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "drivers", "bin")
DATA = os.path.join(ROOT, "data")


@pytest.fixture(scope="module")
def drivers():
    import acg_alp_ldpc_amd as A
    A.build()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "drivers")], stdout=subprocess.DEVNULL)
    return BIN


def test_library_and_header_declare_the_grid_entry_point():
    """CPU: the symbol is in the header, in the ctypes table and in the built library"""
    import acg_alp_ldpc_amd as A
    from acg_alp_ldpc_amd import _lib
    assert "acg_ldpc_mc_run_grid" in _lib.SYMBOLS
    assert "int acg_ldpc_mc_run_grid(" in open(os.path.join(ROOT, "include", "acg_ldpc.h")).read()
    A.build()
    assert hasattr(A.lib(), "acg_ldpc_mc_run_grid")
    assert callable(A.run_experiment_grid)


@pytest.mark.gpu
@pytest.mark.parametrize("noise", ["host", "device"])
def test_grid_path_prints_what_the_per_point_path_prints(drivers, noise):
    """5 x 5 grid at 200 frames: stdout and stderr are byte-identical (the --time line, the last of stderr, apart)"""
    base = [os.path.join(drivers, "acg_qpadmm_params"), "--H", os.path.join(DATA, "optimalH.txt"), "--tests", "200", "--iters", "300",
            "--alpha", "0,2,5", "--mu", "0,1,5", "--noise", noise, "--time"]
    runs = []
    for extra in ([], ["--per-point"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr
        err = r.stderr.splitlines()
        assert err[-1].startswith("grid evaluation wall time: ") and err[-1].endswith(" s")
        runs.append((r.stdout, err[:-1]))
    assert runs[0] == runs[1]
    assert sum(l.startswith("alpha=") for l in runs[0][1]) == 25
    assert "new best fer found" in runs[0][0] and "Best parameters:" in runs[0][0]
    assert any(l == "alpha=0, mu=0: fer=1" for l in runs[0][1])   # guard points (alpha = mu = 0 among them)
