"""GPU: acg_eval --qms-engine streamed writes the rows of --qms-engine lds on H05 — every column but the wall time."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data")
BIN = os.path.join(ROOT, "tools", "drivers", "bin")


@pytest.fixture(scope="module")
def drivers():
    import acg_alp_ldpc_amd as A
    A.lib()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "drivers")], stdout=subprocess.DEVNULL)
    return BIN


def test_eval_driver_refuses_an_unknown_engine(drivers, tmp_path):
    r = subprocess.run([os.path.join(drivers, "acg_eval"), "--H", os.path.join(DATA, "H05.txt"), "--qms-engine", "hbm", "--out", str(tmp_path / "r.csv")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--qms-engine lds or streamed" in r.stderr


@pytest.mark.gpu
def test_eval_driver_streamed_rows_are_the_lds_rows(drivers, tmp_path):
    rows = {}
    for engine in ("lds", "streamed"):
        csv = str(tmp_path / (engine + ".csv"))
        r = subprocess.run([os.path.join(drivers, "acg_eval"), "--H", os.path.join(DATA, "H05.txt"), "--G", os.path.join(DATA, "G05.txt"), "--snrs", "-2,0",
                            "--tests", "1000", "--noise", "device", "--no-bp", "--no-admm", "--qms-engine", engine, "--qms-iters", "15", "--out", csv],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert "Algo: QMS" in r.stdout
        lines = open(csv).read().strip().split("\n")
        assert lines[0].startswith("Method,SNR,Sigma,FER,Time,") and len(lines) == 3
        rows[engine] = [[x for k, x in enumerate(l.split(",")) if k != 4] for l in lines[1:]]
    assert rows["lds"] == rows["streamed"], rows
    assert all(r[0] == "QMS" for r in rows["streamed"]) and 0 < float(rows["streamed"][0][3]) < 1
