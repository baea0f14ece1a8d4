"""GPU: acg_eval with ordered-statistics decoding.  --osd-order K adds an OSD block and one row per SNR, --cascade qms,osd one
more block and row per SNR behind them, with the figures of the Python mirror on the same frames; without the new flags the
report holds the rows it always held."""
import os
import subprocess

import pytest

import layered_q_cases as Q

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data")


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


def _strip(text):   # (without the Time column)
    return [",".join(l.split(",")[:4] + l.split(",")[5:]) for l in text.strip().splitlines()]


def test_eval_driver_rows(A, tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "drivers")], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "tools", "drivers", "bin", "acg_eval")
    base = [exe, "--H", os.path.join(DATA, "H05.txt"), "--G", os.path.join(DATA, "G05.txt"), "--snrs", "-2,-1", "--tests", "400",
            "--bp-iters", "10", "--no-admm"]
    plain = subprocess.run(base + ["--out", str(tmp_path / "a.csv")], capture_output=True, text=True, timeout=120)
    osd = subprocess.run(base + ["--out", str(tmp_path / "b.csv"), "--cascade", "qms,osd", "--osd-order", "1", "--qms-iters", "5"],
                         capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and osd.returncode == 0, plain.stderr + osd.stderr
    a, b = _strip((tmp_path / "a.csv").read_text()), _strip((tmp_path / "b.csv").read_text())
    assert len(a) == 1 + 2 and b[:len(a)] == a and len(b) == len(a) + 2 + 2
    assert "Algo: OSD" in osd.stdout and "Algo: QMS+OSD" in osd.stdout
    assert "OSD" not in plain.stdout and "OSD" not in (tmp_path / "a.csv").read_text()
    drop_time = lambda out: [l.split(", (time=")[0] for l in out.splitlines()]
    assert drop_time(osd.stdout)[:len(plain.stdout.splitlines())] == drop_time(plain.stdout)
    c = Q.case(A, "H05")
    dec = A.OSDDecoder(1)
    cas = A.CascadeDecoder(A.QuantizedMinSumDecoder(5), A.OSDDecoder(1))
    try:
        for k, snr in enumerate((-2.0, -1.0)):
            f = b[len(a) + k].split(",")
            r = A.run_experiment(dec, c.cws, c.H, snr, noise="host")
            assert f[0] == "OSD" and float(f[1]) == snr and abs(float(f[3]) - r.FER()) < 1e-9
            f = b[len(a) + 2 + k].split(",")
            total, _, _ = A.run_experiment_cascade(cas, c.cws, c.H, snr, noise="host")
            assert f[0] == "QMS+OSD" and float(f[1]) == snr and abs(float(f[3]) - total.FER()) < 1e-9
    finally:
        dec.close()
        cas.close()
    # order 0, the default --qms-iters, and an unknown stage
    one = subprocess.run([exe, "--H", os.path.join(DATA, "H05.txt"), "--G", os.path.join(DATA, "G05.txt"), "--snrs", "-1", "--tests", "200",
                          "--no-bp", "--no-admm", "--out", str(tmp_path / "c.csv"), "--cascade", "qms,osd", "--osd-order", "0"],
                         capture_output=True, text=True, timeout=120)
    assert one.returncode == 0, one.stderr
    rows = _strip((tmp_path / "c.csv").read_text())
    assert [r.split(",")[0] for r in rows[1:]] == ["OSD", "QMS+OSD"]
    bad = subprocess.run(base + ["--cascade", "qms,turbo"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--cascade A,B" in bad.stderr
    bad = subprocess.run(base + ["--osd-order", "2", "--out", str(tmp_path / "d.csv")], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "max_iter is the order" in bad.stderr
