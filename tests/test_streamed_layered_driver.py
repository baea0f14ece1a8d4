"""acg_eval --layered-streamed: the rows of the streamed float layered engine equal A.run_experiment on StreamedLayeredBPDecoder /
StreamedLayeredMinSumDecoder for the same host-noise frames — every column but the wall time; a bad value exits 2."""
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


@pytest.mark.parametrize("value", ["spa", "bp,", "minsum,bp", ""])
def test_eval_driver_refuses_an_unknown_value(drivers, tmp_path, value):
    r = subprocess.run([os.path.join(drivers, "acg_eval"), "--H", os.path.join(DATA, "H05.txt"), "--layered-streamed", value,
                        "--out", str(tmp_path / "r.csv")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--layered-streamed bp, minsum or bp,minsum" in r.stderr, (r.returncode, r.stderr)


@pytest.mark.gpu
def test_eval_driver_rows_are_run_experiment(drivers, oracle, tmp_path):
    import acg_alp_ldpc_amd as A
    F, snrs = 300, (-2.0, -1.0)
    csv = str(tmp_path / "r.csv")
    r = subprocess.run([os.path.join(drivers, "acg_eval"), "--H", os.path.join(DATA, "H05.txt"), "--snrs", ",".join(str(s) for s in snrs), "--tests", str(F),
                        "--noise", "host", "--no-bp", "--no-admm", "--layered-streamed", "bp,minsum", "--bp-iters", "20", "--minsum-iters", "15",
                        "--ms-scale", "0.8", "--out", csv], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = open(csv).read().strip().split("\n")
    assert lines[0] == "Method,SNR,Sigma,FER,Time,AvgHamming,AvgHammingCorrect,AvgHammingWrong"
    # (--minsum-iters also asks for the flooding min-sum: its rows come first; the engine's blocks are the last two)
    assert len(lines) == 1 + 6 and r.stdout.count("Algo: MS") == 2 and r.stdout.count("Algo: BP") == 1
    rows = [l.split(",") for l in lines[-4:]]
    assert [x[0] for x in rows] == ["BP", "BP", "MS", "MS"]
    Hm = oracle.read_pcm(os.path.join(DATA, "H05.txt"))
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 239239239, F)
    H = A.ParityCheckMatrix(Hm)
    decs = [A.StreamedLayeredBPDecoder(20), A.StreamedLayeredMinSumDecoder(15, 0.8)]
    try:
        k = 0
        for dec in decs:
            for snr in snrs:
                e = A.run_experiment(dec, cws, H, snr, frames=F, noise="host")
                want = (e.FER(), e.mean_hamming(), e.mean_hamming_ok(), e.mean_hamming_wrong())
                got = tuple(float(rows[k][i]) for i in (3, 5, 6, 7))
                assert float(rows[k][1]) == snr and got == pytest.approx(want, abs=1e-11), (rows[k], want)   # (12 digits in the file)
                assert e.total == F
                k += 1
        assert 0 < float(rows[0][3]) < 1
    finally:
        for dec in decs:
            dec.close()
