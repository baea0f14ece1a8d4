"""acg_optimize_h --batch K: proposals drawn ahead and scored together must leave the search exactly what it is with
--batch 1 — the same proposal sequence (CPU, through --dump-proposals) and the same stdout and saved matrix (GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "drivers", "bin")
DATA = os.path.join(ROOT, "data")


@pytest.fixture(scope="module")
def exe():
    import acg_alp_ldpc_amd as A
    A.build()
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools", "drivers")], stdout=subprocess.DEVNULL)
    return os.path.join(BIN, "acg_optimize_h")


def dump(exe, *extra):
    out = subprocess.run([exe, "--init", os.path.join(DATA, "H05.txt"), "--dump-proposals", "64"] + list(extra), capture_output=True,
                         text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 64
    return lines


def python_chain(seed, count, J):
    """the sequential proposal chain of optimize_H.cpp:66-75, 89-104 restated here, independent of the driver:
    numpy's legacy RandomState(seed) is std::mt19937(seed) and its full-range uint32 draws are the raw outputs"""
    import numpy as np
    import acg_alp_ldpc_amd as A
    H = A.read_pcm(os.path.join(DATA, "H05.txt")).dense()
    Zc, Rr, Cc = 20, H.shape[0] // 20, H.shape[1] // 20
    present = np.array([[bool(H[i * Zc, j * Zc:(j + 1) * Zc].any()) for j in range(Cc)] for i in range(Rr)])
    raw = iter(int(x) for x in np.random.RandomState(seed).randint(0, 2 ** 32, 4 * count, dtype=np.uint32))
    lines = []
    for it in range(count):
        i, j = next(raw) % Rr, next(raw) % Cc
        pres = present[i, j]
        if not pres or next(raw) % 2 == 0:
            pres = not pres
        shift = next(raw) % Zc
        lines.append("%d %d %d %d" % (i, j, int(pres), shift))
        if J > 0 and (it + 1) % J == 0:
            present[i, j] = pres
    return lines


@pytest.mark.parametrize("J", [0, 1, 7])
def test_batched_generator_draws_the_sequential_proposals(exe, J):
    """every J-th proposal accepted (0: none): the batched generator, which draws K proposals from the current matrix and
    rewinds the mt19937 to the state behind the accepted one, prints what the sequential generator prints"""
    want = dump(exe, "--batch", "1", "--accept-every", str(J))
    assert want == python_chain(239, 64, J)
    if J == 0:
        assert want == dump(exe)                    # today's all-rejected chain
    if J == 1:
        assert want == dump(exe, "--accept-all")    # today's all-accepted chain
    for K in (1, 5, 16):
        assert dump(exe, "--batch", str(K), "--accept-every", str(J)) == want, K


def search(exe, tmp_path, noise, K, seed):
    out = tmp_path / ("H_%s_%d.txt" % (noise, K))
    p = subprocess.run([exe, "--random", "4,8", "--Z", "20", "--iters", "24", "--tests", "200", "--admm-iters", "100", "--noise", noise,
                        "--seed", str(seed), "--batch", str(K), "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p.stdout, (out.read_bytes() if out.exists() else b"")


@pytest.mark.gpu
@pytest.mark.parametrize("noise", ["host", "device"])
def test_batched_search_is_the_sequential_search(exe, tmp_path, noise):
    one, saved = search(exe, tmp_path, noise, 1, SEED)
    lines = one.splitlines()
    assert lines[0].startswith("initial FER=") and sum(l.startswith("\tproposal") for l in lines) == 24
    # an acceptance that is not the first proposal of its batch, for K = 5 and K = 16: walk the batches as the driver does
    for K in (5, 16):
        props = [i for i, l in enumerate(lines) if l.startswith("\tproposal")]
        accepted = {props.index(i - 1) for i, l in enumerate(lines) if l.startswith("accept")}
        start, inner = 0, False
        for k in range(24):
            if k in accepted:
                inner = inner or k != start
                start = k + 1
            elif k - start + 1 == K:
                start = k + 1
        assert inner, "pick a --seed whose search accepts inside a batch of %d" % K
    assert saved
    for K in (5, 16):
        assert search(exe, tmp_path, noise, K, SEED) == (one, saved), K


SEED = 239
