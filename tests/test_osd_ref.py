"""CPU: the numpy restatement of ordered-statistics decoding (tests/osd_ref.py) against an independent textbook implementation
(most-reliable basis by elimination on a GENERATOR matrix, then re-encoding), against brute force on the (7,4) Hamming code,
and the properties every frame must have.  No device needed.  The kernel is held to the restatement, frame for frame, in
tests/test_osd_gpu.py."""
import itertools
import os

import numpy as np
import pytest

import osd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "data")

HAMMING = np.array([[1, 0, 1, 0, 1, 0, 1],
                    [0, 1, 1, 0, 0, 1, 1],
                    [0, 0, 0, 1, 1, 1, 1]], dtype=np.uint8)


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    return A


def null_space(Hm):
    """a generator matrix of the code of H: a basis of its null space over GF(2), by elimination (independent of osd_ref)"""
    Hm = (np.asarray(Hm) != 0).astype(np.uint8)
    m, n = Hm.shape
    M = Hm.copy()
    piv, r = [], 0
    for c in range(n):
        rows = np.flatnonzero(M[r:, c]) + r
        if not len(rows):
            continue
        M[[r, rows[0]]] = M[[rows[0], r]]
        for k in np.flatnonzero(M[:, c]):
            if k != r:
                M[k] ^= M[r]
        piv.append(c)
        r += 1
        if r == m:
            break
    free = [c for c in range(n) if c not in piv]
    G = np.zeros((len(free), n), dtype=np.uint8)
    for i, f in enumerate(free):
        G[i, f] = 1
        for k, c in enumerate(piv):
            G[i, c] = M[k, f]
    assert not (G.astype(np.int64) @ Hm.T % 2).any()
    return G


def textbook_osd(G, s, order):
    """Fossorier-Lin on the generator matrix: columns by DESCENDING reliability (the reverse of the restatement's order), the first
    k independent ones are the most reliable basis; hard decisions there, re-encoded; order 1 flips one basis position at a time."""
    s = np.asarray(s).astype(np.int64)
    z, r = (s < 0).astype(np.uint8), np.minimum(np.abs(s), 32767)
    k, n = G.shape
    desc = np.argsort(-((r << 16) | np.arange(n)), kind="stable")
    M = G.copy()
    basis, row = [], 0
    for c in desc:
        rows = np.flatnonzero(M[row:, c]) + row
        if not len(rows):
            continue
        M[[row, rows[0]]] = M[[rows[0], row]]
        for q in np.flatnonzero(M[:, c]):
            if q != row:
                M[q] ^= M[row]
        basis.append(c)
        row += 1
        if row == k:
            break
    basis = np.array(basis)   # M[:, basis] is the identity: a message u encodes to u @ M with word[basis] = u
    encode = lambda u: (u.astype(np.int64) @ M.astype(np.int64) % 2).astype(np.uint8)
    metric = lambda w: int(r[w != z].sum())
    u0 = z[basis]
    best = encode(u0)
    best_M, iters = metric(best), 0
    if order == 1:
        for j in sorted(basis):
            u = u0.copy()
            u[np.flatnonzero(basis == j)[0]] ^= 1
            w = encode(u)
            if metric(w) < best_M:
                best, best_M, iters = w, metric(w), 1
    return best, iters, best_M


def _frames(rng, n, F, scale):
    """soft values with ties: BPSK of the all-zero word through noise, coarsely quantised"""
    y = 1.0 + rng.normal(0, scale, (F, n))
    return np.clip(np.round(y * 8), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("name", ["H05", "H"])
def test_restatement_equals_the_textbook_construction(A, name):
    Hm = np.array(A.read_pcm(os.path.join(DATA, name + ".txt")).dense())
    G = null_space(Hm)
    rng = np.random.default_rng(5)
    s = _frames(rng, Hm.shape[1], 40, 0.9)
    for order in (0, 1):
        w, it, M = R.osd(Hm, s, order)
        for f in range(len(s)):
            tw, tit, tM = textbook_osd(G, s[f], order)
            assert (w[f] == tw).all() and it[f] == tit and M[f] == tM, (name, order, f)
    assert it.any() and not it.all()


def test_hamming_against_brute_force():
    G = null_space(HAMMING)
    words = np.array([(np.array(u) @ G % 2) for u in itertools.product((0, 1), repeat=4)], dtype=np.uint8)
    rng = np.random.default_rng(7)
    s = np.concatenate([_frames(rng, 7, 150, 1.0), rng.integers(-2, 3, (150, 7)).astype(np.int16)])
    improved = 0
    for f in range(len(s)):
        ml = min(R.metric_of(w, s[f]) for w in words)
        w0, _, M0 = R.osd(HAMMING, s[f], 0)
        w1, _, M1 = R.osd(HAMMING, s[f], 1)
        assert ml <= M1[0] <= M0[0]
        improved += M1[0] < M0[0]
    assert improved > 0


@pytest.mark.parametrize("name", ["H05", "H", "hamming"])
def test_properties_of_every_frame(A, name):
    Hm = HAMMING if name == "hamming" else np.array(A.read_pcm(os.path.join(DATA, name + ".txt")).dense())
    n = Hm.shape[1]
    rng = np.random.default_rng(11)
    s = np.concatenate([_frames(rng, n, 20, 0.9), rng.integers(-2, 3, (10, n)).astype(np.int16),
                        np.zeros((1, n), np.int16), np.full((1, n), -32768, np.int16)])
    for order in (0, 1):
        w, it, M = R.osd(Hm, s, order)
        assert not (w.astype(np.int64) @ Hm.T % 2).any(), "not a codeword"
        for f in range(len(s)):
            z, _ = R.reliabilities(s[f])
            I = R.information_set(Hm, s[f])
            differ = np.flatnonzero((w[f] != z) & I)
            assert len(differ) == it[f] <= order            # agrees with z on I \ T, |T| = iters
            assert M[f] == R.metric_of(w[f], s[f])
        assert (R.osd(Hm, s, 0)[2] >= R.osd(Hm, s, 1)[2]).all()


def test_soft_values():
    y = np.array([0.0, -0.0, 1.0, -1.0, 7.9997, 7.99976, 8.0, -8.0, 100.0, -100.0, np.nan, np.inf, -np.inf, 1e-40, -1e-40, 1e300, -1e300,
                  0.000244140625, 0.00024414, -0.000244140625, 2.5 / 4096, -2.5 / 4096])
    want = [0, 0, 4096, -4096, 32766, 32767, 32767, -32767, 32767, -32767, 0, 32767, -32767, 0, 0, 32767, -32767, 1, 0, -1, 2, -2]
    assert R.soft_values(y).tolist() == want
    assert R.soft_values(y.astype(np.float32)).tolist() == want
    with pytest.raises(ValueError):
        R.osd(HAMMING, np.zeros((1, 7), np.int16), 2)
