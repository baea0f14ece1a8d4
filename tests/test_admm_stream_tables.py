"""Streamed QP-ADMM engine (csrc/admm_streamed.hip): its host tables, expanded, are ConstructADMMProblem's A and b.

Host only: compiles tests/admm_stream_tables_check.cpp against csrc/code.cpp with g++ and compares its dump with a numpy
restatement of qp_admm.h:13-102 kept below."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def construct_admm_problem(H):
    """qp_admm.h:13-102 restated: A[i] = [(row, coef), ...] in construction order, b per row."""
    H = np.asarray(H) != 0
    m, n = H.shape
    n_aux = sum(max(int(H[i].sum()) - 3, 0) for i in range(m))
    A = [[] for _ in range(n + n_aux)]
    b = []

    def add_three(i, j, h):
        b.extend([0.0, 0.0, 0.0, 2.0])
        s = len(b)
        for v, cf in ((i, (1, -1, -1, 1)), (j, (-1, 1, -1, 1)), (h, (-1, -1, 1, 1))):
            A[v].extend((s - 4 + r, cf[r]) for r in range(4))

    pos = n
    for i in range(m):
        idx = [int(j) for j in np.nonzero(H[i])[0]]
        if not idx:
            continue
        if len(idx) == 1:
            A[idx[0]].append((len(b), 1))
            b.append(0.0)
            continue
        if len(idx) == 2:
            b.extend([0.0, 0.0])
            s = len(b)
            A[idx[0]] += [(s - 2, 1), (s - 1, -1)]
            A[idx[1]] += [(s - 2, -1), (s - 1, 1)]
            continue
        last = idx[0]
        for j in range(1, len(idx) - 2):
            aux = pos
            pos += 1
            add_three(last, idx[j], aux)
            last = aux
        add_three(last, idx[-2], idx[-1])
    return A, b


def ragged_graph():
    """degree-1 and degree-2 checks, one check of degree 40, one variable of degree 20, no isolated variable"""
    rng = np.random.default_rng(5)
    m, n = 60, 120
    H = np.zeros((m, n), dtype=np.uint8)
    H[0, 0] = 1                      # degree-1 check
    H[1, [1, 2]] = 1                 # degree-2 checks
    H[2, [3, 4]] = 1
    H[3, 5:45] = 1                   # degree 40
    H[4:24, 45] = 1                  # variable 45 in 20 checks
    for i in range(4, m):
        H[i, rng.choice(np.arange(46, n), size=rng.integers(3, 7), replace=False)] = 1
    for j in range(n):               # cover every column
        if not H[:, j].any():
            H[rng.integers(4, m), j] = 1
    return H


def write_txt(H, path):
    with open(path, "w") as f:
        for row in np.asarray(H):
            f.write(",".join(str(int(x != 0)) for x in row) + "\n")


def read_txt(path):
    rows = [ln.strip().rstrip(",") for ln in open(path) if ln.strip()]
    return np.array([[1 if t.strip() == "1" else 0 for t in r.split(",")] for r in rows], dtype=np.uint8)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("admm_stream") / "admm_stream_tables_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "admm_stream_tables_check.cpp"),
                           os.path.join(ROOT, "acg_alp_ldpc_amd", "csrc", "code.cpp"), "-o", out])
    return out


def matrices(tmp):
    from acg_alp_ldpc_amd.codes import regular_ldpc
    out = {name: (os.path.join(ROOT, "data", name + ".txt"), None) for name in ("H05", "optimalH")}
    for name, H in (("configs4", regular_ldpc(5000, 10000, 3, 6, seed=1)), ("ragged", ragged_graph())):
        p = os.path.join(tmp, name + ".txt")
        write_txt(H, p)
        out[name] = (p, H)
    return out


def test_stream_tables_expand_to_construct_admm_problem(exe, tmp_path):
    for name, (path, H) in matrices(str(tmp_path)).items():
        if H is None:
            H = read_txt(path)
        A, b = construct_admm_problem(H)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, name + ": " + r.stdout[-2000:] + r.stderr
        lines = r.stdout.splitlines()
        n_var, n_con = (int(x) for x in lines[0].split())
        assert (n_var, n_con) == (len(A), len(b)), name
        got_A, got_R = {}, {}
        for ln in lines[1:]:
            f = ln.split()
            if f[0] == "A":
                v = [int(x) for x in f[2:]]
                got_A[int(f[1])] = list(zip(v[0::2], v[1::2]))
            else:
                v = [int(x) for x in f[3:]]
                got_R[int(f[1])] = (float(f[2]), list(zip(v[0::2], v[1::2])))
        # v-update: A[i] in construction order, coefficients included (qp_admm.h:134-138)
        for i in range(n_var):
            assert got_A[i] == A[i], (name, i)
        # row update: b_j, then the terms of row j in ascending variable order (qp_admm.h:145-151)
        rows = [[] for _ in range(n_con)]
        for i in range(n_var):
            for j, cf in A[i]:
                rows[j].append((i, cf))
        assert sorted(got_R) == list(range(n_con)), name
        for j in range(n_con):
            assert got_R[j] == (b[j], rows[j]), (name, j)
