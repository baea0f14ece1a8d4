"""CPU: the layering of the workgroup-per-frame layered engine (bp_layered_block_build through acg_ldpc_debug_layers_block /
ParityCheckMatrix.layers_block) — sets of checks of one degree that share no variable, of ANY size: the block rows of a
quasi-cyclic H, else first-fit colouring in row order.  No device needed.  The kernel that walks these sets is held to the
restatements of tests/layered_ref.py in tests/test_layered_block_gpu.py."""
import ctypes as C

import numpy as np
import pytest


def ragged_40x80(A):
    """the matrix of test_layered_ragged_graph: an empty check, a degree-3 and a degree-1 check among degree-6 ones, an isolated
    variable (whose checks drop to degree 5)"""
    Hm = A.regular_ldpc(40, 80, 3, 6, seed=5).copy()
    Hm[0, :] = 0
    Hm[1, np.nonzero(Hm[1])[0][:3]] = 0
    Hm[2, np.nonzero(Hm[2])[0][1:]] = 0          # degree 1
    Hm[:, 7] = 0                                  # an isolated variable
    return Hm


def check_sets(Hm, layers):
    """every non-empty check in exactly one set, no variable twice in a set, one degree per set, occupied slots first"""
    Hm = np.asarray(Hm)
    seen = np.zeros(Hm.shape[0], dtype=int)
    for layer in layers:
        ids = layer[layer >= 0]
        assert len(ids) > 0
        seen[ids] += 1
        sub = Hm[ids]
        assert (sub.sum(axis=0) <= 1).all()
        assert len(set(sub.sum(axis=1))) == 1
        assert (layer[len(ids):] == -1).all()
    deg = Hm.sum(axis=1)
    assert (seen[deg > 0] == 1).all() and (seen[deg == 0] == 0).all()
    assert max((l >= 0).sum() for l in layers) == layers.shape[1]      # width = the largest set


def first_fit(Hm):
    """the rule on the host: a check joins the first set of its degree in which none of its variables occurs yet"""
    sets = []
    for r in range(Hm.shape[0]):
        v = np.nonzero(Hm[r])[0]
        if len(v) == 0:
            continue
        for s in sets:
            if s[0] == len(v) and not s[1][v].any():
                break
        else:
            s = (len(v), np.zeros(Hm.shape[1], dtype=bool), [])
            sets.append(s)
        s[1][v] = True
        s[2].append(r)
    return [s[2] for s in sets]


def test_block_layers_of_the_reference_matrices_are_their_block_rows(matrices):
    import acg_alp_ldpc_amd as A
    for name in ("H05", "optimalH"):
        Z, layers = A.ParityCheckMatrix(matrices[name]).layers_block()
        assert (Z, layers.shape) == (20, (8, 20))
        assert (layers == np.arange(160).reshape(8, 20)).all()
        check_sets(matrices[name], layers)


@pytest.mark.parametrize("case", ["384x768", "2000x4000", "ragged"])
def test_block_layers_are_conflict_free_first_fit_sets(case):
    import acg_alp_ldpc_amd as A
    Hm = {"384x768": lambda: A.regular_ldpc(384, 768, 3, 6, seed=1), "2000x4000": lambda: A.regular_ldpc(2000, 4000, 3, 6, seed=2),
          "ragged": lambda: ragged_40x80(A)}[case]()
    Z, layers = A.ParityCheckMatrix(Hm).layers_block()
    assert Z == 0
    check_sets(Hm, layers)
    want = first_fit(np.asarray(Hm))
    assert [list(l[l >= 0]) for l in layers] == want
    sizes = [int((l >= 0).sum()) for l in layers]
    if case == "384x768":
        assert sizes == [68, 68, 65, 61, 55, 45, 20, 2], sizes
    if case == "2000x4000":
        assert max(sizes) > 256, sizes          # wider than the smallest workgroup: the GPU tests run the multi-pass path
        assert max(sizes) == 353, sizes
    if case == "ragged":
        assert len(set(int(Hm[l[l >= 0][0]].sum()) for l in layers)) >= 3


def test_block_layers_refuse_check_degree_nine():
    import acg_alp_ldpc_amd as A
    Hm = np.zeros((3, 20), dtype=np.uint8)
    Hm[0, :9] = 1
    Hm[1, 9:15] = 1
    Hm[2, 15:] = 1
    H = A.ParityCheckMatrix(Hm)
    nl, w, Z = C.c_int32(), C.c_int32(), C.c_int32()
    rc = A.lib().acg_ldpc_debug_layers_block(H._h, C.byref(nl), C.byref(w), C.byref(Z), None, 0)
    assert rc != 0 and b"degree" in A.lib().acg_ldpc_last_error()
    with pytest.raises(A.LdpcError):
        H.layers_block()
    Hm[0, 8] = 0                                  # degree 8 is accepted
    Z, layers = A.ParityCheckMatrix(Hm).layers_block()
    assert layers.shape[0] == 3 and Z == 0
