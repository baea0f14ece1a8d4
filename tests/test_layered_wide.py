"""CPU: the layering of the wide-check layered engine (bp_layered_block_build with the degree cap 32, through
acg_ldpc_debug_layers_wide / ParityCheckMatrix.layers_wide) on the four codes of tests/layered_wide_cases.py — the rule of
layers_block() (block rows of a quasi-cyclic H, else first-fit colouring of same-degree checks in row order) for checks of up to
32 variables.  No device needed.  The kernel that walks these sets is held to the restatements of tests/layered_ref.py in
tests/test_layered_wide_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import layered_wide_cases as W
from layered_ref import host_phi, layered_minsum, layered_sumproduct_exact
from test_layered_block import check_sets, first_fit


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_wide_layers_are_conflict_free_same_degree_sets(name):
    """every check exactly once, the checks of a set share no variable and have one degree; qc_Z is the circulant size for the
    quasi-cyclic cases (the sets are the block rows) and 0 for `ragged` (first-fit colouring)"""
    import acg_alp_ldpc_amd as A
    Hm = np.array(W.matrix(name))
    Z, layers = A.ParityCheckMatrix(Hm).layers_wide()
    assert Z == W.CASES[name][1]
    check_sets(Hm, layers)
    deg = Hm.sum(axis=1)
    if Z:
        assert (layers == np.arange(Hm.shape[0]).reshape(-1, Z)).all()
    else:
        assert [list(l[l >= 0]) for l in layers] == first_fit(Hm)
    if name == "qc4x24z27":
        assert Hm.shape == (108, 648) and set(deg) == {22, 23} and set(Hm.sum(axis=0)) == {3, 4}
    if name == "qc6x32z64":
        assert Hm.shape == (384, 2048) and set(deg) == {32} and int(Hm.sum()) == 12288
    if name == "qc2x10z300":
        assert Hm.shape == (600, 3000) and set(deg) == {10} and layers.shape == (2, 300)
    if name == "ragged":
        assert Hm.shape == (60, 400) and (Hm.sum(axis=0) > 0).all()
        assert {8, 9, 16, 17} <= set(deg) and deg.min() == 3 and deg.max() == 19


def test_wide_layers_refuse_check_degree_33_and_accept_32():
    import acg_alp_ldpc_amd as A
    Hm = np.zeros((3, 50), dtype=np.uint8)
    Hm[0, :33] = 1
    Hm[1, 33:42] = 1
    Hm[2, 42:] = 1
    H = A.ParityCheckMatrix(Hm)
    nl, w, Z = C.c_int32(), C.c_int32(), C.c_int32()
    rc = A.lib().acg_ldpc_debug_layers_wide(H._h, C.byref(nl), C.byref(w), C.byref(Z), None, 0)
    msg = A.lib().acg_ldpc_last_error()
    assert rc != 0 and b"degree" in msg and b"32" in msg, msg
    with pytest.raises(A.LdpcError):
        H.layers_wide()
    Hm[0, 32] = 0                                  # degree 32 is accepted
    H = A.ParityCheckMatrix(Hm)
    Z, layers = H.layers_wide()
    assert Z == 0 and sorted(int(Hm[l[l >= 0]].sum(axis=1)[0]) for l in layers) == [8, 9, 32]
    with pytest.raises(A.LdpcError, match="degree above 8"):      # the narrow engine's layering refuses as before
        H.layers_block()


def test_ragged_snr_gives_both_exits_in_the_restatement(oracle):
    """the SNR of `ragged` was chosen from the restatements alone: at +3.0 dB, 25 iterations, 200 frames, min-sum and sum-product
    (host phi) both decode some frames and fail others"""
    import acg_alp_ldpc_amd as A
    Hm = np.array(W.matrix("ragged"))
    snr = W.CASES["ragged"][2]
    assert snr == 3.0
    Z, layers = A.ParityCheckMatrix(Hm).layers_wide()
    y = oracle.transmit_frames(np.zeros((200, Hm.shape[1]), dtype=np.uint8), snr, first_seed=1)
    for ok in (layered_minsum(Hm, layers, y, snr, 25, 0.75)[1], layered_sumproduct_exact(Hm, layers, y, snr, 25, host_phi)[1]):
        assert 0 < ok.sum() < 200, int(ok.sum())
