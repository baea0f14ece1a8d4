"""CPU: the host side of the quantiser grid (acg_ldpc_mc_run_quants, run_experiment_quants) — that the points of
tests/quant_grid_cases.py tell a right kernel from a wrong one under the restatement, the refusals that need no device, and
the conversion of the Python call's `quants`.  The kernel is held to the restatement, counter for counter, in
tests/test_quant_grid_gpu.py."""
import ctypes as C

import pytest

import layered_q_cases as Q
import quant_grid_cases as G


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    return A


# ------------------------------------------------------------------------------------------------ (a) the points separate
@pytest.mark.parametrize("name", ["H05", "qc4x24z27"])
def test_restatement_tells_the_points_apart(A, name):
    """the default decodes some frames and fails others; at least three distinct `correct` counts over the points, so one
    point's quantiser used for all of them is caught; the duplicate of the default gets the default's counters"""
    c = Q.case(A, name)
    cws = G.case_words(c)
    got = {k: G.ref_counters(c, G.POINTS[k], G.FIRST, G.FRAMES, cws) for k in G.NAMES}
    for k, v in got.items():
        assert v[2] == G.FRAMES, (k, v)
    assert 0 < got["default"][0] < G.FRAMES, got["default"]
    assert len({v[0] for v in got.values()}) >= 3, got
    assert got["default again"] == got["default"]
    assert G.POINTS["default again"] == G.POINTS["default"] and len(G.LIST) <= 8
    # every point but the duplicate differs from the default, the four single-field ones in what their name says
    diff = {k: [i for i in range(7) if G.POINTS[k][i] != G.DEFAULT[i]] for k in G.NAMES}
    assert (diff["step 0.3"], diff["ch_bits 4"], diff["msg 5 post 10"], diff["offset 0"]) == ([0], [1], [2, 3], [6])
    for k in G.NAMES:
        assert A.lib().acg_ldpc_quant_check(C.byref(A._lib.Quant(*G.POINTS[k]))) == 0, k


# ------------------------------------------------------------------------------------------------ (b) host-only refusals
def test_refusals_that_need_no_device(A):
    """null handle, null quants, n_points = 0: non-zero, the message, and res as it was.  (The call checks these before it looks
    at the handle, so a block of zeros stands in for one where the handle is not what is refused.)"""
    L = A.lib()
    cfg = A._lib.McCfg()
    cfg.frames = 10
    cfg.snr = 1.0
    q = (A._lib.Quant * 2)(A._lib.Quant(*G.DEFAULT), A._lib.Quant(*G.DEFAULT))
    not_a_handle = C.create_string_buffer(4096)
    for what, h, quants, n_points, word in (("null handle", None, q, 2, "null argument"),
                                            ("null quants", not_a_handle, None, 2, "null argument"),
                                            ("no points", not_a_handle, q, 0, "n_points must be >= 1"),
                                            ("negative points", not_a_handle, q, -3, "n_points must be >= 1")):
        res = (A._lib.McResult * 2)()
        for r in res:
            r.correct, r.total, r.time_sec = -7, -7, -7.0
        rc = L.acg_ldpc_mc_run_quants(h, C.byref(cfg), quants, n_points, res)
        msg = L.acg_ldpc_last_error().decode()
        assert rc != 0 and word in msg, (what, rc, msg)
        assert all((r.correct, r.total, r.time_sec, r.sum_iters) == (-7, -7, -7.0, 0) for r in res), what
    assert L.acg_ldpc_mc_run_quants(not_a_handle, None, q, 2, (A._lib.McResult * 2)()) != 0
    assert L.acg_ldpc_mc_run_quants(not_a_handle, C.byref(cfg), q, 2, None) != 0


# ------------------------------------------------------------------------------------------------ (c) Python conversion
def test_python_conversion_of_quants(A):
    """tuples, dicts and QuantConfig give the same structs; a dict leaves the fields it does not name at their defaults; a
    tuple of another length and a decoder of another class are refused before anything is created"""
    want = G.LIST
    as_cfg = [A.QuantConfig(*v) for v in want]
    names = ("llr_step", "ch_bits", "msg_bits", "post_bits", "scale_num", "scale_shift", "offset")
    as_dict = [dict(zip(names, v)) for v in want]
    mixed = [as_cfg[0], want[1], as_dict[2], list(want[3])] + as_cfg[4:]

    def values(arr, n):
        return [tuple(getattr(arr[k], f) for f in names) for k in range(n)]
    for form in (want, as_cfg, as_dict, mixed):
        arr = A.quant_structs(form)
        assert len(arr) == len(want) and C.sizeof(arr) == 32 * len(want)
        assert values(arr, len(want)) == [tuple(v) for v in want]
    assert values(A.quant_structs([dict(offset=0)]), 1) == [G.POINTS["offset 0"]]
    assert values(A.quant_structs([{}]), 1) == [G.DEFAULT]
    assert len(A.quant_structs([])) == 1                      # (never a zero-length ctypes array)
    with pytest.raises(A.LdpcError, match=r"quants\[1\]"):
        A.quant_structs([want[0], (0.5, 6, 6)])
    with pytest.raises(A.LdpcError, match="QuantizedMinSumDecoder"):
        A.run_experiment_quants(A.MinSumDecoder(5), None, None, 1.0, want, frames=8)
