"""CPU: the rate-matched Monte-Carlo run (acg_ldpc_mc_run_rm, acg_ldpc_rm_channel_dev; experiment.run_experiment_rm,
rate_match_pattern; acg_eval --puncture / --shorten) — what is decided without a device: the symbols and their bindings, the
refusal that comes first, the pattern helper, the driver's flag refusals, and tests/rm_ref.py against hand-written values.  The
device is held to rm_ref, value for value and counter for counter, in tests/test_rm_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import layered_q_cases as Q
import rm_cases as RM
import rm_ref
from layered_q_ref import limits

BIN = os.path.join(RM.ROOT, "tools", "drivers", "bin")


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    return A


def test_symbols_are_exported_and_bound_as_the_header_declares(A):
    L = A.lib()
    header = open(os.path.join(RM.ROOT, "include", "acg_ldpc.h")).read()
    want = {"acg_ldpc_mc_run_rm": ("acg_ldpc_decoder *dec, const acg_ldpc_mc_cfg *cfg, const uint8_t *pattern, acg_ldpc_mc_result *res", 4),
            "acg_ldpc_rm_channel_dev": ("acg_ldpc_decoder *dec, const acg_ldpc_mc_cfg *cfg, const uint8_t *pattern, void *out_dev, int32_t *raw_dev, "
                                        "void *stream", 6)}
    for name, (args, count) in want.items():
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m and " ".join(m.group(1).split()) == args, name
        res, argtypes = A._lib.SYMBOLS[name]
        assert res is C.c_int and len(argtypes) == count and getattr(L, name).restype is C.c_int
    assert (A._lib.RM_SENT, A._lib.RM_PUNCTURED, A._lib.RM_SHORTENED) == (0, 1, 2)
    for k, v in (("ACG_LDPC_RM_SENT", 0), ("ACG_LDPC_RM_PUNCTURED", 1), ("ACG_LDPC_RM_SHORTENED", 2)):
        assert re.search(r"\b%s = %d\b" % (k, v), header), k
    assert "not rescaled by the pattern" in header and "Not provided: host (mt19937) noise" in header


def test_null_arguments_are_refused_first_and_without_a_device(A):
    """refusal 1 of the header's order: a null dec, cfg, res or out_dev, whatever else is handed over — a bad cfg, host noise and a
    bad pattern byte included, which come later in the order and need a handle"""
    from acg_alp_ldpc_amd._lib import McCfg, McResult
    L = A.lib()
    bad = McCfg()
    bad.frames, bad.noise = -1, A._lib.NOISE_HOST_MT19937
    pat = np.full(8, 9, dtype=np.uint8)
    res = McResult()
    res.total = 77
    out = np.zeros(8, dtype=np.float32)
    for what, rc in (("run_rm, all null", L.acg_ldpc_mc_run_rm(None, None, None, None)),
                     ("run_rm, null dec", L.acg_ldpc_mc_run_rm(None, C.byref(bad), pat.ctypes.data, C.byref(res))),
                     ("channel_dev, all null", L.acg_ldpc_rm_channel_dev(None, None, None, None, None, None)),
                     ("channel_dev, null dec", L.acg_ldpc_rm_channel_dev(None, C.byref(bad), pat.ctypes.data, out.ctypes.data, None, None))):
        msg = L.acg_ldpc_last_error().decode()
        assert rc != 0 and "null argument" in msg, (what, rc, msg)
    assert res.total == 77 and not out.any()


def test_rate_match_pattern(A):
    p = A.rate_match_pattern(10, punctured=(1, 7), shortened=[9])
    assert p.dtype == np.uint8 and p.tolist() == [0, 1, 0, 0, 0, 0, 0, 1, 0, 2]
    assert A.rate_match_pattern(5).tolist() == [0] * 5
    assert A.rate_match_pattern(4, shortened=range(4)).tolist() == [2] * 4
    assert A.rate_match_pattern(6, punctured=np.array([5, 5])).tolist() == [0, 0, 0, 0, 0, 1]
    with pytest.raises(ValueError, match="index 3 is both"):
        A.rate_match_pattern(8, punctured=(2, 3), shortened=(3, 4))
    for bad in ((8,), (-1,)):
        with pytest.raises(ValueError, match="outside"):
            A.rate_match_pattern(8, punctured=bad)
        with pytest.raises(ValueError, match="outside"):
            A.rate_match_pattern(8, shortened=bad)
    for name in RM.CASES:
        n = {"H05": 280, "deg40": 400, "odd62": 62}[name]
        pun, sho = RM.positions(name, n)
        assert pun and sho and not set(pun) & set(sho)
    assert [len(x) for x in RM.positions("H05", 280)] == [14, 14] and [len(x) for x in RM.positions("deg40", 400)] == [4, 40]


def test_python_wrapper_refuses_a_bad_pattern_before_any_handle_is_made(A):
    Hm = np.array(A.regular_ldpc(31, 62, 3, 6, seed=1))
    dec = A.StreamedLayeredMinSumDecoder(5, 0.75)
    for bad, err in ((np.zeros(61, dtype=np.uint8), "n = 62"), (np.zeros((62, 1), dtype=np.uint8), "n = 62"), (np.zeros(62), "RM_SENT"),
                     (np.full(62, 256), "RM_SENT"), (np.full(62, -1), "RM_SENT")):
        with pytest.raises(ValueError, match=err):
            A.run_experiment_rm(dec, None, Hm, 1.0, pattern=bad, frames=4)
    assert dec.live_handles() == 0


@pytest.fixture(scope="module")
def drivers(A):
    A.lib()
    subprocess.check_call(["make", "-C", os.path.join(RM.ROOT, "tools", "drivers")], stdout=subprocess.DEVNULL)
    return BIN


@pytest.mark.parametrize("flags,message", [
    (["--puncture", "3"], "need an engine with a channel-value entrance"),
    (["--shorten", "3", "--minsum-iters", "5", "--noise", "device"], "need an engine with a channel-value entrance"),
    (["--puncture", "3", "--qms-iters", "5"], "device noise only"),
    (["--puncture", "3", "--qms-engine", "lds", "--noise", "host"], "device noise only"),
    (["--shorten", "3", "--layered-streamed", "bp", "--noise", "host"], "device noise only"),
    (["--puncture", "3", "--qms-engine", "lds", "--noise", "device", "--cascade", "qms,osd"], "do not go with"),
    (["--puncture", "3", "--qms-engine", "lds", "--noise", "device", "--osd-order", "1"], "do not go with"),
    (["--shorten", "3", "--layered-streamed", "minsum", "--noise", "device", "--detail"], "do not go with"),
    (["--puncture", "3,,4", "--qms-iters", "5", "--noise", "device"], "comma-separated indices and a-b ranges"),
    (["--puncture", "7-3", "--qms-iters", "5", "--noise", "device"], "comma-separated indices and a-b ranges"),
    (["--shorten", "x", "--qms-iters", "5", "--noise", "device"], "comma-separated indices and a-b ranges"),
    (["--shorten", "", "--qms-iters", "5", "--noise", "device"], "comma-separated indices and a-b ranges"),
    (["--shorten", "5,280", "--qms-iters", "5", "--noise", "device"], "index 280 is outside the code"),
    (["--puncture", "3-6", "--shorten", "6", "--qms-iters", "5", "--noise", "device"], "index 6 is listed twice"),
])
def test_eval_driver_refuses_before_a_device_is_looked_for(drivers, tmp_path, flags, message):
    r = subprocess.run([os.path.join(drivers, "acg_eval"), "--H", os.path.join(RM.DATA, "H05.txt"), "--out", str(tmp_path / "r.csv")] + flags,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and message in r.stderr and "Algo:" not in r.stdout, (r.returncode, r.stderr)


# ---- rm_ref against hand-written values ------------------------------------------------------------------------------------
SNR0 = 10 * np.log10(2.0)      # sigma^2 = 1 / 4: llr = 8 y exactly in every format


def test_rm_ref_float_values_by_hand():
    y = np.array([[0.5, -0.25, np.nan, np.inf, -np.inf, 1.0, 1.0, -1.0]], dtype=np.float32)
    sent = np.array([[0, 1, 0, 0, 1, 1, 0, 1]], dtype=np.uint8)
    pat = np.array([0, 0, 0, 0, 0, 2, 2, 1], dtype=np.uint8)
    got = rm_ref.channel_values(y, sent, SNR0, pat)
    assert got.dtype == np.float32
    want = np.array([[4.0, -2.0, np.nan, np.inf, -np.inf, -1048576.0, 1048576.0, 0.0]], dtype=np.float32)
    assert np.isnan(got[0, 2]) and (np.delete(got, 2, 1).view(np.uint32) == np.delete(want, 2, 1).view(np.uint32)).all(), got
    assert not np.signbit(got[0, 7])      # punctured: +0, whatever the symbol's sign
    # raw errors over the sent positions: y <= 0 for bit 0, y > 0 for bit 1; NaN is on neither side; -inf for bit 1 is right
    assert rm_ref.raw_errors(y, sent, pat).tolist() == [0]
    y2 = np.array([[0.0, -0.0, 0.0, 1e-30, -3.0, 2.0, -1.0, 5.0]], dtype=np.float32)
    s2 = np.array([[0, 0, 1, 1, 0, 1, 0, 1]], dtype=np.uint8)
    assert rm_ref.raw_errors(y2, s2, None).tolist() == [7]          # all wrong but the 0 sent as bit 1
    assert rm_ref.raw_errors(y2, s2, np.array([0, 1, 0, 2, 0, 1, 2, 0], dtype=np.uint8)).tolist() == [3]
    assert rm_ref.channel_values(y, sent, SNR0, None).view(np.uint32).tolist() == rm_ref.channel_values(y, sent, SNR0, np.zeros(8, np.uint8)).view(np.uint32).tolist()


@pytest.mark.parametrize("qname", sorted(Q.QUANTS))
def test_rm_ref_quantised_values_by_hand(qname):
    """Cmax of the three quantisers; a tie at .5 rounds to even; NaN -> 0; +-inf -> +-Cmax; shortened bit 1 -> -Cmax"""
    quant = Q.QUANTS[qname]
    cmax = limits(quant)[0]
    assert cmax == {"default": 31, "scaled": 31, "saturating": 7}[qname]
    step = quant[0]
    # llr = 8 y: y = step * k / 8 gives t = k exactly; k = 0.5, 1.5, 2.5, -0.5, -1.5 are the ties
    ks = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 3.0, 1000.0], dtype=np.float64)
    y = np.concatenate([ks * step / 8, [np.nan, np.inf, -np.inf, 0.3, 0.3, 0.3]]).astype(np.float32)[None, :]
    sent = np.zeros_like(y, dtype=np.uint8)
    sent[0, -2] = 1
    pat = np.zeros(y.shape[1], dtype=np.uint8)
    pat[-3] = rm_ref.PUNCTURED
    pat[-2:] = rm_ref.SHORTENED
    got = rm_ref.channel_values(y, sent, SNR0, pat, quant)
    assert got.dtype == np.int16
    assert got[0].tolist() == [0, 2, 2, 0, -2, 3, cmax, 0, cmax, -cmax, 0, -cmax, cmax], got
    assert rm_ref.raw_errors(y, sent, pat).tolist() == [3]     # the sent positions -0.5, -1.5 and -inf


def test_rm_ref_counters_by_hand():
    sent = np.array([[1, 0, 1], [0, 0, 0], [1, 1, 0], [0, 1, 0]], dtype=np.uint8)
    bits = np.array([[1, 0, 1], [0, 1, 0], [0, 0, 0], [0, 1, 0]], dtype=np.uint8)
    got = rm_ref.counters([2, 5, 1, 7], bits, [1, 1, 0, 0], [3, 4, 9, 9], sent)
    assert got == {"correct": 1, "pseudo": 1, "total": 4, "sum_hamming": 15, "sum_hamming_ok": 2, "sum_hamming_wrong": 13, "sum_iters": 25}
    assert tuple(got) == rm_ref.FIELDS


def test_cxx_mirror_compiles_and_links(A, tmp_path):
    """run_rate_matched of the three C++ classes with plain g++ against the C-ABI library; the program runs only where it finds a device"""
    A.lib()
    exe = RM.build_cxx_check(tmp_path)
    out = subprocess.run([exe, os.path.join(RM.DATA, "H05.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "n=280 null handle: null argument" in out.stdout, out.stdout
