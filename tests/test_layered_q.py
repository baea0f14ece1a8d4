"""CPU: the host side of the fixed-point layered min-sum engine (acg_ldpc_quant, acg_ldpc_quant_check, the refusal of
acg_ldpc_decoder_create_quantized without a device) and the sanity of its numpy restatement (tests/layered_q_ref.py) against the
float restatement tests/layered_ref.py.  No device needed.  The kernel is held to the restatement, frame for frame, in
tests/test_layered_q_gpu.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import layered_q_cases as Q
from layered_q_ref import check_update, layered_minsum_q, quantize_llr
from layered_ref import layered_minsum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    return A


def _quant(A, *v):
    return A._lib.Quant(*v)


def test_quant_struct_defaults_and_check(A):
    """sizeof 32, acg_ldpc_quant_default = (0.5, 6, 6, 8, 1, 0, 1), and acg_ldpc_quant_check: the default and the other two
    quantisers of the tests pass; one violation of every rule is refused with a message"""
    L = A.lib()
    assert C.sizeof(A._lib.Quant) == 32
    q = A._lib.Quant()
    L.acg_ldpc_quant_default(C.byref(q))
    got = (q.llr_step, q.ch_bits, q.msg_bits, q.post_bits, q.scale_num, q.scale_shift, q.offset)
    assert got == (0.5, 6, 6, 8, 1, 0, 1) == Q.QUANTS["default"] == A.QuantConfig().as_tuple()
    assert L.acg_ldpc_quant_check(C.byref(q)) == 0
    for v in Q.QUANTS.values():
        assert L.acg_ldpc_quant_check(C.byref(_quant(A, *v))) == 0, v
    assert L.acg_ldpc_quant_check(C.byref(_quant(A, 0.125, 16, 8, 16, 256, 8, 127))) == 0          # every upper limit at once
    assert L.acg_ldpc_quant_check(C.byref(_quant(A, 1e-3, 2, 2, 2, 1, 0, 0))) == 0                 # every lower limit
    assert L.acg_ldpc_quant_check(None) != 0
    bad = {
        "llr_step zero": (0.0, 6, 6, 8, 1, 0, 1), "llr_step negative": (-0.5, 6, 6, 8, 1, 0, 1),
        "llr_step infinite": (math.inf, 6, 6, 8, 1, 0, 1), "llr_step NaN": (math.nan, 6, 6, 8, 1, 0, 1),
        "ch_bits below 2": (0.5, 1, 6, 8, 1, 0, 1), "ch_bits above post_bits": (0.5, 9, 6, 8, 1, 0, 1),
        "post_bits above 16": (0.5, 6, 6, 17, 1, 0, 1),
        "msg_bits below 2": (0.5, 6, 1, 8, 1, 0, 0), "msg_bits above 8": (0.5, 6, 9, 12, 1, 0, 1),
        "msg_bits above post_bits": (0.5, 4, 6, 5, 1, 0, 1),
        "scale_shift negative": (0.5, 6, 6, 8, 1, -1, 1), "scale_shift above 8": (0.5, 6, 6, 8, 1, 9, 1),
        "scale_num zero": (0.5, 6, 6, 8, 0, 2, 1), "scale_num above 2^shift": (0.5, 6, 6, 8, 5, 2, 1),
        "offset negative": (0.5, 6, 6, 8, 1, 0, -1), "offset above Rmax": (0.5, 6, 6, 8, 1, 0, 32),
    }
    for what, v in bad.items():
        rc = L.acg_ldpc_quant_check(C.byref(_quant(A, *v)))
        msg = L.acg_ldpc_last_error().decode()
        assert rc != 0 and "invalid quantiser" in msg, (what, rc, msg)


def test_create_quantized_without_a_device_is_an_error_not_a_crash(A):
    """the library has no CPU decode path: on a machine without a HIP device the create call says so; host-side refusals (a bad
    quantiser, a parameter the engine does not take, a check of 33 variables) come first and need no device either"""
    L = A.lib()
    H = A.read_pcm(os.path.join(ROOT, "data", "H05.txt"))

    def create(code, q, **kw):
        p = A._lib.Params()
        L.acg_ldpc_params_default(C.byref(p))
        p.algo, p.schedule, p.max_iter = A._lib.ALGO_MINSUM, A.SCHEDULE_LAYERED, 10
        for k, v in kw.items():
            setattr(p, k, v)
        h = C.c_void_p()
        rc = L.acg_ldpc_decoder_create_quantized(code._h, C.byref(p), C.byref(q) if q is not None else None, C.byref(h))
        msg = L.acg_ldpc_last_error().decode()
        if rc == 0:
            L.acg_ldpc_decoder_destroy(h)
        return rc, msg, h.value
    good = _quant(A, *Q.QUANTS["default"])
    rc, msg, h = create(H, good)
    if A.device_available():
        assert rc == 0, msg
    else:
        assert rc != 0 and "no CPU fallback" in msg and not h, (rc, msg)
    Hm33 = np.zeros((2, 40), dtype=np.uint8)
    Hm33[0, :33] = 1
    Hm33[1, 30:] = 1
    for what, code, q, kw, word in (("null quantiser", H, None, {}, "null"),
                                    ("bad quantiser", H, _quant(A, 0.5, 6, 9, 8, 1, 0, 1), {}, "invalid quantiser"),
                                    ("flooding", H, good, dict(schedule=A.SCHEDULE_FLOODING), "schedule"),
                                    ("sum-product", H, good, dict(algo=A._lib.ALGO_BP), "algo"),
                                    ("fp16", H, good, dict(precision=A.PREC_F16), "precision"),
                                    ("streamed", H, good, dict(engine=A.ENGINE_STREAMED), "engine"),
                                    ("32 lanes", H, good, dict(lanes_per_frame=32), "lanes_per_frame"),
                                    ("degree 33", A.ParityCheckMatrix(Hm33), good, {}, "degree above 32")):
        rc, msg, h = create(code, q, **kw)
        assert rc != 0 and word in msg and not h, (what, rc, msg)


def test_python_class_forces_layered_minsum_and_keys_the_cache_on_the_quantiser(A):
    dec = A.QuantizedMinSumDecoder(10)
    p = dec._params()
    assert (p.algo, p.schedule, p.max_iter) == (A._lib.ALGO_MINSUM, A.SCHEDULE_LAYERED, 10) and dec.name() == "QMS"
    assert dec.quant == A.QuantConfig() and A.QuantizedMinSumDecoder(10, quant=dict(offset=0)).quant.offset == 0
    Hm = np.eye(3, dtype=np.uint8)
    k0 = dec._key(Hm)
    dec.quant = A.QuantConfig(*Q.QUANTS["scaled"])
    assert dec._key(Hm) != k0 and dec._key(Hm)[-7:] == Q.QUANTS["scaled"]


def test_restatement_arithmetic_on_hand_made_checks():
    """check_update on values worked out by hand, default quantiser (Rmax 31, Pmax 127, offset 1) unless said otherwise"""
    d = Q.QUANTS["default"]
    # degree 3, no old messages: magnitudes 5, 2, 9 -> m1 = 2, m2 = 5; offset 1; signs: q = (+, -, +), XOR = 1
    pn, rn, loud = check_update(np.array([5, -2, 9]), np.zeros(3, dtype=np.int64), d)
    assert list(rn) == [-1, 4, -1] and list(pn) == [4, 2, 8] and loud          # odd parity AND a flip
    # a tie at the minimum: both get m1
    pn, rn, loud = check_update(np.array([3, 3, 7]), np.zeros(3, dtype=np.int64), d)
    assert list(rn) == [2, 2, 2] and list(pn) == [5, 5, 9] and not loud
    # one variable: the message is normalise(Rmax) = 30; the posterior clips at Pmax
    pn, rn, loud = check_update(np.array([-4]), np.array([0]), d)
    assert list(rn) == [30] and list(pn) == [26] and loud
    pn, rn, loud = check_update(np.array([120]), np.array([0]), d)
    assert list(rn) == [30] and list(pn) == [127] and not loud
    # |q| above Rmax is cut to Rmax before the minima; P = 0 decides 0
    pn, rn, loud = check_update(np.array([100, -90, 0]), np.array([0, 0, 0]), d)
    assert list(rn) == [0, 0, -30] and list(pn) == [100, -90, -30] and loud
    # scale 3/4 rounded half up: 2 -> (6 + 2) >> 2 = 2, 5 -> (15 + 2) >> 2 = 4, 6 -> (18 + 2) >> 2 = 5
    pn, rn, loud = check_update(np.array([5, 2, 6]), np.zeros(3, dtype=np.int64), Q.QUANTS["scaled"])
    assert list(rn) == [2, 4, 2]
    # the quantiser: half-integers to even, clamp at +-31, NaN -> 0, infinities -> +-31
    t = np.array([0.25, 0.75, 1.25, -0.25, -0.75, 15.5, 15.75, -15.75, 1e30, np.inf, -np.inf, np.nan, 0.0], dtype=np.float32)
    assert list(quantize_llr(t, d)) == [0, 2, 2, 0, -2, 31, 31, -31, 31, 31, -31, 0, 0]


@pytest.fixture(scope="module")
def h05_2000(A):
    """2000 frames of random H05 codewords (data/G05.txt) at -2 dB and the sets of layers_wide()"""
    H = A.read_pcm(os.path.join(ROOT, "data", "H05.txt"))
    G = A.read_pcm(os.path.join(ROOT, "data", "G05.txt")).dense()
    cws = A.gen_random_codewords(G, 2000, 239239239)
    Hm = np.array(H.dense())
    assert not (cws @ Hm.T.astype(np.int64) % 2).any()
    assert cws.any(axis=1).all() and 0.4 < cws.mean() < 0.6           # no all-zero word: P = 0 decides 0 and would flatter the integers
    Z, layers = H.layers_wide()
    assert Z == 20
    y = A.transmit_frames(cws, -2.0)
    fb, fok, _ = layered_minsum(Hm, layers, y, -2.0, 15, 0.75)
    return Hm, layers, cws, y, int((fok == 0).sum() + ((fok == 1) & (fb != cws).any(axis=1)).sum())


@pytest.mark.parametrize("qname", ["default", "scaled"])
def test_restatement_frame_failures_agree_with_float_minsum(h05_2000, qname):
    """frame failures (no word, or a word that is not the sent one) of the integer restatement and of layered_minsum(scale 0.75)
    on the same 2000 frames, 15 iterations: within 3 sqrt(fail_q + fail_float).  A wrong sign or shift gives FER ~ 1."""
    Hm, layers, cws, y, fail_f = h05_2000
    b, ok, it = layered_minsum_q(Hm, layers, y, -2.0, 15, Q.QUANTS[qname])
    fail_q = int((ok == 0).sum() + ((ok == 1) & (b != cws).any(axis=1)).sum())
    print("H05 -2 dB, 2000 frames, 15 iterations: frame failures float %d, %s %d" % (fail_f, qname, fail_q))
    assert 0 < fail_f < 1000
    assert abs(fail_q - fail_f) <= 3.0 * math.sqrt(fail_q + fail_f), (fail_q, fail_f)
    assert ((b[ok == 1] @ Hm.T.astype(np.int64)) % 2 == 0).all()      # ok = 1 words are codewords
    assert not b[ok == 0].any() and (it[ok == 0] == 15).all()


@pytest.mark.parametrize("name", sorted(Q.CASES))
def test_gpu_cases_give_both_exits_in_the_restatement(A, name):
    """at the SNR of every case of tests/test_layered_q_gpu.py the restatement with the default quantiser decodes some frames
    and fails others"""
    c = Q.case(A, name)
    ok = c.ref("default")[1]
    assert 0 < ok.sum() < len(ok), (name, int(ok.sum()))
    if name == "diag10":
        deg = sorted(int(c.Hm[l[l >= 0]].sum(axis=1)[0]) for l in c.layers)
        assert deg == Q.DIAG_DEGREES and c.Z == 0 and c.width == 1
    if name == "qc2x10z300":
        assert c.width == 300


def test_cxx_mirror_compiles_and_links(A, tmp_path):
    """acg_ldpc::QuantizedMinSumDecoder (include/acg_ldpc_decoder.hpp) with plain g++ against the C-ABI library; the program decodes
    only where it finds a device (tests/test_layered_q_gpu.py)"""
    import subprocess
    A.lib()
    exe = Q.build_cxx_check(tmp_path)
    out = subprocess.run([exe, os.path.join(ROOT, "data", "H05.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "m=160 n=280 E=860 quant=0.5,6,6,8,1,0,1 check=0 sizeof=32" in out.stdout and "name=QMS" in out.stdout
