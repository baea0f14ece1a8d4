"""CPU: the integer entrance of the fixed-point layered min-sum engine (acg_ldpc_quantize_dev, acg_ldpc_decode_batch_q_dev,
acg_ldpc_decode_batch_q; QuantizedMinSumDecoder.decode_llr_batch) — its restatement tests/layered_q_io_ref.py tied to the pinned
restatement tests/layered_q_ref.py, the meaning of "the latched posterior", and what the library and the Python wrapper refuse
without a device.  The kernel is held to the restatement, value for value, in tests/test_layered_q_io_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import layered_q_cases as Q
import layered_q_io_cases as IO
from layered_q_io_ref import clamp_channel, decode_int
from layered_q_ref import limits


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    return A


@pytest.mark.parametrize("qname", sorted(Q.QUANTS))
@pytest.mark.parametrize("name", sorted(Q.CASES))
def test_decode_int_of_quantised_symbols_is_the_pinned_restatement(A, name, qname):
    """decode_int(quantize(y)) = layered_minsum_q(y) in word, flag and iteration; (post < 0) is the word of every ok frame;
    |post| <= Pmax; max_iter = 0 returns the clamped input"""
    c = Q.case(A, name)
    quant = Q.QUANTS[qname]
    cmax, _, pmax = limits(quant)
    bits, ok, iters, post = IO.ref(A, name, qname)
    wb, wok, wit = c.ref(qname)
    assert (ok == wok).all() and (iters == wit).all() and (bits == wb).all(), (name, qname)
    assert post.dtype == np.int16 and post.shape == bits.shape and np.abs(post.astype(np.int32)).max() <= pmax
    assert ((post < 0)[ok == 1] == (bits[ok == 1] == 1)).all()
    ch = IO.channel(A, name, qname)
    assert np.abs(ch.astype(np.int32)).max() <= cmax
    b0, ok0, it0, p0 = IO.ref(A, name, qname, 0)
    assert not ok0.any() and not b0.any() and (it0 == 0).all() and (p0 == ch).all()
    # beyond the range: -32768 and 32767 start from -Cmax and +Cmax
    wide = ch[:8].astype(np.int32) * 1000
    wide[0, :2] = (-32768, 32767)
    got = decode_int(c.Hm, c.layers, wide.astype(np.int16), 0, quant)[3]
    assert (got == clamp_channel(wide, quant)).all() and tuple(got[0, :2]) == (-cmax, cmax)


@pytest.mark.parametrize("name", IO.MOVING)
def test_latched_posterior_is_not_the_final_state(A, name):
    """a variant of the restatement that goes on sweeping latched frames (what copying P out at the end of a fixed-work run would
    return): its posteriors differ from decode_int's on at least half of the frames that latch before max_iter, its word, flag
    and iteration on none.  So the device's early_exit = 0 runs of these cases tell the two apart."""
    c = Q.case(A, name)
    bits, ok, iters, post = IO.ref(A, name, "default")
    vb, vok, vit, vpost = IO.ref(A, name, "default", keep_sweeping=True)
    assert (vb == bits).all() and (vok == ok).all() and (vit == iters).all()
    early = (ok == 1) & (iters < c.iters)
    moved = (vpost != post).any(axis=1)
    print("%s: %d of %d frames that latch before iteration %d have other posteriors when swept on" % (name, int((moved & early).sum()), int(early.sum()), c.iters))
    assert early.sum() >= 100 and 2 * (moved & early).sum() >= early.sum(), (name, int((moved & early).sum()), int(early.sum()))
    assert not moved[ok == 0].any()                     # a frame that never latched has run every iteration either way


def test_library_has_the_three_symbols_and_refuses_a_null_handle(A):
    """no device needed: each entry point returns non-zero with a message for a null handle"""
    L = A.lib()
    buf = np.zeros(8, dtype=np.int16)
    y = np.zeros(8)
    out = np.zeros(8, dtype=np.uint8)
    for what, rc in (("quantize_dev", L.acg_ldpc_quantize_dev(None, y.ctypes.data, 1, 8, 0.0, buf.ctypes.data, None)),
                     ("decode_batch_q_dev", L.acg_ldpc_decode_batch_q_dev(None, buf.ctypes.data, 1, out.ctypes.data, out.ctypes.data, None, None, None)),
                     ("decode_batch_q", L.acg_ldpc_decode_batch_q(None, buf.ctypes.data, 1, out.ctypes.data, out.ctypes.data, None, None)),
                     ("decode_batch_q, no frames", L.acg_ldpc_decode_batch_q(None, None, 0, None, None, None, None))):
        msg = L.acg_ldpc_last_error().decode()
        assert rc != 0 and "null decoder" in msg, (what, rc, msg)
    for name in ("acg_ldpc_quantize_dev", "acg_ldpc_decode_batch_q_dev", "acg_ldpc_decode_batch_q"):
        assert name in A._lib.SYMBOLS and getattr(L, name).restype is C.c_int


def test_cxx_mirror_compiles_and_links(A, tmp_path):
    """the integer entrance's members of acg_ldpc::QuantizedMinSumDecoder with plain g++ against the C-ABI library; the program
    decodes only where it finds a device (tests/test_layered_q_io_gpu.py)"""
    import os
    import subprocess
    A.lib()
    exe = IO.build_cxx_io_check(tmp_path)
    out = subprocess.run([exe, os.path.join(IO.ROOT, "data", "H05.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "m=160 n=280 E=860 null handle: null decoder" in out.stdout


def test_python_wrapper_refuses_floats_and_values_outside_int16(A):
    """before any handle is made: unquantised LLRs (a floating-point array) are a TypeError, integers beyond int16 a ValueError"""
    dec = A.QuantizedMinSumDecoder(5)
    Hm = Q.diag10()
    n = Hm.shape[1]
    with pytest.raises(TypeError, match="integer channel values"):
        dec.decode_llr_batch(Hm, np.zeros((2, n)))
    with pytest.raises(TypeError, match="integer channel values"):
        dec.decode_llr_batch(Hm, np.zeros((2, n), dtype=np.float32))
    for v in (32768, -32769):
        c = np.zeros((2, n), dtype=np.int32)
        c[1, 3] = v
        with pytest.raises(ValueError, match="int16"):
            dec.decode_llr_batch(Hm, c)
    assert dec.live_handles() == 0
