"""GPU: the streamed fixed-point layered min-sum engine (acg_ldpc_decoder_create_quantized_streamed, bp_streamed_q_kernel;
StreamedQuantizedMinSumDecoder) against its restatements — tests/layered_q_io_ref.py on the cases of tests/layered_q_cases.py,
tests/streamed_q_ref.py on the codes no other engine takes — and against the LDS engine on every code both accept: word, flag,
exit iteration and EVERY posterior of EVERY frame identical, nothing tolerated."""
import numpy as np
import pytest

import layered_q_cases as Q
import layered_q_io_cases as IO
import streamed_q_cases as S
from layered_q_io_ref import clamp_channel
from layered_q_ref import limits
from streamed_q_ref import decode_int_sparse, edges_of
from test_layered_q_io_gpu import _assert_same4, _dev_decode
from test_layered_block_gpu import _assert_same

pytestmark = pytest.mark.gpu

KERNEL = "bp_streamed_q_kernel"


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


def _dec(A, it, qname="default", ee=True, **kw):
    return A.StreamedQuantizedMinSumDecoder(it, quant=A.QuantConfig(*Q.QUANTS[qname]), early_exit=ee, **kw)


def _lds(A, it, qname="default", ee=True):
    return A.QuantizedMinSumDecoder(it, quant=A.QuantConfig(*Q.QUANTS[qname]), early_exit=ee)


# ------------------------------------------------------------------------------------------------ 1. equals the restatement
@pytest.mark.parametrize("qname", sorted(Q.QUANTS))
@pytest.mark.parametrize("name", sorted(Q.CASES))
def test_equals_restatement(A, name, qname):
    """every case x quantiser, early exit and fixed work (on the cases of IO.MOVING the fixed-work run tells the latched
    posterior from the final state); then 0 and 1 iterations: max_iter = 0 fails every frame with the clamped channel value as
    its posterior"""
    c = Q.case(A, name)
    ch = IO.channel(A, name, qname)
    want = IO.ref(A, name, qname)
    for ee in (True, False):
        dec = _dec(A, c.iters, qname, ee)
        try:
            _assert_same4(dec.decode_llr_batch(c.H, ch), want, (name, qname, "early exit" if ee else "fixed work"))
            d = dec.describe(c.H)
            assert "kernel=%s " % KERNEL in d and "schedule=layered" in d and "engine=streamed" in d, d
            assert dec.name() == "QMS"
        finally:
            dec.close()
    for it in (0, 1):
        w = IO.ref(A, name, qname, it)
        for ee in (True, False):
            dec = _dec(A, it, qname, ee)
            try:
                got = dec.decode_llr_batch(c.H, ch)
                _assert_same4(got, w, (name, qname, "max_iter", it, ee))
                if it == 0:
                    assert not got[1].any() and not got[0].any() and (got[2] == 0).all() and (got[3] == ch).all()
            finally:
                dec.close()
    if qname == "default":
        assert 0 < want[1].sum() < len(want[1])


# -------------------------------------------------------------------------------------------------- 2. equals the LDS engine
@pytest.mark.parametrize("qname", sorted(Q.QUANTS))
@pytest.mark.parametrize("name", sorted(Q.CASES))
def test_equals_lds_engine(A, name, qname):
    """the same channel values through decode_llr_batch of both engines"""
    c = Q.case(A, name)
    ch = IO.channel(A, name, qname)
    lds, dec = _lds(A, c.iters, qname), _dec(A, c.iters, qname)
    try:
        want = lds.decode_llr_batch(c.H, ch)
        assert "kernel=bp_layered_q_kernel " in lds.describe(c.H)
        _assert_same4(dec.decode_llr_batch(c.H, ch), want, (name, qname))
    finally:
        lds.close()
        dec.close()


# ------------------------------------------------------------------------------------------------------------ 3. wide checks
@pytest.mark.parametrize("name", ["deg48", "deg40"])
def test_wide_checks(A, name):
    w = S.wide(A, name)
    with pytest.raises(A.LdpcError, match="degree above 32"):
        _lds(A, w.iters).handle(w.H)
    for qname in sorted(Q.QUANTS):
        for ee in (True, False):
            dec = _dec(A, w.iters, qname, ee)
            try:
                _assert_same4(dec.decode_llr_batch(w.H, w.channel(qname)), w.ref(qname), (name, qname, ee))
            finally:
                dec.close()
    ok = w.ref("default")[1]
    assert 0 < ok.sum() < w.frames


# ------------------------------------------------------------------------------------------------------------- 4. beyond LDS
def test_beyond_lds(A):
    """2050 x 41 000, check degree 40: 164 000 bytes of state per frame.  The LDS engine's create call still refuses it."""
    w = S.wide(A, "big")
    lds = _lds(A, w.iters)
    with pytest.raises(A.LdpcError, match="degree above 32"):
        lds.handle(w.H)
    assert lds.live_handles() == 0
    dec = _dec(A, w.iters)
    try:
        _assert_same4(dec.decode_llr_batch(w.H, w.channel()), w.ref(), "big")
        assert "state_bytes_per_frame=164000 " in dec.describe(w.H)
        lay = dec.layout(w.H)
        assert lay["lds_bytes_per_frame"] == 0 and lay["lanes_per_frame"] == 1 and lay["frames_per_block"] % 64 == 0
    finally:
        dec.close()
    ok = w.ref()[1]
    assert 0 < ok.sum() < w.frames, int(ok.sum())


def test_beyond_lds_low_degree_is_refused_by_the_lds_engine_for_size(A):
    """the matrix of test_layered_q_gpu's "frame beyond LDS" refusal (n = 82 000, two checks of 32): refused there for its size,
    decoded here"""
    Hm = np.zeros((2, 82000), dtype=np.uint8)
    Hm[0, :32] = 1
    Hm[1, -32:] = 1
    lds = _lds(A, 3)
    with pytest.raises(A.LdpcError, match="does not fit in LDS"):
        lds.handle(Hm)
    rng = np.random.default_rng(5)
    ch = rng.integers(-31, 32, size=(5, 82000)).astype(np.int16)
    want = decode_int_sparse(edges_of(Hm), 82000, [[0], [1]], ch, 3)
    dec = _dec(A, 3)
    try:
        _assert_same4(dec.decode_llr_batch(Hm, ch), want, "n = 82000")
    finally:
        dec.close()
    assert 0 < want[1].sum() < 5, want[1]


# ---------------------------------------------------------------------------------------- 5. frame counts and reuse of a slab
def test_frame_counts_and_slab_reuse(A, monkeypatch):
    """1, 63, 64, 65 frames, and 3 T + 5 on a handle of TWO tiles (ACG_STREAMQ_TILES=2): every slab is used twice, by frames that
    latch at other iterations and fail elsewhere.  Then another decode of other frames on the same handle."""
    monkeypatch.setenv("ACG_STREAMQ_TILES", "2")
    c = Q.case(A, "H05")
    ch = IO.channel(A, "H05", "default")
    want = IO.ref(A, "H05", "default")
    dec = _dec(A, c.iters)
    try:
        d = dec.describe(c.H)
        assert " tiles=2 " in d, d
        T = dec.layout(c.H)["frames_per_block"]
        assert " T=%d " % T in d and dec.layout(c.H)["grid_blocks"] == 2
        for F in (1, 63, 64, 65, 3 * T + 5):
            assert F <= c.frames
            _assert_same4(dec.decode_llr_batch(c.H, ch[:F]), tuple(a[:F] for a in want), ("frames", F))
        lo = c.frames - (3 * T + 5)
        _assert_same4(dec.decode_llr_batch(c.H, ch[lo:]), tuple(a[lo:] for a in want), "second decode")
        # the order reversed: a slab's second occupant is not the one it had before
        _assert_same4(dec.decode_llr_batch(c.H, ch[::-1]), tuple(a[::-1] for a in want), "reversed")
        assert dec.live_handles() == 1
    finally:
        dec.close()


# --------------------------------------------------------------------------------------------------------------- 6. edge inputs
def test_edge_inputs(A):
    """channel values of -32768 and 32767 (clamped to -+Cmax), variables in no check, a one-variable check (m2 = Rmax)"""
    Hm = np.concatenate([Q.diag10(), np.zeros((len(Q.DIAG_DEGREES), 3), dtype=np.uint8)], axis=1)
    Hm[1, -1] = 1                                     # the check of two variables gets a third, far from its others
    n = Hm.shape[1]
    rng = np.random.default_rng(3)
    ch = rng.integers(-40, 41, size=(130, n)).astype(np.int16)
    ch[:, 0] = rng.choice(np.array([-32768, 32767, -1, 0, 1], dtype=np.int16), 130)      # the one-variable check
    ch[::3, -2] = -32768                              # an unconnected variable
    ch[1::3, -3] = 32767
    ch[5] = -32768
    H = A.ParityCheckMatrix(Hm)
    for qname in sorted(Q.QUANTS):
        quant = Q.QUANTS[qname]
        want = decode_int_sparse(edges_of(Hm), n, H.layers_any()[1], ch, 5, quant)
        dec = _dec(A, 5, qname)
        try:
            got = dec.decode_llr_batch(H, ch)
            _assert_same4(got, want, ("edge inputs", qname))
            cm = limits(quant)[0]
            assert (got[3][:, -2] == clamp_channel(ch[:, -2], quant)).all() and got[3][0, -2] == -cm
            assert ((got[0][:, -2] == 1) == (ch[:, -2] < 0))[got[1] == 1].all()
        finally:
            dec.close()


# ---------------------------------------------------------------------------------------------- 7. input types and streams
@pytest.mark.parametrize("f32", [False, True])
def test_symbol_entrances(A, f32):
    """double and float symbols through the host entrance and through decode_batch_dev = the restatement's quantiser followed
    by the integer path; quantize_dev = the restatement's quantiser"""
    import torch
    c = Q.case(A, "H05")
    y = c.y.astype(np.float32) if f32 else c.y
    want = c.ref("default", symbols_f32=f32)
    dec = _dec(A, c.iters)
    try:
        _assert_same(dec.decode_batch(c.H, y, c.snr), want, ("host", f32))
        F, nw = c.frames, (c.n + 31) // 32
        yd = torch.from_numpy(y).cuda()
        cd = torch.full((F, c.n), -777, dtype=torch.int16, device="cuda")
        bits = torch.zeros((F, nw), dtype=torch.int32, device="cuda")
        ok = torch.zeros(F, dtype=torch.uint8, device="cuda")
        it = torch.zeros(F, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        dec.decode_batch_dev(c.H, yd.data_ptr(), not f32, F, c.snr, bits.data_ptr(), ok.data_ptr(), it.data_ptr())
        dec.quantize_dev(c.H, yd.data_ptr(), not f32, F * c.n, c.snr, cd.data_ptr())
        dec.sync(c.H)
        words = bits.cpu().numpy().view(np.uint32)
        got = (((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.uint8).reshape(F, nw * 32)[:, :c.n], ok.cpu().numpy(), it.cpu().numpy())
        _assert_same(got, want, ("device", f32))
        if not f32:
            assert (cd.cpu().numpy() == IO.channel(A, "H05", "default")).all()
    finally:
        dec.close()


def test_symbol_entrance_in_chunks(A, monkeypatch):
    """one tile: the symbol entrance stages T frames at a time"""
    monkeypatch.setenv("ACG_STREAMQ_TILES", "1")
    c = Q.case(A, "H05")
    dec = _dec(A, c.iters)
    try:
        _assert_same(dec.decode_batch(c.H, c.y, c.snr), c.ref("default"), "chunks")
    finally:
        dec.close()


def test_two_streams(A):
    """two launches of one handle on two streams, neither waited for in between: the slabs belong to the handle, so the second
    is ordered behind the first on the device, and both are right"""
    import torch
    c = Q.case(A, "H05")
    ch = IO.channel(A, "H05", "default")
    want = IO.ref(A, "H05", "default")
    F, nw, h = c.frames, (c.n + 31) // 32, c.frames // 2
    dec = _dec(A, c.iters)
    try:
        dec.handle(c.H)
        s = [torch.cuda.Stream(), torch.cuda.Stream()]
        part = [slice(0, h), slice(h, F)]
        cd = [torch.from_numpy(np.array(ch[p])).cuda() for p in part]
        bits = [torch.zeros((p.stop - p.start, nw), dtype=torch.int32, device="cuda") for p in part]
        ok = [torch.zeros(p.stop - p.start, dtype=torch.uint8, device="cuda") for p in part]
        it = [torch.zeros(p.stop - p.start, dtype=torch.int32, device="cuda") for p in part]
        post = [torch.zeros((p.stop - p.start, c.n), dtype=torch.int16, device="cuda") for p in part]
        torch.cuda.synchronize()
        for k in (0, 1, 0, 1):
            dec.decode_llr_batch_dev(c.H, cd[k].data_ptr(), part[k].stop - part[k].start, bits[k].data_ptr(), ok[k].data_ptr(), it[k].data_ptr(),
                                     post[k].data_ptr(), s[k].cuda_stream)
        torch.cuda.synchronize()
        for k in (0, 1):
            words = bits[k].cpu().numpy().view(np.uint32)
            b = ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.uint8).reshape(-1, nw * 32)[:, :c.n]
            _assert_same4((b, ok[k].cpu().numpy(), it[k].cpu().numpy(), post[k].cpu().numpy()), tuple(a[part[k]] for a in want), ("stream", k))
    finally:
        dec.close()


def test_null_outputs(A):
    """the device entrance with no iteration and no posterior buffer"""
    c = Q.case(A, "diag10")
    ch = IO.channel(A, "diag10", "default")
    want = IO.ref(A, "diag10", "default")
    dec = _dec(A, c.iters)
    try:
        b, ok, it, post = _dev_decode(dec, c.H, ch, want_post=False, want_iters=False)
        assert it is None and post is None and (b == want[0]).all() and (ok == want[1]).all()
        _assert_same4(_dev_decode(dec, c.H, ch), want, "diag10, device")
        _dev_decode(dec, c.H, ch[:0])
    finally:
        dec.close()


# -------------------------------------------------------------------------------------------------------------- 8. Monte-Carlo
def test_monte_carlo_counters_equal_the_lds_engine(A):
    """acg_ldpc_mc_run and _detail with device noise on H05: the seven counters of an LDS-engine handle with the same parameters"""
    c = Q.case(A, "H05")
    F, first, seed = 1024, (1 << 33) + 5, 2
    cws = c.cws[:7]
    fields = ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong", "sum_iters")
    res = []
    for dec in (_lds(A, c.iters), _dec(A, c.iters)):
        try:
            r = A.run_experiment(dec, cws, c.H, c.snr, frames=F, first_frame=first, noise="device", seed=seed)
            d = A.run_experiment_detail(dec, cws, c.H, c.snr, frames=F, first_frame=first, noise="device", seed=seed, cap=5)
            res.append((tuple(getattr(r, f) for f in fields), tuple(getattr(d, f) for f in fields), d.bit_errors, list(d.events["frame"])))
        finally:
            dec.close()
    assert res[0] == res[1], res
    assert res[1][0] == res[1][1] and res[1][0][2] == F and 0 < res[1][0][0] < F


# ----------------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_on_a_live_handle(A):
    c = Q.case(A, "H05")
    L = A.lib()
    dec = _dec(A, 10)
    try:
        h, _ = dec.handle(c.H)
        with pytest.raises(A.LdpcError, match="streamed quantized engine has no grid form"):
            A.run_experiment_quants(dec, None, c.H, c.snr, [Q.QUANTS["default"]], frames=64, noise="device")
        with pytest.raises(A.LdpcError, match="QP-ADMM"):
            A.run_experiment_grid(dec, None, c.H, c.snr, [1.0], [0.5], frames=64, noise="device")
        buf = np.zeros((2, c.n), dtype=np.int16)
        out = np.zeros((2, c.n), dtype=np.uint8)
        for what, rc in (("frames < 0", L.acg_ldpc_decode_batch_q(h, buf.ctypes.data, -1, out.ctypes.data, out.ctypes.data, None, None)),
                         ("null c", L.acg_ldpc_decode_batch_q(h, None, 2, out.ctypes.data, out.ctypes.data, None, None)),
                         ("null bits", L.acg_ldpc_decode_batch_q(h, buf.ctypes.data, 2, None, out.ctypes.data, None, None)),
                         ("dev, null c", L.acg_ldpc_decode_batch_q_dev(h, None, 2, None, None, None, None, None)),
                         ("quantize, null y", L.acg_ldpc_quantize_dev(h, None, 1, 8, 0.0, None, None))):
            assert rc != 0 and L.acg_ldpc_last_error(), what
        assert L.acg_ldpc_decode_batch_q(h, None, 0, None, None, None, None) == 0
        # and the handle still decodes
        ch = IO.channel(A, "H05", "default")
        _assert_same4(dec.decode_llr_batch(c.H, ch[:70]), tuple(a[:70] for a in IO.ref(A, "H05", "default", 10)), "after the refusals")
    finally:
        dec.close()
    for what, d, word in (("fused", A.StreamedQuantizedMinSumDecoder(10, engine=A.ENGINE_FUSED), "engine"),
                          ("lanes", A.StreamedQuantizedMinSumDecoder(10, lanes_per_frame=64), "lanes_per_frame"),
                          ("flooding", A.StreamedQuantizedMinSumDecoder(10, schedule=A.SCHEDULE_FLOODING), "schedule"),
                          ("msg_bits 9", A.StreamedQuantizedMinSumDecoder(10, quant=dict(msg_bits=9, post_bits=12)), "invalid quantiser")):
        with pytest.raises(A.LdpcError, match=word):
            d.handle(c.H)
        assert d.live_handles() == 0, what
    ok = A.StreamedQuantizedMinSumDecoder(10, engine=A.ENGINE_STREAMED)
    try:
        assert "engine=streamed" in ok.describe(c.H)
    finally:
        ok.close()


# ------------------------------------------------------------------------------------------------------------ 10. C++ mirror
def test_cxx_mirror_decodes(A, tmp_path):
    """tests/cxx_streamed_q_check.cpp: two H05 frames of channel values through acg_ldpc::StreamedQuantizedMinSumDecoder and
    through acg_ldpc::QuantizedMinSumDecoder, all four outputs equal"""
    import os
    import subprocess
    exe = S.build_cxx_check(tmp_path)
    out = subprocess.run([exe, os.path.join(Q.ROOT, "data", "H05.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "same=1 " in out.stdout and "kernel=%s " % KERNEL in out.stdout, out.stdout
