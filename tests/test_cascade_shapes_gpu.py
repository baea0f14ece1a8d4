"""GPU: the hand-over kernels of a two-stage decode (csrc/cascade_kernels.hip) at the shapes production chunks have and
tests/test_cascade_gpu.py (300-400 frames: one tile, no stride; uint4 rows but for the 400 frames of diag10, n = 169, which take
the uint32_t / uint64_t gather) never reaches:

  1  the tile loop of cascade_select_kernel (failures on both sides of every tile boundary), the uint64_t and uint32_t gathers
  2  an odd chunk: ok + f0, iters + f0, stage + f0 at odd frames, and the caller's ok / stage at odd byte addresses
  3  the element-wide gather chosen by the base pointer alone (rows of 16-byte multiples, y_dev shifted by one element)
  4  the chunk cap and across it: 64 tiles, the gather's row loop striding, a second chunk of one frame
  5  the uint16_t gather of the int16 posterior hand-over
  6  the stride loop of cascade_scatter_kernel
  7  acg_ldpc_cascade_mc_run with several tiles per chunk, cascade_sum_iters_kernel behind it

Which frames fail stage 0 is designed (tests/cascade_shapes_cases.py; tests/test_cascade_shapes.py qualifies it on the CPU).  Every
comparison is exact in word, flag, iteration count and stage of every frame: against the two numpy restatements composed (1, 2,
7) and against the two handles run by hand (_compose of tests/test_cascade_gpu.py).  The outputs stand between sentinel rows,
in front and behind, which must survive."""
import ctypes as C

import numpy as np
import pytest

import cascade_shapes_cases as S
import layered_q_cases as Q
from layered_ref import layered_minsum
from mc_decode_path import mc_cfg, sent_words
from mc_detail_ref import mc_detail, pack_bits
from test_cascade_gpu import SEVEN, _cascade_dev, _compose, _counters, _same, _stage_alone

pytestmark = pytest.mark.gpu

HEAD, TAIL = 16, 3        # sentinel rows in front of and behind the F rows of every output


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


def _minsum(A, it):
    return A.MinSumDecoder(it, S.SCALE, schedule=A.SCHEDULE_LAYERED)


@pytest.fixture(scope="module")
def cas(A):
    """stage 0: one layered min-sum iteration; stage 1: twenty"""
    cas = A.CascadeDecoder(_minsum(A, S.ITERS[0]), _minsum(A, S.ITERS[1]))
    yield cas
    cas.close()


def _guarded(A, cas, H, y, snr, y_shift=0, head_flags=HEAD):
    """acg_ldpc_cascade_decode_batch_dev on host symbols y [F, n] with every output at an offset into a longer buffer: HEAD
    sentinel rows in front (head_flags bytes for ok and stage), TAIL behind.  y_shift: y_dev starts that many ELEMENTS into its
    allocation.  -> (words, ok, iters, stage), {name: the device address handed over}"""
    import torch
    from acg_alp_ldpc_amd._lib import check
    h, _ = cas.handle(H)
    F, n = y.shape
    nw = (n + 31) // 32
    flat = np.zeros(y.size + y_shift, dtype=y.dtype)
    flat[y_shift:] = y.reshape(-1)
    yd = torch.from_numpy(flat).cuda()
    bits = torch.full((HEAD + F + TAIL, nw), -1, dtype=torch.int32, device="cuda")
    it = torch.full((HEAD + F + TAIL,), -7, dtype=torch.int32, device="cuda")
    ok = torch.full((head_flags + F + TAIL,), 7, dtype=torch.uint8, device="cuda")
    st = torch.full((head_flags + F + TAIL,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptr = {"y": yd.data_ptr() + y_shift * yd.element_size(), "bits": bits.data_ptr() + HEAD * nw * 4, "ok": ok.data_ptr() + head_flags,
           "iters": it.data_ptr() + HEAD * 4, "stage": st.data_ptr() + head_flags}
    check(A.lib().acg_ldpc_cascade_decode_batch_dev(h, ptr["y"], 1 if y.dtype == np.float64 else 0, F, float(snr), ptr["bits"], ptr["ok"],
                                                    ptr["iters"], ptr["stage"], None))
    torch.cuda.synchronize()
    for name, buf, head, sentinel in (("bits", bits, HEAD, -1), ("iters", it, HEAD, -7), ("ok", ok, head_flags, 7), ("stage", st, head_flags, 9)):
        assert (buf[:head] == sentinel).all(), "%s: a row in front of the batch was written" % name
        assert (buf[head + F:] == sentinel).all(), "%s: a row past the batch was written" % name
    return (bits.cpu().numpy().view(np.uint32)[HEAD:HEAD + F], ok.cpu().numpy()[head_flags:head_flags + F], it.cpu().numpy()[HEAD:HEAD + F],
            st.cpu().numpy()[head_flags:head_flags + F]), ptr


def _layered_kernel(cas, H):
    """both stages walk the sets of ParityCheckMatrix.layers(), which is what the restatement is given"""
    d = cas.describe(H)
    assert d.count("kernel=bp_layered_kernel ") == 2, d


# ------------------------------------------------------------------------------ 1. tile boundaries of the select scan
@pytest.mark.parametrize("dtype,elem", [(np.float64, 8), (np.float32, 4)])
def test_select_scan_over_two_and_ten_tiles(A, cas, dtype, elem, monkeypatch):
    """5 chunks of 2048 frames = two tiles each, every chunk with its own pattern; then the same frames as one chunk of ten
    tiles.  First to reach: the tile loop (the `base` carry, wsum re-used behind the second barrier); the uint64_t gather
    (float64) and the uint32_t gather (float32) on more rows than a tile has."""
    c = S.code(A)
    fail, y, r = S.restated(A, "tiles", dtype)
    F = len(fail)
    assert F == 5 * 2 * S.TILE and y.dtype == dtype and (c.n * elem) % 16 != 0, "the rows must keep the gather off uint4"
    assert (r.ok0 == ~fail).all()
    _layered_kernel(cas, c.H)
    by_hand, K = _compose(A, cas, c.H, y, S.SNR)
    assert K == int(fail.sum())
    _same(by_hand, r.out, ("tiles", dtype.__name__, "the two handles by hand against the restatement"))
    monkeypatch.setenv("ACG_CASCADE_CHUNK", str(2 * S.TILE))
    got, _ = _guarded(A, cas, c.H, y, S.SNR)
    assert "chunk=%d " % (2 * S.TILE) in cas.describe(c.H)
    _same(got, r.out, ("tiles", dtype.__name__, "chunks of two tiles against the restatement"))
    _same(got, by_hand, ("tiles", dtype.__name__, "chunks of two tiles"))
    assert cas.last_call(c.H)[0] == K
    monkeypatch.delenv("ACG_CASCADE_CHUNK")
    got, _ = _guarded(A, cas, c.H, y, S.SNR)
    assert "chunk=%d " % F in cas.describe(c.H)
    _same(got, r.out, ("tiles", dtype.__name__, "one chunk of ten tiles against the restatement"))
    _same(got, by_hand, ("tiles", dtype.__name__, "one chunk of ten tiles"))
    assert cas.last_call(c.H)[0] == K


# ------------------------------------------------------------------------------------------------------ 2. odd chunk
def test_odd_chunk_and_odd_flag_addresses(A, cas, monkeypatch):
    """2051 frames in chunks of 1025: a tile of one frame, and chunks whose ok / iters / stage begin at an odd frame; then the
    caller's ok and stage themselves at an odd byte.  First to reach: the select kernel's byte loads at an odd address."""
    c = S.code(A)
    fail, y, r = S.restated(A, "odd")
    assert len(fail) == 2051 and (r.ok0 == ~fail).all() and (c.n * 8) % 16 != 0
    by_hand, K = _compose(A, cas, c.H, y, S.SNR)
    _same(by_hand, r.out, ("odd", "the two handles by hand against the restatement"))
    monkeypatch.setenv("ACG_CASCADE_CHUNK", "1025")
    for head in (HEAD, HEAD + 1):
        got, ptr = _guarded(A, cas, c.H, y, S.SNR, head_flags=head)
        assert "chunk=1025 " in cas.describe(c.H)
        assert ptr["ok"] % 2 == ptr["stage"] % 2 == head % 2, "torch allocations are at least 2-byte aligned"
        assert (ptr["ok"] + (1025 if head == HEAD else 0)) % 2 == 1
        _same(got, r.out, ("odd", "flags at +%d" % head, "against the restatement"))
        _same(got, by_hand, ("odd", "flags at +%d" % head))
        assert cas.last_call(c.H)[0] == K == int(fail.sum())


# ------------------------------------------------------------------------------------- 3. aligned rows, unaligned base
@pytest.mark.parametrize("dtype,elem", [(np.float64, 8), (np.float32, 4)])
def test_unaligned_base_alone_selects_the_element_gather(A, cas, dtype, elem):
    """H05, n = 280: rows of 16-byte multiples.  y_dev one element into its allocation takes the uint64_t / uint32_t gather,
    the unshifted pointer uint4; both must give the composition."""
    c = Q.case(A, "H05")
    fail, first = S.base_mask()
    y = S.symbols(A, c, fail, first, dtype)
    F = len(fail)
    assert F > S.TILE and (c.n * elem) % 16 == 0
    want, K = _compose(A, cas, c.H, y, S.SNR)
    print("H05 %s: K = %d of %d frames, %d masked" % (dtype.__name__, K, F, int(fail.sum())))
    assert K == int(fail.sum()) and 0 < K < F
    got, ptr = _guarded(A, cas, c.H, y, S.SNR, y_shift=1)
    assert ptr["y"] % 16 == elem, "the shifted pointer must keep the gather off uint4"
    _same(got, want, ("H05", dtype.__name__, "y_dev shifted by one element"))
    assert cas.last_call(c.H)[0] == K
    got, ptr = _guarded(A, cas, c.H, y, S.SNR)
    assert ptr["y"] % 16 == 0
    _same(got, want, ("H05", dtype.__name__, "y_dev aligned"))


# --------------------------------------------------------------------------------------------- 4. the cap and across it
def test_chunk_cap_and_one_frame_beyond(A, cas):
    """65537 float32 frames with the default chunk: 65536 + 1.  64 tiles in one select; about 13 000 failed rows for 8192
    gathering wavefronts, so the row loop strides.  First to reach: the gather's stride."""
    c = S.code(A)
    fail, first = S.cap_mask()
    F = len(fail)
    assert F == (1 << 16) + 1 and fail[-1] and int(fail[:1 << 16].sum()) > 8192 and (c.n * 4) % 16 != 0
    y = S.symbols(A, c, fail, first, np.float32)
    want, K = _compose(A, cas, c.H, y, S.SNR)
    assert K == int(fail.sum()) and (want[3] == np.where(fail, 2, 1)).all()
    repaired = want[0][(want[3] == 2) & (want[1] == 1)]
    assert (repaired[1:] != repaired[:-1]).any(axis=1).all()      # a row gathered or scattered one place off is another word
    got, _ = _guarded(A, cas, c.H, y, S.SNR)
    assert "chunk=65536 " in cas.describe(c.H)
    _same(got, want, "65537 frames")
    assert cas.last_call(c.H)[0] == K


# ------------------------------------------------------------------------------------------------- 5. int16 gather
def test_posterior_rows_of_558_bytes(A):
    """a one-iteration fixed-point first stage and OSD-0: the failed frames' int16 posterior rows, 558 bytes each, are what
    the gather moves.  First to reach: the uint16_t gather."""
    from test_osd_cascade_gpu import _by_hand
    c = S.code(A)
    fail, first = S.q_mask()
    y = S.symbols(A, c, fail, first)
    assert len(fail) > S.TILE and (c.n * 2) % 16 != 0
    cas = A.CascadeDecoder(A.QuantizedMinSumDecoder(1, quant=A.QuantConfig(*Q.QUANTS["default"])), A.OSDDecoder(0))
    try:
        want, K = _by_hand(A, cas, c.H, y, S.SNR)
        assert (want[3] == np.where(fail, 2, 1)).all(), "stage 0 does not fail exactly the masked frames: another seed"
        assert K == int(fail.sum()) and (want[1] == 1).all()
        got, _ = _guarded(A, cas, c.H, y, S.SNR)
        _same(got, want, "QMS-1 -> OSD-0")
        assert cas.last_call(c.H)[0] == K
        assert cas.describe(c.H).endswith(" handover=posteriors")
    finally:
        cas.close()


# ------------------------------------------------------------------------------------------- 6. scatter stride loop
def test_scatter_strides_on_the_5000_x_10000_code(A):
    """the chunk cap of this code is 3355 float64 frames (256 MiB of symbols) and a row has 313 words + 1 slot: 1 053 470
    (row, slot) pairs for 4096 x 256 threads.  Stage 0 runs no iteration, so every frame is handed over and the expectation
    is stage 1 alone.  No generator of this code is at hand: the all-zero word is sent, half the frames clean, so the flags vary
    by row and the words are told from their sentinels only.  First to reach: the scatter's stride."""
    Hm = A.regular_ldpc(5000, 10000, 3, 6, seed=1)
    H = A.ParityCheckMatrix(Hm)
    F, nw, snr = 3355, 313, 2.0
    assert F == (256 << 20) // (10000 * 8) and F * (nw + 1) > 4096 * 256
    rng = np.random.default_rng(20266)
    y = np.ones((F, 10000))
    noisy = S.bernoulli(F, 0.5, 20267)
    y[noisy] += np.sqrt(10.0 ** (-snr / 10.0) / 2.0) * rng.standard_normal((int(noisy.sum()), 10000))
    cas = A.CascadeDecoder(_minsum(A, 0), _minsum(A, 1))
    try:
        alone = _stage_alone(A, cas, H, 1, y, snr)
        assert (alone[1] == ~noisy).all() and (alone[2] == 1).all()
        got, _ = _guarded(A, cas, H, y, snr)
        assert "chunk=%d " % F in cas.describe(H)
        _same(got, alone + (np.full(F, 2, dtype=np.uint8),), "5000 x 10000, K = F")
        assert cas.last_call(H)[0] == F
    finally:
        cas.close()


# -------------------------------------------------------------------------------------------------- 7. Monte-Carlo
def test_mc_run_with_tiles(A, monkeypatch):
    """acg_ldpc_cascade_mc_run on 3000 device-noise frames: one chunk of three tiles, chunks of 1000 and of 1500 (two tiles).
    The failure pattern is the noise's own, so stage 0 runs two iterations, which pass some frames at -2 dB."""
    import torch
    from acg_alp_ldpc_amd._lib import check
    c = S.code(A)
    F, seed, first_frame = 3000, 11, (1 << 33) + 5
    cas = A.CascadeDecoder(_minsum(A, 2), _minsum(A, S.ITERS[1]))
    try:
        run = lambda: A.run_experiment_cascade(cas, c.cws, c.H, S.SNR, frames=F, first_frame=first_frame, noise="device", seed=seed)
        key = lambda r: (_counters(r[0]), _counters(r[1]), {k: v for k, v in r[2].items() if k != "second_kernel_ms"})
        whole = run()
        assert "chunk=%d " % F in cas.describe(c.H)
        for chunk in ("1000", "1500"):
            monkeypatch.setenv("ACG_CASCADE_CHUNK", chunk)
            assert key(run()) == key(whole), chunk
            assert "chunk=%s " % chunk in cas.describe(c.H)
        monkeypatch.delenv("ACG_CASCADE_CHUNK")
        # the classification of the device decode on acg_ldpc_awgn_dev's symbols
        yd = torch.empty((F, c.n), dtype=torch.float32, device="cuda")
        cfg = mc_cfg(A, c.cws, S.SNR, F, first_frame, seed, "device")
        check(A.lib().acg_ldpc_awgn_dev(cas.stage_handle(c.H, 0), C.byref(cfg), yd.data_ptr(), None))
        torch.cuda.synchronize()
        y = yd.cpu().numpy()
        sent = sent_words(c.cws, c.n, first_frame, F)
        w, ok, it, st = _cascade_dev(A, cas, c.H, y, S.SNR)
        want, _, _ = mc_detail(y, w, ok, it, sent, c.Hm)
        assert _counters(whole[0]) == {f: want[f] for f in SEVEN}
        w0, ok0, it0 = _stage_alone(A, cas, c.H, 0, y, S.SNR)
        want0, _, _ = mc_detail(y, w0, ok0, it0, sent, c.Hm)
        assert _counters(whole[1]) == {f: want0[f] for f in SEVEN}
        K = int((st == 2).sum())
        print("MS-2 -> MS-20, H05m1 at %g dB: %d of %d frames handed over, %d repaired" % (S.SNR, K, F, whole[2]["second_correct"]))
        assert whole[2]["second_frames"] == K == int((ok0 == 0).sum()) and 0 < K < F
        assert whole[2]["second_sum_iters"] == int(it[st == 2].sum())
        # the restatement on a sample: both outcomes at stage 0, and they are the device's
        sample = np.arange(256) * (F // 256)
        _layered_kernel(cas, c.H)
        b, rok, rit = layered_minsum(c.Hm, c.layers, y[sample], S.SNR, 2, S.SCALE, symbols_f32=True)
        assert 0 < rok.sum() < len(sample)
        _same((w0[sample], ok0[sample], it0[sample], None), (pack_bits(b), rok, rit, None), "stage 0 on a sample against the restatement")
    finally:
        cas.close()
