"""GPU: the posterior hand-over of a cascade whose first stage is a quantized handle and whose second is OSD.  A frame the first
stage fails gets what OSD's integer entrance returns for the int16 posteriors of the first stage's integer entrance.  Every
frame's word, flag, iters and stage are compared with (a) that composition by hand through public calls and (b) the composition
of the two numpy restatements (layered_q_io_ref.decode_int -> osd_ref.osd); nothing tolerated.  Every other pairing keeps the
symbol hand-over."""
import numpy as np
import pytest

import layered_q_cases as Q
import osd_ref as R
from layered_q_io_ref import decode_int
from layered_q_ref import DEFAULT, quantize
from mc_detail_ref import mc_detail, pack_bits, unpack_bits
from test_cascade_gpu import SEVEN, _cascade_dev, _compose, _counters, _same, _symbols

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


def _by_hand(A, cas, H, y, snr):
    """quantize_dev -> decode_batch_q_dev with posteriors -> OSD integer entrance on the numpy-compacted failed rows -> merge,
    through the cascade's borrowed stage handles -> (words, ok, iters, stage), K"""
    import torch
    from acg_alp_ldpc_amd._lib import check
    L = A.lib()
    h0, h1 = cas.stage_handle(H, 0), cas.stage_handle(H, 1)
    F, n = y.shape
    nw = (n + 31) // 32
    yd = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    c = torch.zeros((F, n), dtype=torch.int16, device="cuda")
    post = torch.zeros((F, n), dtype=torch.int16, device="cuda")
    bits = torch.zeros((F, nw), dtype=torch.int32, device="cuda")
    ok = torch.zeros(F, dtype=torch.uint8, device="cuda")
    it = torch.zeros(F, dtype=torch.int32, device="cuda")
    check(L.acg_ldpc_quantize_dev(h0, yd.data_ptr(), 1 if y.dtype == np.float64 else 0, F * n, float(snr), c.data_ptr(), None))
    check(L.acg_ldpc_decode_batch_q_dev(h0, c.data_ptr(), F, bits.data_ptr(), ok.data_ptr(), it.data_ptr(), post.data_ptr(), None))
    check(L.acg_ldpc_decoder_sync(h0))
    w, ok, it, post = bits.cpu().numpy().view(np.uint32).copy(), ok.cpu().numpy().copy(), it.cpu().numpy().copy(), post.cpu().numpy()
    stage = np.ones(F, dtype=np.uint8)
    fail = np.flatnonzero(ok == 0)
    if len(fail):
        K = len(fail)
        sd = torch.from_numpy(np.ascontiguousarray(post[fail])).cuda()
        b2 = torch.zeros((K, nw), dtype=torch.int32, device="cuda")
        ok2 = torch.zeros(K, dtype=torch.uint8, device="cuda")
        it2 = torch.zeros(K, dtype=torch.int32, device="cuda")
        check(L.acg_ldpc_osd_decode_batch_dev(h1, sd.data_ptr(), K, b2.data_ptr(), ok2.data_ptr(), it2.data_ptr(), None))
        check(L.acg_ldpc_decoder_sync(h1))
        w[fail], ok[fail], it[fail], stage[fail] = b2.cpu().numpy().view(np.uint32), ok2.cpu().numpy(), it2.cpu().numpy(), 2
    return (w, ok, it, stage), len(fail)


def _restated(c, y, snr, iters, order):
    """the two restatements composed -> (packed words, ok, iters, stage)"""
    ch = quantize(y, snr, DEFAULT, symbols_f32=y.dtype == np.float32)
    bits, ok, it, st = R.cascade(decode_int(c.Hm, c.layers, ch, iters, DEFAULT), c.Hm, order)
    return pack_bits(bits), ok, it, st


@pytest.mark.parametrize("case,snr", [("H05", -2.0), ("H", None)])
def test_posteriors_are_handed_over(A, case, snr, monkeypatch):
    c, snr, y64 = _symbols(A, case, snr)
    cas = A.CascadeDecoder(A.QuantizedMinSumDecoder(5), A.OSDDecoder(1))
    try:
        assert cas.name() == "QMS+OSD"
        for y in (y64, y64.astype(np.float32)):
            want, K = _by_hand(A, cas, c.H, y, snr)
            print("%s %s: K = %d of %d frames, %d of them with iters = 1" % (case, y.dtype, K, len(y), int(want[2][want[3] == 2].sum())))
            assert 0 < K < len(y)
            ref = _restated(c, y, snr, 5, 1)
            _same(want, ref, (case, y.dtype, "by hand against the restatements"))
            _same(_cascade_dev(A, cas, c.H, y, snr), want, (case, y.dtype))
            assert cas.last_call(c.H)[0] == K
            _same(_cascade_dev(A, cas, c.H, y, snr, want_iters=False, want_stage=False), want, (case, y.dtype, "iters and stage NULL"))
            # the host entry takes the same route
            bits, hok, hit, hst = cas.decode_batch(c.H, y, snr)
            assert (bits == unpack_bits(want[0], c.n)).all() and (hok == want[1]).all() and (hit == want[2]).all() and (hst == want[3]).all()
            assert cas.last_call(c.H)[0] == K
        d = cas.describe(c.H)
        assert d.endswith(" handover=posteriors") and "last_second_frames=%d" % K in d
        # the hand-over is the posteriors, not the symbols: OSD on the failed frames' symbols gives other words
        sym = R.osd(c.Hm, R.soft_values(y64[want[3] == 2]), 1)[0]
        assert (sym != unpack_bits(want[0][want[3] == 2], c.n)).any()
        # chunks: full ones, a last one of 99 frames, of one frame
        monkeypatch.setenv("ACG_CASCADE_CHUNK", "100")
        whole, _ = _by_hand(A, cas, c.H, y64, snr)
        for F in (len(y64), len(y64) - 1, len(y64) - 99):
            _same(_cascade_dev(A, cas, c.H, y64[:F], snr), tuple(x[:F] for x in whole), (case, "chunks of 100", F))
            assert "chunk=100 " in cas.describe(c.H)
        bits, hok, hit, hst = cas.decode_batch(c.H, y64[:250], snr)
        assert (bits == unpack_bits(whole[0][:250], c.n)).all() and (hst == whole[3][:250]).all() and (hit == whole[2][:250]).all()
    finally:
        cas.close()


def test_no_frame_and_every_frame_handed_over(A):
    c, snr, y = _symbols(A, "H05", 6.0)
    cas = A.CascadeDecoder(A.QuantizedMinSumDecoder(15), A.OSDDecoder(1))
    try:
        want, K = _by_hand(A, cas, c.H, y, snr)
        assert K == 0
        _same(_cascade_dev(A, cas, c.H, y, snr), want, "K = 0")
        assert cas.last_call(c.H)[0] == 0
        assert len(_cascade_dev(A, cas, c.H, y[:0], snr)[1]) == 0
    finally:
        cas.close()
    c, snr, y = _symbols(A, "H05", -2.0)
    cas = A.CascadeDecoder(A.QuantizedMinSumDecoder(0), A.OSDDecoder(1))
    try:
        want, K = _by_hand(A, cas, c.H, y, snr)
        assert K == len(y) and (want[3] == 2).all() and (want[1] == 1).all()
        _same(want, _restated(c, y, snr, 0, 1), "K = F, by hand against the restatements")
        _same(_cascade_dev(A, cas, c.H, y, snr), want, "K = F")
        assert cas.last_call(c.H)[0] == len(y)
        for f in (0, 7):
            _same(_cascade_dev(A, cas, c.H, y[f:f + 1], snr), tuple(x[f:f + 1] for x in want), ("one frame", f))
    finally:
        cas.close()


def test_other_pairings_hand_over_symbols(A):
    c, snr, y = _symbols(A, "H05", -2.0)
    for first, second, name in ((lambda: A.BeliefPropagationDecoder(10), lambda: A.OSDDecoder(1), "BP+OSD"),
                                (lambda: A.OSDDecoder(0), lambda: A.BeliefPropagationDecoder(10), "OSD+BP"),
                                (lambda: A.MinSumDecoder(10, 0.75), lambda: A.BeliefPropagationDecoder(50), "MS+BP")):
        cas = A.CascadeDecoder(first(), second())
        try:
            assert cas.name() == name
            want, K = _compose(A, cas, c.H, y, snr)       # stage 0 alone, stage 1 alone on the failed rows' SYMBOLS
            assert (0 < K < len(y)) == (name != "OSD+BP")
            _same(_cascade_dev(A, cas, c.H, y, snr), want, name)
            assert cas.describe(c.H).endswith(" handover=symbols")
            bits, hok, hit, hst = cas.decode_batch(c.H, y, snr)
            assert (bits == unpack_bits(want[0], c.n)).all() and (hok == want[1]).all() and (hit == want[2]).all() and (hst == want[3]).all()
            if name == "BP+OSD":
                sym = R.osd(c.Hm, R.soft_values(y[want[3] == 2]), 1)
                assert (unpack_bits(want[0][want[3] == 2], c.n) == sym[0]).all() and (want[2][want[3] == 2] == sym[1]).all()
        finally:
            cas.close()


def test_mc_counters(A, monkeypatch):
    c, snr, y = _symbols(A, "H05", -2.0)
    F = len(y)
    cas = A.CascadeDecoder(A.QuantizedMinSumDecoder(5), A.OSDDecoder(1))
    try:
        w, ok, it, st = _restated(c, y, snr, 5, 1)
        want, _, _ = mc_detail(y, w, ok, it, c.cws, c.Hm)
        ch = quantize(y, snr, DEFAULT)
        b0, ok0, it0, _ = decode_int(c.Hm, c.layers, ch, 5, DEFAULT)
        want0, _, _ = mc_detail(y, pack_bits(b0), ok0, it0, c.cws, c.Hm)
        for chunk in (None, "150"):
            if chunk:
                monkeypatch.setenv("ACG_CASCADE_CHUNK", chunk)
            total, first, ex = A.run_experiment_cascade(cas, c.cws, c.H, snr, noise="host")
            assert _counters(total) == {f: want[f] for f in SEVEN} and _counters(first) == {f: want0[f] for f in SEVEN}
            assert total.correct == first.correct + ex["second_correct"] and total.correct >= first.correct
            assert total.pseudo == first.pseudo + ex["second_pseudo"]
            assert ex["second_frames"] == int((st == 2).sum()) == ex["second_correct"] + ex["second_pseudo"]
            assert ex["second_sum_iters"] == int(it[st == 2].sum())
            print("QMS-5 -> OSD-1, H05 at %g dB, %d frames: %d handed over, %d repaired, %d pseudo" % (snr, F, ex["second_frames"], ex["second_correct"], ex["second_pseudo"]))
        # device noise: shards merge to the whole
        monkeypatch.delenv("ACG_CASCADE_CHUNK")
        key = lambda r: (_counters(r[0]), _counters(r[1]), {k: v for k, v in r[2].items() if k != "second_kernel_ms"})
        whole = A.run_experiment_cascade(cas, c.cws, c.H, snr, frames=F, first_frame=500, noise="device", seed=3)
        a = A.run_experiment_cascade(cas, c.cws, c.H, snr, frames=130, first_frame=500, noise="device", seed=3)
        b = A.run_experiment_cascade(cas, c.cws, c.H, snr, frames=F - 130, first_frame=630, noise="device", seed=3)
        assert key(A.merge_cascade_results(a, b)) == key(whole)
        assert whole[0].correct == whole[1].correct + whole[2]["second_correct"] and whole[0].correct >= whole[1].correct
    finally:
        cas.close()
