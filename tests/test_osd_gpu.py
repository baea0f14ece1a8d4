"""GPU: ordered-statistics decoding (algo = ACG_LDPC_OSD, osd.hip) against its numpy restatement tests/osd_ref.py: the word, the
flag and iters of EVERY frame are equal, nothing tolerated.  Codes and frames: tests/layered_q_cases.py (300-400 frames of
host-noise symbols each), the (7,4) Hamming code (m, n < 32) and a rank-deficient H05 of 162 rows.  Then ties, edge frames,
the quantiser, frame counts, untouched output rows, streams, host entries, Monte-Carlo runs and every refusal."""
import ctypes as C
import os

import numpy as np
import pytest

import layered_q_cases as Q
import osd_ref as R
from mc_decode_path import mc_cfg, sent_words
from mc_detail_ref import mc_detail, pack_bits, unpack_bits
from test_cascade_gpu import _decode_dev

pytestmark = pytest.mark.gpu

SEVEN = ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong", "sum_iters")
CASES = ["H", "H05", "ragged", "qc4x24z27", "diag10"]
EXTRA = ["hamming", "H05_rank_deficient"]
HAMMING = np.array([[1, 0, 1, 0, 1, 0, 1],
                    [0, 1, 1, 0, 0, 1, 1],
                    [0, 0, 0, 1, 1, 1, 1]], dtype=np.uint8)


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


class _M:
    """a matrix, its symbols and the restatement's answers for them (both orders on one elimination, computed once)"""
    _made = {}

    def __init__(self, A, name):
        if name in CASES:
            c = Q.case(A, name)
            self.H, self.Hm, self.y, self.cws, self.snr = c.H, c.Hm, c.y, c.cws, c.snr
        else:
            if name == "hamming":
                self.Hm = HAMMING
            else:
                h = Q.case(A, "H05").Hm
                self.Hm = np.concatenate([h, h[:1], h[1:2] ^ h[2:3]]).astype(np.uint8)
                assert self.Hm.shape == (162, 280)
            self.H = A.ParityCheckMatrix(self.Hm)
            self.cws, self.snr = None, 0.0
            rng = np.random.default_rng(3)
            self.y = 1.0 + rng.normal(0, 0.8, (200, self.Hm.shape[1]))
        self.n = self.Hm.shape[1]
        self.s = R.soft_values(self.y)
        self._ref = {}

    def ref(self, s=None, key="symbols"):
        """{order: (words, iters, metric)} for the soft values s (the symbols' own when None)"""
        if key not in self._ref:
            self._ref[key] = R.osd_orders(self.Hm, self.s if s is None else s)
        return self._ref[key]


def M(A, name):
    if name not in _M._made:
        _M._made[name] = _M(A, name)
    return _M._made[name]


def _osd_dev(A, dec, H, s, want_iters=True, stream=None, extra=1):
    """acg_ldpc_osd_decode_batch_dev on host soft values s [F, n] int16 -> words [F, nw], ok, iters or None.  The outputs are
    `extra` rows longer than F and filled with sentinels: rows past F, and iters handed over as NULL, must keep them."""
    import torch
    F, n = s.shape
    nw = (n + 31) // 32
    sd = torch.from_numpy(np.ascontiguousarray(s)).cuda() if F else torch.zeros(8, dtype=torch.int16, device="cuda")
    bits = torch.full((F + extra, nw), -1, dtype=torch.int32, device="cuda")
    ok = torch.full((F + extra,), 7, dtype=torch.uint8, device="cuda")
    it = torch.full((F + extra,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dec.decode_soft_batch_dev(H, sd.data_ptr() if F else None, F, bits.data_ptr(), ok.data_ptr(), it.data_ptr() if want_iters else None, stream)
    torch.cuda.synchronize()
    assert (bits[F:] == -1).all() and (ok[F:] == 7).all() and (it[F:] == -7).all(), "a row past the batch was written"
    if not want_iters:
        assert (it == -7).all()
    return bits.cpu().numpy().view(np.uint32)[:F], ok.cpu().numpy()[:F], it.cpu().numpy()[:F] if want_iters else None


def _same(got, want, n, ctx):
    """got = (packed words, ok, iters or None) of the device, want = (words [F, n], iters, ...) of the restatement"""
    w, ok, it = got
    bad = (unpack_bits(w, n) != want[0]).any(axis=1) | (ok != 1)
    if it is not None:
        bad |= it != want[1]
    if bad.any():
        f = int(np.flatnonzero(bad)[0])
        pytest.fail("%s: %d of %d frames differ; first: frame %d, device ok %d iters %s, restatement iters %d, %d bits differ"
                    % (ctx, int(bad.sum()), len(bad), f, ok[f], None if it is None else it[f], want[1][f],
                       int((unpack_bits(w[f:f + 1], n)[0] != want[0][f]).sum())))
    pad = n % 32
    if pad:
        assert not (w[:, -1] >> np.uint32(pad)).any(), "bits past n are set in the last word"


# ------------------------------------------------------------------------- 1. every frame equals the restatement
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", CASES + EXTRA)
def test_every_frame_equals_the_restatement(A, name, order):
    m = M(A, name)
    want = m.ref()[order]
    if order == 1 and name != "diag10":   # (disjoint single-parity checks: order 0 is already maximum-likelihood)
        assert 0 < want[1].sum(), "order 1 never improves on order 0 for these frames"
    for L in (0, 64, 128, 256):
        dec = A.OSDDecoder(order, lanes_per_frame=L)
        try:
            h, _ = dec.handle(m.H)
            assert dec.name() == "OSD" == A.lib().acg_ldpc_decoder_name(h).decode()
            # integer entrance, then the symbol entrance with double and float symbols
            _same(_osd_dev(A, dec, m.H, m.s), want, m.n, (name, order, L, "soft values"))
            for y in (m.y, m.y.astype(np.float32)):
                got = _decode_dev(A.lib().acg_ldpc_decode_batch_dev, h, y, 123.0, m.n)[:3]
                _same(got, want, m.n, (name, order, L, "symbols", y.dtype))
            d = dec.describe(m.H)
            lay = dec.layout(m.H)
            auto = 64 if m.n <= 128 else 128 if m.n <= 256 else 256
            assert lay["lanes_per_frame"] == (L or auto) and lay["frames_per_block"] == 1
            assert 0 < lay["lds_bytes_per_frame"] <= 160 * 1024 and "lds_block=%d " % lay["lds_bytes_per_frame"] in d
            rank = 160 if name.startswith("H05") else {"H": 64, "hamming": 3, "diag10": 10}.get(name)
            assert "kernel=osd_kernel" in d and "order=%d " % order in d and "block=%d " % (L or auto) in d and "workgroups_per_cu=" in d
            assert rank is None or "rank=%d " % rank in d
        finally:
            dec.close()


def test_symbol_entrance_of_float_and_double_agree_with_the_quantiser(A):
    m = M(A, "H05")
    y32 = m.y.astype(np.float32)
    assert (A.OSDDecoder.soft_values(m.y) == m.s).all() and (A.OSDDecoder.soft_values(y32) == R.soft_values(y32)).all()
    assert (R.soft_values(y32) == m.s).all()    # a double is rounded to float first: the two entrances see the same values


# ------------------------------------------------------------------------------------ 2. ties and edge frames
@pytest.mark.parametrize("name", ["H05", "hamming", "H05_rank_deficient", "qc4x24z27"])
def test_ties_in_keys_and_metrics(A, name):
    m = M(A, name)
    s = np.random.default_rng(17).integers(-2, 3, (120, m.n)).astype(np.int16)
    want = m.ref(s, "ties")
    for order in (0, 1):
        dec = A.OSDDecoder(order)
        try:
            _same(_osd_dev(A, dec, m.H, s), want[order], m.n, (name, order, "values -2..2"))
        finally:
            dec.close()


def test_edge_frames(A):
    m = M(A, "H05")
    sent = m.cws[:3]
    s = np.concatenate([np.zeros((1, m.n), np.int16), np.full((1, m.n), -32768, np.int16),
                        np.where(sent != 0, -32767, 32767).astype(np.int16)])
    want = m.ref(s, "edges")
    for order in (0, 1):
        assert (want[order][0][2:] == sent).all() and (want[order][1][2:] == 0).all()
        dec = A.OSDDecoder(order)
        try:
            got = _osd_dev(A, dec, m.H, s)
            _same(got, want[order], m.n, ("edge frames", order))
            assert (unpack_bits(got[0], m.n)[2:] == sent).all() and (got[2][2:] == 0).all()
        finally:
            dec.close()


def test_quantiser(A):
    e = np.float64(1) / 4096
    y = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-40, -1e-40, 1e-310, 1e300, -1e300, 3.4e38, 4e38, 7.999755859375, 7.99975586,
                  7.9997558, 8.0, -7.999755859375, -8.0, -7.9997, e, -e, 0.999 * e, 1.5 * e, -1.5 * e, 32766.5 * e, 32767.5 * e, -32767.5 * e])
    y = np.concatenate([y, np.random.default_rng(1).normal(0, 3, 1000), np.random.default_rng(2).normal(0, 1e-3, 200)])
    for arr in (y, y.astype(np.float32)):
        with np.errstate(over="ignore"):
            assert (A.OSDDecoder.soft_values(arr) == R.soft_values(arr)).all(), arr.dtype
    assert R.soft_values(y[:6]).tolist() == [0, 0, 0, 32767, -32767, 0]


# ------------------------------------------------------------------- 3. frame counts, output buffers, streams, host
def test_zero_and_one_frame_and_null_iters(A):
    m = M(A, "H05")
    want = m.ref()[1]
    dec = A.OSDDecoder(1)
    try:
        h, _ = dec.handle(m.H)
        assert len(_osd_dev(A, dec, m.H, m.s[:0])[1]) == 0             # nothing launched: every sentinel survives (checked inside)
        assert len(_decode_dev(A.lib().acg_ldpc_decode_batch_dev, h, m.y[:0], 0.0, m.n)[1]) == 0
        for f in (0, int(np.flatnonzero(want[1] == 1)[0]), int(np.flatnonzero(want[1] == 0)[0])):
            one = tuple(x[f:f + 1] for x in want)
            _same(_osd_dev(A, dec, m.H, m.s[f:f + 1]), one, m.n, ("one frame", f))
            _same(_decode_dev(A.lib().acg_ldpc_decode_batch_dev, h, m.y[f:f + 1], 0.0, m.n)[:3], one, m.n, ("one frame, symbols", f))
        _same(_osd_dev(A, dec, m.H, m.s, want_iters=False, extra=3), want, m.n, "iters NULL")
        _same(_decode_dev(A.lib().acg_ldpc_decode_batch_dev, h, m.y, 0.0, m.n, want_iters=False)[:3], want, m.n, "iters NULL, symbols")
    finally:
        dec.close()


def test_two_launches_on_two_streams(A):
    import torch
    m = M(A, "H05")
    want = m.ref()[1]
    dec = A.OSDDecoder(1)
    try:
        nw = (m.n + 31) // 32
        sd = torch.from_numpy(m.s).cuda()
        half = len(m.s) // 2
        outs = []
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        for k, st in enumerate(streams):
            F = half if k == 0 else len(m.s) - half
            bits = torch.full((F, nw), -1, dtype=torch.int32, device="cuda")
            ok = torch.full((F,), 7, dtype=torch.uint8, device="cuda")
            it = torch.full((F,), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            dec.decode_soft_batch_dev(m.H, sd[k * half:].data_ptr(), F, bits.data_ptr(), ok.data_ptr(), it.data_ptr(), st.cuda_stream)
            outs.append((bits, ok, it))
        torch.cuda.synchronize()
        for k, (bits, ok, it) in enumerate(outs):
            sl = slice(0, half) if k == 0 else slice(half, None)
            _same((bits.cpu().numpy().view(np.uint32), ok.cpu().numpy(), it.cpu().numpy()), tuple(x[sl] for x in want), m.n, ("stream", k))
    finally:
        dec.close()


@pytest.mark.parametrize("name", ["H05", "hamming"])
def test_host_entries_equal_the_device_entries(A, name):
    m = M(A, name)
    for order in (0, 1):
        want = m.ref()[order]
        dec = A.OSDDecoder(order)
        try:
            bits, ok, it = dec.decode_soft_batch(m.H, m.s)
            assert bits.dtype == np.uint8 and (bits == want[0]).all() and (ok == 1).all() and (it == want[1]).all()
            bits, ok, it = dec.decode_soft_batch(m.H, m.s.astype(np.int64))
            assert (bits == want[0]).all() and (it == want[1]).all()
            for y in (m.y, m.y.astype(np.float32)):
                bits, ok, it = dec.decode_batch(m.H, y, -3.0)
                assert (bits == want[0]).all() and (ok == 1).all() and (it == want[1]).all()
            word, good = dec.decode(m.H, m.y[0], 0.0)
            assert good and (word == want[0][0]).all()
            with pytest.raises(TypeError):
                dec.decode_soft_batch(m.H, m.y)
            with pytest.raises(ValueError):
                dec.decode_soft_batch(m.H, np.full((1, m.n), 40000))
            assert len(dec.decode_soft_batch(m.H, m.s[:0])[1]) == 0
        finally:
            dec.close()


# -------------------------------------------------------------------------------------------------- 4. Monte-Carlo
def _counters(r):
    return {f: int(getattr(r, f)) for f in SEVEN}


def test_mc_counters_equal_the_restatements(A, monkeypatch):
    import torch
    from acg_alp_ldpc_amd._lib import check
    m = M(A, "H05")
    F = len(m.y)
    dec = A.OSDDecoder(1)
    try:
        h, _ = dec.handle(m.H)
        # host noise: the case's own symbols
        want = m.ref()[1]
        exp, _, _ = mc_detail(m.y, pack_bits(want[0]), np.ones(F, np.uint8), want[1], m.cws, m.Hm)
        assert 0 < exp["correct"] < F and exp["pseudo"] == F - exp["correct"]      # OSD always returns a codeword
        assert _counters(A.run_experiment(dec, m.cws, m.H, m.snr, noise="host")) == {f: exp[f] for f in SEVEN}
        monkeypatch.setenv("ACG_MC_DETAIL_CHUNK", "150")                           # 400 frames: two full chunks and one of 100
        det = A.run_experiment_detail(dec, m.cws, m.H, m.snr, noise="host", cap=8)
        assert _counters(det) == {f: exp[f] for f in SEVEN}
        assert det.bit_errors == exp["bit_errors"] and det.word_frames == F and det.noncodeword_frames == 0
        assert det.min_pseudo_weight == exp["min_pseudo_weight"] and det.min_pseudo_frame == exp["min_pseudo_frame"]
        # device noise: the symbols of acg_ldpc_awgn_dev through the restatement
        first, seed = 1000, 11
        yd = torch.empty((F, m.n), dtype=torch.float32, device="cuda")
        cfg = mc_cfg(A, m.cws, m.snr, F, first, seed, "device")
        check(A.lib().acg_ldpc_awgn_dev(h, C.byref(cfg), yd.data_ptr(), None))
        torch.cuda.synchronize()
        y = yd.cpu().numpy()
        w, it, _ = R.osd(m.Hm, R.soft_values(y), 1)
        sent = sent_words(m.cws, m.n, first, F)
        exp, _, _ = mc_detail(y, pack_bits(w), np.ones(F, np.uint8), it, sent, m.Hm, first_frame=first)
        got = A.run_experiment(dec, m.cws, m.H, m.snr, frames=F, first_frame=first, noise="device", seed=seed)
        assert _counters(got) == {f: exp[f] for f in SEVEN}
        det = A.run_experiment_detail(dec, m.cws, m.H, m.snr, frames=F, first_frame=first, noise="device", seed=seed, cap=4)
        assert _counters(det) == {f: exp[f] for f in SEVEN} and det.bit_errors == exp["bit_errors"]
        assert det.min_pseudo_weight == exp["min_pseudo_weight"] and det.min_pseudo_frame == exp["min_pseudo_frame"]
    finally:
        dec.close()


# ------------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals(A):
    import torch
    from acg_alp_ldpc_amd import _lib
    L = A.lib()
    m = M(A, "H05")
    err = lambda: L.acg_ldpc_last_error().decode()

    def refused(H, match, **kw):
        order = kw.pop("order", 1)
        dec = A.OSDDecoder(order, **kw)
        try:
            with pytest.raises(A.LdpcError, match=match):
                dec.handle(H)
        finally:
            dec.close()
    refused(m.H, "OSD: max_iter is the order and must be 0 or 1", order=2)
    refused(m.H, "max_iter", order=-1)
    for prec in (A.PREC_F64, A.PREC_F32, A.PREC_F16):
        refused(m.H, "OSD: precision must be", precision=prec)
    refused(m.H, "OSD: engine must be", engine=A.ENGINE_STREAMED)
    refused(m.H, "OSD: schedule must be", schedule=A.SCHEDULE_LAYERED)
    for lanes in (32, 100, 512, 1024, -64):
        refused(m.H, "OSD: lanes_per_frame must be 0, 64, 128 or 256", lanes_per_frame=lanes)
    refused(Q.case(A, "qc2x10z300").H, "OSD: a frame .* does not fit in LDS")
    wide = np.zeros((1, 65536), dtype=np.uint8)
    wide[0, :3] = 1
    refused(A.ParityCheckMatrix(wide), "OSD: n must be <= 65535")
    # ignored parameters are ignored
    osd = A.OSDDecoder(1, early_exit=False)
    bp = A.BeliefPropagationDecoder(5)
    qms = A.QuantizedMinSumDecoder(3)
    try:
        assert (osd.decode_soft_batch(m.H, m.s[:50])[0] == m.ref()[1][0][:50]).all()
        h, hb, hq = osd.handle(m.H)[0], bp.handle(m.H)[0], qms.handle(m.H)[0]
        nw = (m.n + 31) // 32
        sd = torch.from_numpy(m.s[:4]).cuda()
        bits = torch.full((4, nw), -1, dtype=torch.int32, device="cuda")
        ok = torch.full((4,), 7, dtype=torch.uint8, device="cuda")
        # the integer entrance: wrong handles, null and negative arguments; zero frames is a no-op
        for wrong in (hb, hq):
            assert L.acg_ldpc_osd_decode_batch_dev(wrong, sd.data_ptr(), 4, bits.data_ptr(), ok.data_ptr(), None, None) != 0
            assert "ACG_LDPC_OSD" in err()
        assert L.acg_ldpc_osd_decode_batch_dev(None, sd.data_ptr(), 4, bits.data_ptr(), ok.data_ptr(), None, None) != 0 and "null decoder" in err()
        assert L.acg_ldpc_osd_decode_batch_dev(h, sd.data_ptr(), -1, bits.data_ptr(), ok.data_ptr(), None, None) != 0
        assert L.acg_ldpc_osd_decode_batch_dev(h, None, 4, bits.data_ptr(), ok.data_ptr(), None, None) != 0
        assert L.acg_ldpc_osd_decode_batch_dev(h, None, 0, None, None, None, None) == 0
        hbits, hok = np.zeros((4, m.n), np.uint8), np.zeros(4, np.uint8)
        s4 = np.ascontiguousarray(m.s[:4])
        assert L.acg_ldpc_osd_decode_batch(hb, s4.ctypes.data, 4, hbits.ctypes.data, hok.ctypes.data, None) != 0 and "ACG_LDPC_OSD" in err()
        assert L.acg_ldpc_osd_decode_batch(h, None, 4, hbits.ctypes.data, hok.ctypes.data, None) != 0
        assert L.acg_ldpc_osd_decode_batch(h, s4.ctypes.data, 4, None, hok.ctypes.data, None) != 0
        assert L.acg_ldpc_osd_decode_batch(h, s4.ctypes.data, 4, hbits.ctypes.data, None, None) != 0
        assert L.acg_ldpc_osd_decode_batch(h, s4.ctypes.data, -2, hbits.ctypes.data, hok.ctypes.data, None) != 0
        assert L.acg_ldpc_osd_decode_batch(h, None, 0, None, None, None) == 0
        # an OSD handle is not a quantized one, and no grid takes it
        assert L.acg_ldpc_decode_batch_q_dev(h, sd.data_ptr(), 4, bits.data_ptr(), ok.data_ptr(), None, None, None) != 0
        assert L.acg_ldpc_quantize_dev(h, sd.data_ptr(), 0, 4, 0.0, sd.data_ptr(), None) != 0
        torch.cuda.synchronize()
        assert (bits == -1).all() and (ok == 7).all()
        cfg = mc_cfg(A, m.cws, m.snr, 64, 0, 1, "device")
        res = (_lib.McResult * 2)()
        al = (C.c_double * 2)(1.2, 1.2)
        assert L.acg_ldpc_mc_run_grid(h, C.byref(cfg), al, al, 2, res) != 0 and "QP-ADMM" in err()
        q = (_lib.Quant * 1)(A.QuantConfig().as_struct())
        assert L.acg_ldpc_mc_run_quants(h, C.byref(cfg), q, 1, res) != 0 and "quantized" in err()
        out = np.zeros(4, np.int16)
        assert L.acg_ldpc_debug_osd_soft(None, 1, 4, out.ctypes.data) != 0
        assert L.acg_ldpc_debug_osd_soft(m.y.ctypes.data, 1, -1, out.ctypes.data) != 0
        assert L.acg_ldpc_debug_osd_soft(m.y.ctypes.data, 1, 0, out.ctypes.data) == 0
    finally:
        osd.close()
        bp.close()
        qms.close()
