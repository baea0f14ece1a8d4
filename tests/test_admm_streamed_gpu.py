"""Streamed QP-ADMM engine (csrc/admm_streamed.hip): per-frame state in HBM, one lane per frame, any code size.

Large codes fall through to it from ENGINE_AUTO where the LDS kernels refuse them; ENGINE_STREAMED forces it on any code,
which lets the small pinned codes compare it with the golden fixtures and the LDS kernels."""
import os

import numpy as np
import pytest

from golden_util import ADMM_ITERS, MATS, SNRS, known, load, unpack

pytestmark = pytest.mark.gpu
DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data")
NO_FIT = "does not fit in LDS"


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


@pytest.fixture(scope="module")
def pcm(A, matrices):
    return {k: A.ParityCheckMatrix(v) for k, v in matrices.items()}


@pytest.fixture(scope="module")
def big(A):
    """BASELINE configs[4]: the (3,6)-regular 5000 x 10000 stress code"""
    Hm = A.regular_ldpc(5000, 10000, 3, 6, seed=1)
    return Hm, A.ParityCheckMatrix(Hm)


def big_frames(A, oracle, Hm, H, snr, count, first_seed):
    G, ok = H.get_orthogonal()
    assert ok
    cws = oracle.gen_codewords(G, 77, count)
    return oracle.transmit_frames(cws, snr, first_seed=first_seed)


def test_large_code_decodes_through_the_default_engine(A, oracle, ref, big):
    Hm, H = big
    ys = {snr: big_frames(A, oracle, Hm, H, snr, 12, 1000 + int(snr)) for snr in (2.0, -0.5)}
    words = {}
    for ee in (True, False):
        dec = A.QPADMMDecoder(1.95, 0.5, 100, 1e-5, early_exit=ee)
        lay = dec.layout(H)
        assert lay["lanes_per_frame"] == 1 and lay["lds_bytes_per_frame"] == 0 and lay["frames_per_block"] == 64, lay
        assert "engine=streamed" in dec.describe(H) and "f64=1" in dec.describe(H)
        for snr, y in ys.items():
            bits, ok, iters = dec.decode_batch(H, y, snr)
            ob, ook, oit = oracle.qpadmm_decode(Hm, y, snr, 1.95, 0.5, 100, 1e-5, threads=8)
            assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all(), (ee, snr)
            if snr == -0.5:
                assert (iters == 100).any(), "the hard SNR must keep some frames to the sweep limit"
            if snr == 2.0:
                assert (iters < 100).any()
            rb, rok, _ = ref.qpadmm_decode(Hm, y[:2], snr, 1.95, 0.5, 100, 1e-5)
            assert (bits[:2] == rb).all() and (ok[:2] == rok).all(), (ee, snr)
            words[snr] = bits
        dec.close()
    f32 = A.QPADMMDecoder(1.95, 0.5, 100, 1e-5, precision=A.PREC_F32)
    assert "f64=0" in f32.describe(H)
    same = 0
    for snr, y in ys.items():
        bits, ok, _ = f32.decode_batch(H, y, snr)
        same += int((bits == words[snr]).all(axis=1).sum())
    f32.close()
    assert same >= 22, same   # (fp32 against fp64; fp32 against its own restatement: tests/test_admm_f32_exact_gpu.py)


@pytest.mark.parametrize("name", MATS)
def test_forced_streamed_golden_and_lds_parity(A, oracle, matrices, pcm, name):
    H = pcm[name]
    for snr in SNRS:
        g = load(name, snr)
        alpha, mu = g["admm_alpha_mu"]
        for it in ADMM_ITERS:
            for tag, eps in (("e0", 0.0), ("e5", 1e-5)):
                dec = A.QPADMMDecoder(alpha, mu, it, eps, engine=A.ENGINE_STREAMED)
                bits, ok, iters = dec.decode_batch(H, g["y"], snr)
                dec.close()
                assert (ok == g["admm%d_%s_ok" % (it, tag)]).all(), (name, snr, it, tag)
                assert (bits == unpack(g["admm%d_%s_bits" % (it, tag)], H.n)).all(), (name, snr, it, tag)
    alpha, mu = load(name, -2.0)["admm_alpha_mu"]
    st = A.QPADMMDecoder(alpha, mu, 100, 1e-5, engine=A.ENGINE_STREAMED)
    lds = A.QPADMMDecoder(alpha, mu, 100, 1e-5)
    lay = st.layout(H)
    assert lay["lanes_per_frame"] == 1 and lay["grid_blocks"] >= 1, lay
    assert lds.layout(H)["lanes_per_frame"] != 1
    G, _ = oracle.get_orthogonal(matrices[name])
    many = lay["grid_blocks"] * 64 + 5          # more tiles than slabs: the tile hand-out loops
    cws = oracle.gen_codewords(G, 4321, many)
    y = oracle.transmit_frames(cws, -2.0, first_seed=5000)
    for F in (3000, 1, 63, 65, many):
        a = st.decode_batch(H, y[:F], -2.0)
        b = lds.decode_batch(H, y[:F], -2.0)
        for u, v in zip(a, b):
            assert (u == v).all(), (name, F)
    st.close()
    lds.close()


@pytest.mark.parametrize("idx", [5, 6, 7, 8, 9, 10, 12])
def test_mc_host_noise_known_answers_streamed(A, matrices, pcm, idx):
    e = known()["experiments"][idx]
    assert e["kind"] == "qpadmm"
    H = pcm[e["matrix"]]
    if e["codewords"].startswith("G05"):
        from oracle.pyoracle import Oracle
        G = Oracle().read_pcm(os.path.join(DATA, "G05.txt"))
    else:
        G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 1000, 239239239)
    dec = A.QPADMMDecoder(e["alpha"], e["mu"], e["max_iter"], 1e-5, engine=A.ENGINE_STREAMED)
    r = A.run_experiment(dec, cws, H, e["snr"], noise="host")
    dec.close()
    for k in ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong"):
        assert getattr(r, k) == e[k], (k, r, e)


def test_mc_device_noise_equals_lds_kernel(A, pcm):
    H = pcm["H05"]
    G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 4096, 239239239)
    runs = []
    for kw in (dict(engine=A.ENGINE_STREAMED), dict()):
        dec = A.QPADMMDecoder(1.95, 0.5, 100, 1e-5, **kw)
        runs.append(A.run_experiment(dec, cws, H, -2.0, frames=20000, noise="device", seed=99))
        dec.close()
    assert runs[0].total == 20000
    assert (runs[0].as_vector() == runs[1].as_vector()).all(), runs


def test_corners_against_the_oracle(A, oracle, matrices, pcm):
    Hm, H = matrices["H05"], pcm["H05"]
    G, _ = oracle.get_orthogonal(Hm)
    cws = oracle.gen_codewords(G, 31, 300)
    y = oracle.transmit_frames(cws, -1.0, first_seed=800)
    cases = [(1.95, 0.5, 0, 1e-5), (1.95, 0.5, 1, 1e-5), (1.95, 0.5, 60, 0.0), (5.0, 0.5, 30, 1e-5)]  # last: guard fires
    for alpha, mu, it, eps in cases:
        ob, ook, oit = oracle.qpadmm_decode(Hm, y, -1.0, alpha, mu, it, eps, threads=8)
        for ee in (True, False):
            dec = A.QPADMMDecoder(alpha, mu, it, eps, engine=A.ENGINE_STREAMED, early_exit=ee)
            bits, ok, iters = dec.decode_batch(H, y, -1.0)
            dec.close()
            assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all(), (alpha, mu, it, eps, ee)
    # the guard in Monte-Carlo runs: every frame fails (experiment.h:109-120), host and device noise
    dec = A.QPADMMDecoder(5.0, 0.5, 30, 1e-5, engine=A.ENGINE_STREAMED)
    cw = np.asarray(A.gen_random_codewords(np.asarray(G), 200, 239239239))
    r = A.run_experiment(dec, cw, H, -1.0, noise="host")
    o = oracle.experiment("qpadmm", Hm, cw, -1.0, 30, 5.0, 0.5, 1e-5)
    for k in ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong"):
        assert getattr(r, k) == o[k], (k, r, o)
    r = A.run_experiment(dec, cw, H, -1.0, frames=5000, noise="device", seed=3)
    dec.close()
    assert (r.correct, r.pseudo, r.total, r.sum_hamming_ok, r.sum_iters) == (0, 0, 5000, 0, 0), r
    assert r.sum_hamming_wrong == r.sum_hamming > 0, r
    # non-finite and extreme symbols (test_edge_graphs_and_extreme_symbols_other_engines)
    yy = oracle.transmit_frames(oracle.gen_codewords(G, 8, 60), 0.0, first_seed=70000)
    yy[0, 3] = np.nan
    yy[1, 10] = np.inf
    yy[2, 17] = -np.inf
    yy[3, :5] = 0.0
    yy[4, 100] = 1e300
    ob, ook, oit = oracle.qpadmm_decode(Hm, yy, 0.0, 1.95, 0.5, 40, 1e-5, threads=4)
    dec = A.QPADMMDecoder(1.95, 0.5, 40, 1e-5, engine=A.ENGINE_STREAMED)
    bits, ok, iters = dec.decode_batch(H, yy, 0.0)
    dec.close()
    assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all()
    # ragged graph: degree-1 and degree-2 checks, a degree-40 check, a degree-20 variable, no isolated variable
    from test_admm_stream_tables import ragged_graph
    R = ragged_graph()
    assert R.sum(axis=1).max() == 40 and R.sum(axis=0).max() == 20 and R.sum(axis=0).min() >= 1
    assert sorted(set(R.sum(axis=1).tolist()))[:2] == [1, 2]
    rng = np.random.default_rng(11)
    yr = 1.0 + 0.8 * rng.standard_normal((150, R.shape[1]))
    ob, ook, oit = oracle.qpadmm_decode(R, yr, 1.0, 0.6, 1.0, 80, 1e-5, threads=4)
    for kw in (dict(engine=A.ENGINE_STREAMED), dict(engine=A.ENGINE_STREAMED, early_exit=False)):
        dec = A.QPADMMDecoder(0.6, 1.0, 80, 1e-5, **kw)
        bits, ok, iters = dec.decode_batch(R, yr, 1.0)
        dec.close()
        assert (ok == ook).all() and (bits == ob).all() and (iters == oit).all(), kw


def test_one_handle_two_streams(A, oracle, matrices, pcm):
    import torch
    H = pcm["H05"]
    G, _ = H.get_orthogonal()
    cws = A.gen_random_codewords(G, 512, 7)
    snr, F = -1.0, 20000
    dec = A.QPADMMDecoder(1.95, 0.5, 100, 1e-5, engine=A.ENGINE_STREAMED)
    nw = (H.n + 31) // 32
    ys = [torch.from_numpy(A.transmit_frames(cws, snr, first_frame=b * F, frames=F)).cuda() for b in range(2)]

    def outs():
        return (torch.full((F, nw), -1, dtype=torch.int32, device="cuda"), torch.full((F,), 7, dtype=torch.uint8, device="cuda"),
                torch.full((F,), -1, dtype=torch.int32, device="cuda"))
    serial = []
    for b in range(2):
        o = outs()
        dec.decode_batch_dev(H, ys[b].data_ptr(), True, F, snr, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr())
        dec.sync(H)
        serial.append([t.cpu().numpy() for t in o])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    par = [outs(), outs()]
    torch.cuda.synchronize()
    for b in range(2):
        o = par[b]
        dec.decode_batch_dev(H, ys[b].data_ptr(), True, F, snr, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(),
                             streams[b].cuda_stream)
    torch.cuda.synchronize()
    for b in range(2):
        for u, v in zip(par[b], serial[b]):
            assert (u.cpu().numpy() == v).all(), b
    assert set(np.unique(serial[0][1]).tolist()) == {1}
    dec.close()


def test_refusals_kept(A, big):
    _, H = big
    for kw, msg in ((dict(engine=A.ENGINE_FUSED), NO_FIT), (dict(lanes_per_frame=64), NO_FIT),
                    (dict(engine=A.ENGINE_STREAMED, lanes_per_frame=64), "lanes_per_frame must be 0")):
        dec = A.QPADMMDecoder(1.95, 0.5, 100, 1e-5, **kw)
        with pytest.raises(A.LdpcError, match=msg):
            dec.handle(H)
        dec.close()
