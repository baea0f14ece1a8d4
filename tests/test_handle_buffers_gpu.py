"""Buffers of one decoder handle that are re-grown and re-used (csrc/device_mem.hpp: DeviceBuf / PinnedBuf owners).

A handle keeps its staging, symbol, codeword, counter and table buffers between calls and only ever grows them.  Every
test here runs a sequence of calls of different sizes on ONE handle and requires each result to equal, field for field, what
a handle created for that call alone gives.  H05 (n = 280) and an n = 75 code whose last symbol quad is ragged; fp32, and
fp64 once per test.  The last test covers a create that is refused after its tables were uploaded, and a destroy right
behind an asynchronous launch on a caller stream."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT_FIELDS = ("correct", "pseudo", "total", "sum_hamming", "sum_hamming_ok", "sum_hamming_wrong", "sum_iters")
SNR = {"H05": -2.0, "n75": 1.0}


def ints(r):
    return tuple(getattr(r, f) for f in INT_FIELDS)


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


@pytest.fixture(scope="module")
def codes(A, matrices):
    """name -> (ParityCheckMatrix, two different sets of 37 codewords)"""
    out = {}
    for name, Hm in (("H05", matrices["H05"]), ("n75", A.regular_ldpc(45, 75, 3, 5, seed=1))):
        H = A.ParityCheckMatrix(Hm)
        G, _ = H.get_orthogonal()
        a = np.ascontiguousarray(A.gen_random_codewords(G, 37, 11), dtype=np.uint8)
        b = np.ascontiguousarray(A.gen_random_codewords(G, 37, 12), dtype=np.uint8)
        assert a.any() and b.any() and (a != b).any()
        out[name] = (H, a, b)
    return out


def on_one_handle_and_fresh(make, call, steps):
    """call(decoder, step) for every step on one decoder, and each on a decoder of its own"""
    dec = make()
    got = [call(dec, s) for s in steps]
    dec.close()
    want = []
    for s in steps:
        fresh = make()
        want.append(call(fresh, s))
        fresh.close()
    return got, want


@pytest.mark.parametrize("code", ["H05", "n75"])
@pytest.mark.parametrize("kind", ["bp-f32", "bp-f64", "admm-f32"])
def test_host_decode_1_300_1_frames(A, codes, kind, code):
    """acg_ldpc_decode_batch / _f32: the pinned and device staging sets grow for 300 frames and are kept for the single
    frames behind them; then the same with float symbols (another element size in the same buffers)"""
    H, cws, _ = codes[code]
    make = {"bp-f32": lambda: A.BeliefPropagationDecoder(30), "bp-f64": lambda: A.BeliefPropagationDecoder(30, precision=A.PREC_F64),
            "admm-f32": lambda: A.QPADMMDecoder(1.95, 0.5, 60, 1e-5, precision=A.PREC_F32)}[kind]
    y = A.transmit_frames(cws[np.arange(300) % len(cws)], SNR[code])
    steps = [(1, np.float64), (300, np.float64), (1, np.float64), (300, np.float32), (1, np.float32)]

    def call(dec, step):
        frames, dt = step
        return dec.decode_batch(H, np.ascontiguousarray(y[:frames], dtype=dt), SNR[code])

    got, want = on_one_handle_and_fresh(make, call, steps)
    for s, g, w in zip(steps, got, want):
        for u, v in zip(g, w):
            assert u.shape == v.shape and (u == v).all(), s
    assert got[1][1].any()  # (ok flags: the decodes are not all failures)


def unfused_routes(A):
    """Monte-Carlo routes AWGN kernel -> decode -> classify kernel: the symbols and the decode outputs sit in handle buffers.
    The paired-frame F16 min-sum decoder accepts check degree <= 8 and variable degree <= 4: the n = 75 code, not H05, whose
    F16 route is the layered F16 min-sum decoder with ACG_LAY_UNFUSED_MC (set by the tests below)."""
    return {"streamed-bp-f32": lambda: A.BeliefPropagationDecoder(30, engine=A.ENGINE_STREAMED),
            "streamed-bp-f64": lambda: A.BeliefPropagationDecoder(30, engine=A.ENGINE_STREAMED, precision=A.PREC_F64),
            "minsum-f16": lambda: A.MinSumDecoder(30, 0.75, precision=A.PREC_F16),
            "layered-f16": lambda: A.MinSumDecoder(20, 0.75, schedule=A.SCHEDULE_LAYERED, precision=A.PREC_F16)}


UNFUSED = [("streamed-bp-f32", "H05"), ("streamed-bp-f32", "n75"), ("streamed-bp-f64", "H05"), ("streamed-bp-f64", "n75"),
           ("minsum-f16", "n75"), ("layered-f16", "H05"), ("layered-f16", "n75")]


@pytest.mark.parametrize("route,code", UNFUSED)
def test_device_noise_monte_carlo_256_1024_256_frames(A, codes, monkeypatch, route, code):
    monkeypatch.setenv("ACG_LAY_UNFUSED_MC", "1")
    H, cws, _ = codes[code]

    def call(dec, frames):
        return ints(A.run_experiment(dec, cws, H, SNR[code], frames=frames, first_frame=3, noise="device", seed=7))

    got, want = on_one_handle_and_fresh(unfused_routes(A)[route], call, [256, 1024, 256])
    assert got == want
    assert [g[2] for g in got] == [256, 1024, 256] and got[1][0] > 0


@pytest.mark.parametrize("route,code", [("fused-bp-f32", "H05"), ("fused-bp-f32", "n75"), ("fused-bp-f64", "H05"), ("fused-bp-f64", "n75"),
                                        ("streamed-bp-f32", "H05"), ("streamed-bp-f32", "n75"), ("minsum-f16", "n75"), ("layered-f16", "H05")])
def test_codeword_set_replaced_and_restored(A, codes, monkeypatch, route, code):
    """two different codeword sets of the same count, then the first again: the device copy is keyed on the content"""
    monkeypatch.setenv("ACG_LAY_UNFUSED_MC", "1")
    H, cws_a, cws_b = codes[code]
    make = dict(unfused_routes(A), **{"fused-bp-f32": lambda: A.BeliefPropagationDecoder(30),
                                      "fused-bp-f64": lambda: A.BeliefPropagationDecoder(30, precision=A.PREC_F64)})[route]

    def call(dec, cws):
        return ints(A.run_experiment(dec, cws, H, SNR[code], frames=256, noise="device", seed=5))

    got, want = on_one_handle_and_fresh(make, call, [cws_a, cws_b, cws_a])
    assert got == want
    assert got[0] == got[2] and got[0] != got[1]  # (the raw-channel Hamming sums depend on the words sent)


@pytest.mark.parametrize("noise", ["device", "host"])
@pytest.mark.parametrize("code", ["H05", "n75"])
@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_grid_2_9_2_points_in_two_chunks(A, codes, monkeypatch, prec, code, noise):
    """acg_ldpc_mc_run_grid under ACG_MC_GRID_BUDGET = 500 virtual frames per launch: 100 frames x 9 points take two chunks
    of points (5 + 4), so the counter rows and the per-point tables grow between the calls and the tables are rewritten
    between the chunks"""
    H, cws, _ = codes[code]
    monkeypatch.setenv("ACG_MC_GRID_BUDGET", "500")
    precision = A.PREC_F32 if prec == "f32" else A.PREC_F64
    e_min = H.admm_shape()["e_min"]
    nine = ([0.9, 1.2, 1.95, 0.0, 1.5, 0.7, 1.95, 1.1, 0.4], [0.5, 0.55, 0.5, 0.0, 0.6, 0.3, 0.9, 0.45, 0.35])
    assert sum(e_min * m <= a for a, m in zip(*nine)) == 1  # one guard point (alpha = mu = 0)
    two = ([1.95, 1.2], [0.5, 0.55])

    def call(dec, pts):
        return [ints(r) for r in A.run_experiment_grid(dec, cws, H, SNR[code], pts[0], pts[1], frames=100, noise=noise, seed=9)]

    got, want = on_one_handle_and_fresh(lambda: A.QPADMMDecoder(1.0, 0.5, 60, 1e-5, precision=precision), call, [two, nine, two])
    assert got == want
    assert [len(g) for g in got] == [2, 9, 2] and got[0] == got[2] and all(r[2] == 100 for g in got for r in g)


def test_refused_create_then_create_then_destroy_behind_a_launch(A, codes):
    """QP-ADMM on the LDS engine refuses a code whose frame does not fit only after its tables were uploaded: the refusal
    releases them, the process goes on creating decoders, and a handle destroyed right behind an asynchronous
    acg_ldpc_decode_batch_dev on a caller stream lets that launch finish first"""
    import torch
    big = A.ParityCheckMatrix(A.regular_ldpc(1000, 2000, 3, 6, seed=1))
    for _ in range(2):
        refused = A.QPADMMDecoder(1.95, 0.5, 100, 1e-5, engine=A.ENGINE_FUSED)
        with pytest.raises(A.LdpcError, match="does not fit in LDS"):
            refused.handle(big)
        assert refused.live_handles() == 0
        refused.close()
    H, cws, _ = codes["H05"]
    F = 300
    y = A.transmit_frames(cws[np.arange(F) % len(cws)], SNR["H05"])
    for make in (lambda: A.BeliefPropagationDecoder(30), lambda: A.QPADMMDecoder(1.95, 0.5, 60, 1e-5),
                 lambda: A.BeliefPropagationDecoder(30, engine=A.ENGINE_STREAMED)):
        ref = make()
        want = ref.decode_batch(H, y, SNR["H05"])
        ref.close()
        dev = torch.device("cuda:0")
        yd = torch.from_numpy(y).to(dev)
        bits = torch.zeros((F, (H.n + 31) // 32), dtype=torch.int32, device=dev)
        ok = torch.full((F,), 7, dtype=torch.uint8, device=dev)
        iters = torch.full((F,), -1, dtype=torch.int32, device=dev)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        dec = make()
        dec.decode_batch_dev(H, yd.data_ptr(), True, F, SNR["H05"], bits.data_ptr(), ok.data_ptr(), iters.data_ptr(), stream.cuda_stream)
        dec.close()  # acg_ldpc_decoder_destroy with the launch possibly still in flight
        stream.synchronize()
        words = bits.cpu().numpy().view(np.uint32)
        unpacked = ((words[:, np.arange(H.n) // 32] >> (np.arange(H.n) % 32).astype(np.uint32)) & 1).astype(np.uint8)
        assert (ok.cpu().numpy() == want[1]).all() and (iters.cpu().numpy() == want[2]).all()
        assert (unpacked == want[0]).all()
