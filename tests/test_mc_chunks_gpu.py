"""GPU: the unfused route of acg_ldpc_mc_run (AWGN kernel -> decode -> classify kernel, csrc/mc.hip: mc_frames) across chunk
boundaries.  Its chunk is at least 2^31 / (4 n) frames — about 1.9 million for H05 — so no test reached a second chunk;
ACG_MC_CHUNK lowers it.  Any chunking and any sharding give the same seven counters, on a handle that classifies by the
decoder's flag (streamed BP) and on one that classifies with the CSR walk (workgroup-per-frame QP-ADMM)."""
import ctypes as C

import numpy as np
import pytest

from test_handle_buffers_gpu import INT_FIELDS, SNR

pytestmark = pytest.mark.gpu

FRAMES, FIRST, SEED = 300, 1000, 7


@pytest.fixture(scope="module")
def A():
    import acg_alp_ldpc_amd as A
    assert A.device_available(), "no HIP device: the product has no CPU fallback"
    return A


def ints(r):
    return {f: getattr(r, f) for f in INT_FIELDS}


@pytest.mark.parametrize("route", ["streamed-bp-f32", "admm-f32"])
def test_chunks_and_shards_give_the_same_counters(A, matrices, monkeypatch, route):
    """H05, 300 frames from frame 1000 (no multiple of the 37 codewords): ACG_MC_CHUNK=64 makes five chunks, the last of 44
    frames, none a multiple of 256; [0, 130) and [130, 300) merged with acg_ldpc_mc_merge; both equal the run in one chunk"""
    from acg_alp_ldpc_amd._lib import McCfg, McResult, lib
    H = A.ParityCheckMatrix(matrices["H05"])
    G, _ = H.get_orthogonal()
    cws = np.ascontiguousarray(A.gen_random_codewords(G, 37, 11), dtype=np.uint8)
    dec = {"streamed-bp-f32": lambda: A.BeliefPropagationDecoder(30, engine=A.ENGINE_STREAMED),
           "admm-f32": lambda: A.QPADMMDecoder(1.95, 0.5, 60, 1e-5, precision=A.PREC_F32)}[route]()
    try:
        if route == "admm-f32":
            assert "mc_grid=single-launch" in dec.describe(H)     # the workgroup-per-frame kernel: the unfused route, CSR walk

        def run():
            return ints(A.run_experiment(dec, cws, H, SNR["H05"], frames=FRAMES, first_frame=FIRST, noise="device", seed=SEED))

        whole = run()
        monkeypatch.setenv("ACG_MC_CHUNK", "64")
        chunked = run()
        monkeypatch.delenv("ACG_MC_CHUNK")
        h, _ = dec.handle(H)
        parts = []
        for lo, cnt in ((0, 130), (130, 170)):
            cfg = McCfg()
            cfg.frames, cfg.first_frame, cfg.snr, cfg.seed, cfg.noise = cnt, FIRST + lo, SNR["H05"], SEED, A._lib.NOISE_DEVICE_PHILOX
            cfg.codewords, cfg.n_codewords = cws.ctypes.data, cws.shape[0]
            r = McResult()
            assert lib().acg_ldpc_mc_run(h, C.byref(cfg), C.byref(r)) == 0, lib().acg_ldpc_last_error()
            parts.append(r)
        lib().acg_ldpc_mc_merge(C.byref(parts[0]), C.byref(parts[1]))
        merged = ints(parts[0])
        print(route, whole)
        assert chunked == whole, (chunked, whole)
        assert merged == whole, (merged, whole)
        assert whole["total"] == FRAMES and whole["sum_iters"] > 0 and whole["sum_hamming"] > 0
    finally:
        dec.close()
