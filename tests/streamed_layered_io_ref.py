"""numpy restatement of the LLR entrance of the streamed float layered engine (acg_ldpc_decode_batch_llr, _llr_dev; the IO
instances of bp_streamed_layered_kernel): fp32 LLRs in, fp32 posterior LLRs out.

tests/layered_ref.py stays the one definition of the check arithmetic and of the control (_run_layered): layered_minsum and
layered_sumproduct_exact are called as they are.  Only their channel step is replaced for the duration of a call — by
prepare_llr: NaN -> +0, clamp to +-2^20, and nothing else (sum-product's ONE multiply by (float) Dom<float>::scale is the
`channel_llr_f32(...) * LOG2E_F32` of layered_sumproduct_exact itself) — and the output step is added: the posteriors= list, for
sum-product times (float) ln 2 in ONE fp32 multiply, back to natural-log LLR units.  A latched frame's posteriors are those of
the round boundary at which its word was formed (layer_step writes P for the live frames only); a failed frame's those after
max_iter iterations; max_iter = 0 returns the clamped input (sum-product: scaled and scaled back)."""
import contextlib
import threading

import numpy as np

import layered_ref

LLR_CLAMP = np.float32(1048576.0)               # 2^20
LN2_F32 = np.float32(0.6931471805599453)
_swap = threading.Lock()


def prepare_llr(L):
    """what the kernel's fill() makes of fp32 LLRs before sum-product's multiply: NaN -> +0, then clamp to +-2^20 (-0 stays -0)"""
    x = np.array(L, dtype=np.float32)
    x[np.isnan(x)] = np.float32(0.0)
    return np.minimum(np.maximum(x, -LLR_CLAMP), LLR_CLAMP)


@contextlib.contextmanager
def _channel_step(P0):
    """layered_ref.channel_llr_f32 returns P0 while the block runs"""
    with _swap:
        kept = layered_ref.channel_llr_f32
        layered_ref.channel_llr_f32 = lambda y, snr, symbols_f32=False: P0
        try:
            yield
        finally:
            layered_ref.channel_llr_f32 = kept


def decode_llr(Hm, layers, L, max_iter, algo, scale=1.0, phi=None):
    """Hm, layers, max_iter, scale, phi: as layered_ref.layered_minsum (algo = "minsum") / layered_sumproduct_exact ("bp");
    L: [F, n] LLRs, positive = bit 0 (any real dtype, rounded to fp32 first).
    -> bits [F, n] uint8 (zeros for failed frames), ok [F] uint8, iters [F] int32, post [F, n] float32"""
    assert algo in ("minsum", "bp")
    L = np.asarray(L)
    P0 = prepare_llr(L)
    post = []
    with _channel_step(P0):
        if algo == "minsum":
            bits, ok, iters = layered_ref.layered_minsum(Hm, layers, L, 0.0, max_iter, scale, posteriors=post)
        else:
            bits, ok, iters = layered_ref.layered_sumproduct_exact(Hm, layers, L, 0.0, max_iter, phi, posteriors=post)
    P = post[0]
    assert P.dtype == np.float32
    return bits, ok, iters, (P if algo == "minsum" else P * LN2_F32)
