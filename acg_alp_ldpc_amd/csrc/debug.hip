// C ABI of libacg_ldpc_hip.so (include/acg_ldpc.h), part 4: the acg_ldpc_debug_* helpers (tests only).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "handle.hpp"

using namespace acg;

extern "C" {

static int acg_ldpc_debug_bp_trace_impl(const acg_ldpc_code *code, const double *y, int32_t frames, double snr, int32_t iters,
                            int32_t f64, int32_t engine, int32_t lanes_per_frame, double *c2v, double *v2c_mag,
                            double *v2c_sgn, double *post) {
    if (!code || !y || frames < 1 || frames > 64 || iters < 1) {
        set_error("bad argument (1..64 frames, iters >= 1)");
        return 1;
    }
    const bool fused = (engine == ACG_LDPC_ENGINE_FUSED);
    acg_ldpc_params p;
    acg_ldpc_params_default(&p);
    p.algo = ACG_LDPC_BP_SUMPRODUCT;
    p.max_iter = iters;
    p.early_exit = 0;
    p.engine = fused ? ACG_LDPC_ENGINE_FUSED : ACG_LDPC_ENGINE_STREAMED;
    p.lanes_per_frame = fused ? lanes_per_frame : 0;
    p.precision = f64 ? ACG_LDPC_PREC_F64 : ACG_LDPC_PREC_DEFAULT;
    acg_ldpc_decoder *made = nullptr;
    if (int rc = acg_ldpc_decoder_create(code, &p, &made)) return rc;
    const DecoderPtr own(made);  // destroyed on every return, after the three dumps below
    acg_ldpc_decoder *d = made;
    const int n = d->c.n, E = d->c.E;
    const size_t ts = f64 ? 8 : 4;
    // words per frame of the three dumps: streamed [E][64] / [E][64] / [n][64]; fused [frame][a_words] x2 / [frame][n_vpass*L]
    size_t wc = (size_t) E * 64, wp = (size_t) n * 64;
    if (fused) {
        const void *kp = nullptr;
        // ACG_BP_TRACE_SAT=1 / 2 (tests): the dump from the fixed-work instance with the phi fast path / with the one-series phi
        // as well, in the place of the plain instance (fp32, 32 lanes per frame)
        const char *tenv = getenv("ACG_BP_TRACE_SAT");
        const int tsat = tenv ? atoi(tenv) : 0;
        if (d->variant == 2 && d->maxd <= 8) kp = bp_kernel_ptr_dbg(f64, d->L, tsat);
        else if (d->variant == -1 && d->L == 256 && d->blk_idxlds && !d->blk_idxreg) kp = bp_block_kernel_ptr_dbg(f64);
        if (!kp) {
            set_error("no debug instance of the fused kernel for this code / lanes_per_frame");
            return 3;
        }
        if (d->lds_block > 64 * 1024) (void) hipFuncSetAttribute(kp, hipFuncAttributeMaxDynamicSharedMemorySize, (int) d->lds_block);
        d->kernel[0] = kp;
        // absorbed degree-1 variables: their edge words and LLRs follow the message array / the slot-order LLRs
        wc = (size_t) frames * (d->tab.a_words + d->lay.n_apass * d->L);
        wp = (size_t) frames * (d->lay.n_vpass + d->lay.n_apass) * d->L;
    }
    DeviceBuf dc, dv, dp;
    if (dc.reserve(wc * ts) || dv.reserve(wc * ts) || dp.reserve(wp * ts)) {
        set_error("hipMalloc failed");
        return 10;
    }
    if (int rc = ensure_staging(d, frames)) return rc;
    if (hipMemcpy(d->st_y.p, y, (size_t) frames * n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return 10;
    DecodeArgs a = decode_args(d->st_y.p, 1, frames, snr);
    stage_outputs(d, a);
    a.dbg_c2v = dc.p;
    a.dbg_v2c = dv.p;
    a.dbg_post = dp.p;
    if (int rc = launch_decode(d, a, d->stream)) return rc;
    if (hipStreamSynchronize(d->stream) != hipSuccess) {
        set_error("sync failed");
        return 10;
    }
    std::vector<unsigned char> hc(wc * ts), hv(wc * ts), hp(wp * ts);
    (void) hipMemcpy(hc.data(), dc.p, hc.size(), hipMemcpyDeviceToHost);
    (void) hipMemcpy(hv.data(), dv.p, hv.size(), hipMemcpyDeviceToHost);
    (void) hipMemcpy(hp.data(), dp.p, hp.size(), hipMemcpyDeviceToHost);
    // the fp32 kernels work in the log2(e)-scaled message domain (bp_core.inc: Dom<float>): undo it here
    const double unscale = f64 ? 1.0 : 0.693147180559945309;
    auto get = [&](const std::vector<unsigned char> &b, size_t idx) -> double {
        if (f64) return reinterpret_cast<const double *>(b.data())[idx];
        return unscale * (double) reinterpret_cast<const float *>(b.data())[idx];
    };
    // a v->c word = magnitude | hard-decision bit in the LSB | sign: strip the LSB before reading it
    auto get_v2c = [&](size_t idx) -> double {
        if (f64) {
            uint64_t u = reinterpret_cast<const uint64_t *>(hv.data())[idx] & ~1ull;
            double w;
            std::memcpy(&w, &u, 8);
            return w;
        }
        uint32_t u = reinterpret_cast<const uint32_t *>(hv.data())[idx] & ~1u;
        float wf;
        std::memcpy(&wf, &u, 4);
        return unscale * (double) wf;
    };
    // where edge e (check-major, variables ascending — the oracle's trace order) and variable v live in the dumps
    std::vector<size_t> epos((size_t) E), vslot((size_t) n, (size_t) -1);
    if (fused) {
        const BpLayout &lay = d->lay;
        for (int sl = 0; sl < lay.n_cpass * lay.L; sl++) {
            const int chk = lay.c_chk[sl];
            if (chk < 0) continue;
            const int pss = sl / lay.L, l = sl % lay.L;
            const int q = pss - (lay.n_cpass - lay.n_apass);  // >= 0: absorbed pass, its last edge is the register word
            const int deg = d->c.row_ptr[chk + 1] - d->c.row_ptr[chk];
            for (int j = 0; j < deg; j++)
                epos[(size_t) d->c.row_ptr[chk] + j] = (q >= 0 && j == deg - 1)
                                                           ? (size_t) d->tab.a_words + (size_t) q * lay.L + l
                                                           : (size_t) lay.c_off[pss] + (size_t) j * lay.L + l;
        }
        for (int sl = 0; sl < lay.n_vpass * lay.L; sl++)
            if (lay.v_var[sl] >= 0) vslot[lay.v_var[sl]] = (size_t) sl;
        for (int sl = 0; sl < lay.n_apass * lay.L; sl++)
            if (lay.a_var[sl] >= 0) vslot[lay.a_var[sl]] = (size_t) lay.n_vpass * lay.L + sl;
    }
    const size_t cstride = (size_t) d->tab.a_words + (size_t) d->lay.n_apass * d->L;
    const size_t pstride = (size_t) (d->lay.n_vpass + d->lay.n_apass) * d->L;
    for (int f = 0; f < frames; f++) {
        auto eidx = [&](int e) { return fused ? (size_t) f * cstride + epos[e] : (size_t) e * 64 + f; };
        for (int e = 0; e < E; e++) {
            c2v[(size_t) f * E + e] = get(hc, eidx(e));
            const double w = get_v2c(eidx(e));
            v2c_mag[(size_t) f * E + e] = std::fabs(w);
            v2c_sgn[(size_t) f * E + e] = std::signbit(w) ? -1.0 : 1.0;
        }
        for (int v = 0; v < n; v++) {
            if (!fused) {
                post[(size_t) f * n + v] = get(hp, (size_t) v * 64 + f);
                continue;
            }
            // estimate() = llr + sum of the c->v mailbox (bp.h:85-90), summed here from the kernel's own c->v words
            // and channel LLR (slot order dump), checks ascending
            double sum = 0;
            for (int k = d->c.col_ptr[v]; k < d->c.col_ptr[v + 1]; k++) sum += c2v[(size_t) f * E + d->c.col_edge[k]];
            post[(size_t) f * n + v] = get(hp, (size_t) f * pstride + vslot[v]) + sum;
        }
    }
    return 0;
}

int acg_ldpc_debug_bp_trace(const acg_ldpc_code *code, const double *y, int32_t frames, double snr, int32_t iters,
                            int32_t f64, int32_t engine, int32_t lanes_per_frame, double *c2v, double *v2c_mag,
                            double *v2c_sgn, double *post) {
    return guarded([&] { return acg_ldpc_debug_bp_trace_impl(code, y, frames, snr, iters, f64, engine, lanes_per_frame, c2v, v2c_mag, v2c_sgn, post); });
}

int acg_ldpc_debug_ring_tasks(const acg_ldpc_code *code, int32_t *n_ctask, int32_t *n_vtask, int32_t *ctask, int32_t *vtask, int64_t cap,
                              int32_t *consts) {
    return guarded([&]() -> int {
        if (!code) {
            set_error("null argument");
            return 1;
        }
        RingTasks rt;
        ring_tasks_build(code->c, rt);
        if (n_ctask) *n_ctask = rt.n_ctask;
        if (n_vtask) *n_vtask = rt.n_vtask;
        if (ctask)
            for (int64_t i = 0; i < std::min<int64_t>(cap, (int64_t) rt.ctask.size()); i++) ctask[i] = rt.ctask[(size_t) i];
        if (vtask)
            for (int64_t i = 0; i < std::min<int64_t>(cap, (int64_t) rt.vtask.size()); i++) vtask[i] = rt.vtask[(size_t) i];
        if (consts) {
            consts[0] = RING_WAVES;
            consts[1] = RING_SLOTS;
            consts[2] = RING_SLOT_LINES;
            consts[3] = RING_VAR_EDGE_LINES;
        }
        return 0;
    });
}

static int debug_layers_block(const acg_ldpc_code *code, int max_degree, int32_t *n_layers, int32_t *width, int32_t *qc_Z, int32_t *chk, int64_t cap) {
    return guarded([&]() -> int {
        if (!code) {
            set_error("null argument");
            return 1;
        }
        LayeredBlockLayout ll;
        if (!bp_layered_block_build(code->c, ll, max_degree)) return 3;
        if (n_layers) *n_layers = ll.n_sets;
        if (width) *width = ll.width;
        if (qc_Z) *qc_Z = ll.qc ? ll.Z : 0;
        if (chk)
            for (int64_t i = 0; i < std::min<int64_t>(cap, (int64_t) ll.chk.size()); i++) chk[i] = ll.chk[(size_t) i];
        return 0;
    });
}

int acg_ldpc_debug_layers_block(const acg_ldpc_code *code, int32_t *n_layers, int32_t *width, int32_t *qc_Z, int32_t *chk, int64_t cap) {
    return debug_layers_block(code, 8, n_layers, width, qc_Z, chk, cap);
}

int acg_ldpc_debug_layers_wide(const acg_ldpc_code *code, int32_t *n_layers, int32_t *width, int32_t *qc_Z, int32_t *chk, int64_t cap) {
    return debug_layers_block(code, 32, n_layers, width, qc_Z, chk, cap);
}

int acg_ldpc_debug_layers_any(const acg_ldpc_code *code, int32_t *n_layers, int32_t *width, int32_t *qc_Z, int32_t *chk, int64_t cap) {
    return debug_layers_block(code, INT32_MAX, n_layers, width, qc_Z, chk, cap);
}

int acg_ldpc_debug_layers(const acg_ldpc_code *code, int32_t *lanes, int32_t *n_layers, int32_t *qc_Z, int32_t *chk, int64_t cap) {
    return guarded([&]() -> int {
        if (!code) {
            set_error("null argument");
            return 1;
        }
        LayeredLayout ll;
        if (!bp_layered_build(code->c, ll)) return 3;
        if (lanes) *lanes = ll.G;
        if (n_layers) *n_layers = ll.n_layers;
        if (qc_Z) *qc_Z = ll.qc ? ll.Z : 0;
        if (chk)
            for (int64_t i = 0; i < std::min<int64_t>(cap, (int64_t) ll.chk.size()); i++) chk[i] = ll.chk[(size_t) i];
        return 0;
    });
}

static int acg_ldpc_debug_phi_impl(const void *x_host, void *out_host, int32_t n, int32_t f64) {
    const size_t es = f64 ? 8 : 4;
    DeviceBuf dx, dout;
    if (int rc = dx.reserve(es * n)) return rc;
    if (int rc = dout.reserve(es * n)) return rc;
    HIP_OK(hipMemcpy(dx.p, x_host, es * n, hipMemcpyHostToDevice));
    HIP_OK(phi_debug_launch(dx.p, dout.p, n, f64, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out_host, dout.p, es * n, hipMemcpyDeviceToHost));
    return 0;
}

int acg_ldpc_debug_phi(const void *x_host, void *out_host, int32_t n, int32_t f64) {
    return guarded([&] { return acg_ldpc_debug_phi_impl(x_host, out_host, n, f64); });
}

static int acg_ldpc_debug_quantize_impl(const void *y_host, int32_t y_is_f64, int64_t count, double snr, const acg_ldpc_quant *q,
                                        int16_t *out_host) {
    if (!y_host || !out_host || count < 0) {
        set_error("bad argument");
        return 1;
    }
    if (int rc = acg_ldpc_quant_check(q)) return rc;
    if (count == 0) return 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available: libacg_ldpc_hip has no CPU fallback");
        return 20;
    }
    const size_t es = y_is_f64 ? 8 : 4;
    DeviceBuf dy, dout;
    if (int rc = dy.reserve(es * (size_t) count)) return rc;
    if (int rc = dout.reserve(sizeof(int16_t) * (size_t) count)) return rc;
    HIP_OK(hipMemcpy(dy.p, y_host, es * (size_t) count, hipMemcpyHostToDevice));
    const DecodeArgs a = decode_args(dy.p, y_is_f64 ? 1 : 0, count, snr);
    HIP_OK(quantize_debug_launch(a, quant_args(*q), count, dout.as<int16_t>(), nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out_host, dout.p, sizeof(int16_t) * (size_t) count, hipMemcpyDeviceToHost));
    return 0;
}

int acg_ldpc_debug_quantize(const void *y_host, int32_t y_is_f64, int64_t count, double snr, const acg_ldpc_quant *q,
                            int16_t *out_host) {
    return guarded([&] { return acg_ldpc_debug_quantize_impl(y_host, y_is_f64, count, snr, q, out_host); });
}

static int acg_ldpc_debug_osd_soft_impl(const void *y_host, int32_t y_is_f64, int64_t count, int16_t *out_host) {
    if (!y_host || !out_host || count < 0) {
        set_error("bad argument");
        return 1;
    }
    if (count == 0) return 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available: libacg_ldpc_hip has no CPU fallback");
        return 20;
    }
    const size_t es = y_is_f64 ? 8 : 4;
    DeviceBuf dy, dout;
    if (int rc = dy.reserve(es * (size_t) count)) return rc;
    if (int rc = dout.reserve(sizeof(int16_t) * (size_t) count)) return rc;
    HIP_OK(hipMemcpy(dy.p, y_host, es * (size_t) count, hipMemcpyHostToDevice));
    HIP_OK(osd_soft_debug_launch(dy.p, y_is_f64 ? 1 : 0, count, dout.as<int16_t>(), nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out_host, dout.p, sizeof(int16_t) * (size_t) count, hipMemcpyDeviceToHost));
    return 0;
}

int acg_ldpc_debug_osd_soft(const void *y_host, int32_t y_is_f64, int64_t count, int16_t *out_host) {
    return guarded([&] { return acg_ldpc_debug_osd_soft_impl(y_host, y_is_f64, count, out_host); });
}

static int acg_ldpc_debug_phi_sat_impl(const void *x_host, void *out_host, int32_t n) {
    DeviceBuf dx, dout;
    if (int rc = dx.reserve(4 * (size_t) n)) return rc;
    if (int rc = dout.reserve(12 * (size_t) n)) return rc;
    HIP_OK(hipMemcpy(dx.p, x_host, 4 * (size_t) n, hipMemcpyHostToDevice));
    HIP_OK(phi_sat_debug_launch(dx.as<float>(), dout.as<uint32_t>(), n, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out_host, dout.p, 12 * (size_t) n, hipMemcpyDeviceToHost));
    return 0;
}

static int acg_ldpc_debug_freeze_stats_impl(acg_ldpc_decoder *d, int32_t enable, int64_t *frames_frozen, int64_t *sweeps_not_run) {
    if (!d) {
        set_error("null decoder");
        return 1;
    }
    std::lock_guard<std::recursive_mutex> lk(d->mu);
    HIP_OK(hipSetDevice(d->device));
    // every launch of the handle so far, on its own stream or a caller's
    HIP_OK(hipStreamSynchronize(d->stream));
    for (int k = 0; k < acg_ldpc_decoder::WORK_RING; k++)
        if (d->ring_used[k]) HIP_OK(hipEventSynchronize(d->ring_ev[k]));
    unsigned long long h = 0;
    if (d->freeze_ws.p) {  // the counter is the head of the workspace
        HIP_OK(hipMemcpy(&h, d->freeze_ws.p, sizeof(h), hipMemcpyDeviceToHost));
        HIP_OK(hipMemset(d->freeze_ws.p, 0, sizeof(h)));
    }
    if (frames_frozen) *frames_frozen = (int64_t) (h >> FREEZE_STATS_SHIFT);
    if (sweeps_not_run) *sweeps_not_run = (int64_t) (h & ((1ull << FREEZE_STATS_SHIFT) - 1));
    d->freeze_count = enable != 0 && d->freeze;
    return 0;
}

int acg_ldpc_debug_freeze_stats(acg_ldpc_decoder *d, int32_t enable, int64_t *frames_frozen, int64_t *sweeps_not_run) {
    return guarded([&] { return acg_ldpc_debug_freeze_stats_impl(d, enable, frames_frozen, sweeps_not_run); });
}

static int acg_ldpc_debug_freeze_passes_impl(acg_ldpc_decoder *d, int64_t *store_passes, int64_t *compare_passes) {
    if (!d) {
        set_error("null decoder");
        return 1;
    }
    std::lock_guard<std::recursive_mutex> lk(d->mu);
    HIP_OK(hipSetDevice(d->device));
    HIP_OK(hipStreamSynchronize(d->stream));
    for (int k = 0; k < acg_ldpc_decoder::WORK_RING; k++)
        if (d->ring_used[k]) HIP_OK(hipEventSynchronize(d->ring_ev[k]));
    unsigned long long h[2] = {0, 0};
    static_assert(FREEZE_WS_COMPARES == FREEZE_WS_STORES + 1 && (FREEZE_WS_COMPARES + 1) * 2 <= FREEZE_WS_HEAD, "the two counts are adjacent words of the head");
    if (d->freeze_ws.p) {
        unsigned long long *p = d->freeze_ws.as<unsigned long long>() + FREEZE_WS_STORES;
        HIP_OK(hipMemcpy(h, p, sizeof(h), hipMemcpyDeviceToHost));
        HIP_OK(hipMemset(p, 0, sizeof(h)));
    }
    if (store_passes) *store_passes = (int64_t) h[0];
    if (compare_passes) *compare_passes = (int64_t) h[1];
    return 0;
}

int acg_ldpc_debug_freeze_passes(acg_ldpc_decoder *d, int64_t *store_passes, int64_t *compare_passes) {
    return guarded([&] { return acg_ldpc_debug_freeze_passes_impl(d, store_passes, compare_passes); });
}

int acg_ldpc_debug_phi_sat(const void *x_host, void *out_host, int32_t n) {
    return guarded([&] { return acg_ldpc_debug_phi_sat_impl(x_host, out_host, n); });
}

static int acg_ldpc_debug_phi_split_impl(uint32_t *out_host) {
    if (!out_host) {
        set_error("null argument");
        return 1;
    }
    DeviceBuf dout;
    if (int rc = dout.reserve(sizeof(uint32_t) * PHI_SPLIT_NOUT)) return rc;
    HIP_OK(phi_split_debug_launch(dout.as<uint32_t>(), nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(out_host, dout.p, sizeof(uint32_t) * PHI_SPLIT_NOUT, hipMemcpyDeviceToHost));
    return 0;
}

int acg_ldpc_debug_phi_split(uint32_t *out_host) {
    return guarded([&] { return acg_ldpc_debug_phi_split_impl(out_host); });
}

// host only: a copy out of the workspace the streamed layered engines keep a tile's state in; no kernel takes part
static int acg_ldpc_debug_streamed_slab_impl(acg_ldpc_decoder *d, int32_t slab, void *out_host, int64_t cap_bytes, int64_t *slab_bytes) {
    if (!slab_bytes) {
        set_error("null slab_bytes");
        return 1;
    }
    *slab_bytes = 0;
    if (!d) {
        set_error("null decoder");
        return 1;
    }
    if (!d->streaml && !d->streamq) {
        set_error("acg_ldpc_debug_streamed_slab needs a decoder of acg_ldpc_decoder_create_layered_streamed or acg_ldpc_decoder_create_quantized_streamed");
        return 3;
    }
    std::lock_guard<std::recursive_mutex> lk(d->mu);
    const int tiles = d->sl_tiles;
    const int64_t bytes = d->sltab.slab_bytes;
    const unsigned char *ws = d->sl_ws.as<unsigned char>();
    *slab_bytes = bytes;
    if (slab < 0 || slab >= tiles) {
        set_error("slab " + std::to_string(slab) + " is outside 0 ... " + std::to_string(tiles - 1) + " (the handle's tiles)");
        return 1;
    }
    if (!out_host) return 0;  // the size query
    if (cap_bytes < 0) {
        set_error("negative cap_bytes");
        return 1;
    }
    HIP_OK(hipSetDevice(d->device));
    HIP_OK(hipDeviceSynchronize());  // every launch of the handle so far, on its own stream or a caller's
    const size_t take = (size_t) std::min<int64_t>(cap_bytes, bytes);
    if (take) HIP_OK(hipMemcpy(out_host, ws + (size_t) slab * (size_t) bytes, take, hipMemcpyDeviceToHost));
    return 0;
}

int acg_ldpc_debug_streamed_slab(acg_ldpc_decoder *d, int32_t slab, void *out_host, int64_t cap_bytes, int64_t *slab_bytes) {
    return guarded([&] { return acg_ldpc_debug_streamed_slab_impl(d, slab, out_host, cap_bytes, slab_bytes); });
}

}  // extern "C"
