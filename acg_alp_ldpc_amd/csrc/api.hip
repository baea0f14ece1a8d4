// C ABI of libacg_ldpc_hip.so (include/acg_ldpc.h), part 1: the error slot, the code entry points, and the creation, setup
// and description of decoder handles.  decode.hip holds the decode entry points, mc.hip the Monte-Carlo ones, debug.hip the
// test helpers; handle.hpp is what the four share.  There is deliberately NO CPU decode path in this library: without a HIP
// device every decoder entry point fails with an error code and message.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "handle.hpp"

namespace acg {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
const std::string &last_error() { return g_err; }

bool ScatteredAlloc::create(size_t want, size_t chunk_bytes, int dev, bool shuffle, int spread) {
    hipMemAllocationProp prop{};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = dev;
    size_t gran = 0;
    if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum) != hipSuccess || gran == 0) return false;
    chunk = (std::max(chunk_bytes, gran) + gran - 1) / gran * gran;
    const size_t n = (want + chunk - 1) / chunk;
    bytes = n * chunk;
    if (hipMemAddressReserve(&va, bytes, 0, nullptr, 0) != hipSuccess) {
        va = nullptr;
        return false;
    }
    handles.reserve(n);
    mapped.assign(n, 0);
    {
        std::vector<hipMemGenericAllocationHandle_t> spare;
        bool okc = true;
        for (size_t i = 0; i < n * (size_t) std::max(spread, 1) && okc; i++) {
            hipMemGenericAllocationHandle_t h;
            if (hipMemCreate(&h, chunk, &prop, 0) != hipSuccess) {
                okc = i >= n && handles.size() == n;   // out of memory while over-allocating: keep what there is if it suffices
                if (!okc && handles.size() < n && !spare.empty()) {  // not enough kept ones: take spares
                    while (handles.size() < n && !spare.empty()) {
                        handles.push_back(spare.back());
                        spare.pop_back();
                    }
                    okc = handles.size() == n;
                }
                break;
            }
            if (handles.size() < n && i % (size_t) std::max(spread, 1) == 0) handles.push_back(h);
            else spare.push_back(h);
        }
        while (handles.size() < n && !spare.empty()) {
            handles.push_back(spare.back());
            spare.pop_back();
        }
        for (auto &h : spare) (void) hipMemRelease(h);
        if (handles.size() != n) {
            (void) hipGetLastError();
            release();
            return false;
        }
    }
    // physical chunk i (creation order: neighbours in physical memory more often than not) -> virtual slot perm[i]
    std::vector<size_t> perm(n);
    for (size_t i = 0; i < n; i++) perm[i] = i;
    if (shuffle) {
        uint64_t x = 0x9E3779B97F4A7C15ull;  // fixed seed: the layout of a given size is the same in every process
        for (size_t i = n; i > 1; i--) {
            x ^= x << 13;
            x ^= x >> 7;
            x ^= x << 17;
            std::swap(perm[i - 1], perm[(size_t) (x % i)]);
        }
    }
    std::vector<hipMemGenericAllocationHandle_t> by_slot(n);
    for (size_t i = 0; i < n; i++) by_slot[perm[i]] = handles[i];
    handles = by_slot;
    for (size_t s = 0; s < n; s++) {
        if (hipMemMap((char *) va + s * chunk, chunk, 0, handles[s], 0) != hipSuccess) {
            release();
            return false;
        }
        mapped[s] = 1;
    }
    hipMemAccessDesc acc{};
    acc.location = prop.location;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    if (hipMemSetAccess(va, bytes, &acc, 1) != hipSuccess) {
        release();
        return false;
    }
    return true;
}

}  // namespace acg

using namespace acg;

// one check degree and one variable degree
static bool is_regular(const Code &c) {
    bool regular = c.max_cdeg >= 1 && c.max_vdeg >= 1;
    for (int i = 0; i < c.m && regular; i++) regular = (c.row_ptr[i + 1] - c.row_ptr[i] == c.max_cdeg);
    for (int j = 0; j < c.n && regular; j++) regular = (c.col_ptr[j + 1] - c.col_ptr[j] == c.max_vdeg);
    return regular;
}

// kernel[mc] (or the pair handed in) = kp: raise its dynamic-LDS limit where the workgroup needs more than 64 KiB, and size the grid by its occupancy
static int bind_kernel(acg_ldpc_decoder *d, const void *kp, const void *&kernel, int &grid_cap) {
    if (d->lds_block > 64 * 1024) HIP_OK(hipFuncSetAttribute(kp, hipFuncAttributeMaxDynamicSharedMemorySize, (int) d->lds_block));
    int occ = 0;
    HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kp, d->block, d->lds_block));
    kernel = kp;
    grid_cap = std::max(occ, 1) * d->cu_count;
    return 0;
}
static int bind_kernel(acg_ldpc_decoder *d, int mc, const void *kp) { return bind_kernel(d, kp, d->kernel[mc], d->grid_cap[mc]); }

extern "C" {

void acg_ldpc_params_default(acg_ldpc_params *p) {
    std::memset(p, 0, sizeof(*p));
    p->algo = ACG_LDPC_BP_SUMPRODUCT;
    p->max_iter = 50;
    p->alpha = 1.95;   // main.cpp:33
    p->mu = 0.5;
    p->eps_stop = 1e-5;  // qp_admm.h:182
    p->ms_scale = 1.0;
    p->early_exit = 1;
    p->precision = ACG_LDPC_PREC_DEFAULT;
    p->device = -1;
    p->lanes_per_frame = 0;
}

const char *acg_ldpc_last_error(void) { return g_err.c_str(); }

int acg_ldpc_device_available(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n > 0 ? 1 : 0;
}

// ---------------------------------------------------------------- code
static int acg_ldpc_code_from_dense_impl(const uint8_t *H, int32_t m, int32_t n, acg_ldpc_code **out) {
    if (!H || !out) {
        set_error("null argument");
        return 1;
    }
    auto *c = new acg_ldpc_code();
    if (!code_build(c->c, H, m, n)) {
        delete c;
        return 2;
    }
    *out = c;
    return 0;
}

int acg_ldpc_code_from_dense(const uint8_t *H, int32_t m, int32_t n, acg_ldpc_code **out) {
    return guarded([&] { return acg_ldpc_code_from_dense_impl(H, m, n, out); });
}

static int acg_ldpc_code_load_txt_impl(const char *path, acg_ldpc_code **out) {
    if (!path || !out) {
        set_error("null argument");
        return 1;
    }
    std::vector<uint8_t> H;
    int m = 0, n = 0;
    if (!code_read_txt(path, H, m, n)) return 2;
    return acg_ldpc_code_from_dense(H.data(), m, n, out);
}

int acg_ldpc_code_load_txt(const char *path, acg_ldpc_code **out) {
    return guarded([&] { return acg_ldpc_code_load_txt_impl(path, out); });
}

static int acg_ldpc_code_save_txt_impl(const acg_ldpc_code *code, const char *path) {
    if (!code || !path) {
        set_error("null argument");
        return 1;
    }
    return code_write_txt(code->c, path) ? 0 : 2;
}

int acg_ldpc_code_save_txt(const acg_ldpc_code *code, const char *path) {
    return guarded([&] { return acg_ldpc_code_save_txt_impl(code, path); });
}

void acg_ldpc_code_destroy(acg_ldpc_code *code) { delete code; }

void acg_ldpc_code_dims(const acg_ldpc_code *code, int32_t *m, int32_t *n, int32_t *E) {
    if (m) *m = code->c.m;
    if (n) *n = code->c.n;
    if (E) *E = code->c.E;
}

void acg_ldpc_code_dense(const acg_ldpc_code *code, uint8_t *H) {
    std::memcpy(H, code->c.H.data(), code->c.H.size());
}

void acg_ldpc_code_admm_shape(const acg_ldpc_code *code, int32_t *n_var, int32_t *n_con, int32_t *nnz, double *e_min,
                              double *e_max) {
    const AdmmLayout &a = code->c.admm;
    if (n_var) *n_var = a.n_var;
    if (n_con) *n_con = a.n_con;
    if (nnz) *nnz = a.nnz;
    if (e_min) *e_min = a.e_min;
    if (e_max) *e_max = a.e_max;
}

static int acg_ldpc_code_generator_impl(const acg_ldpc_code *code, uint8_t *G) {
    if (!code || !G) {
        set_error("null argument");
        return 2;
    }
    if (code->c.n <= code->c.m) {
        set_error("generator needs n > m");
        return 2;
    }
    return code_generator(code->c, G) ? 0 : 1;
}

int acg_ldpc_code_generator(const acg_ldpc_code *code, uint8_t *G) {
    return guarded([&] { return acg_ldpc_code_generator_impl(code, G); });
}

int acg_ldpc_code_is_codeword(const acg_ldpc_code *code, const uint8_t *bits) {
    return code_is_codeword(code->c, bits) ? 1 : 0;
}

}  // extern "C"

// ---------------------------------------------------------------- decoder
static int decoder_setup_streamed(acg_ldpc_decoder *d) {
    const Code &c = d->c;
    if (std::max(c.max_cdeg, c.max_vdeg) > 16) {
        set_error("node degree above 16 is not supported by the streamed BP engine");
        return 3;
    }
    d->streamed = true;
    d->f64 = (d->p.precision == ACG_LDPC_PREC_F64) ? 1 : 0;
    d->L = 1;
    StreamTables &t = d->stab;
#define UP32S(vec, field) \
    if (!(t.field = upload_keep(vec, d->dev_allocs))) return 10;
    UP32S(c.row_ptr, row_ptr)
    UP32S(c.col_ptr, col_ptr)
    UP32S(c.col_edge, col_edge)
    t.m = c.m;
    t.n = c.n;
    t.E = c.E;
    t.nwords = (c.n + 31) / 32;
    const size_t ts = d->f64 ? 8 : 4;
    // LDS-DMA ring engine (fp32, node degrees that fit a ring slot): cut the sweeps into tasks
    size_t hb_bytes = (size_t) t.nwords * 64 * 4;  // HB[nwords][64] (u32)
    if (!d->f64 && c.max_cdeg <= RING_MAX_CDEG && c.max_vdeg <= RING_MAX_VDEG && getenv("ACG_STREAM_NO_RING") == nullptr) {
        RingTasks rt;
        ring_tasks_build(c, rt);
        const std::vector<int32_t> &hct = rt.ctask, &hvt = rt.vtask, &hvw = rt.vtask_of_word;
        struct { size_t n; size_t size() const { return n; } } ct{(size_t) rt.n_ctask}, vt{(size_t) rt.n_vtask};
        std::vector<int32_t> ce = c.col_edge;
        ce.resize(ce.size() + 4, 0);  // the gather reads its edge ids four at a time
        UP32S(hct, ctask)
        UP32S(hvt, vtask)
        UP32S(hvw, vtask_of_word)
        UP32S(ce, col_edge)
        t.n_ctask = (int32_t) ct.size();
        t.n_vtask = (int32_t) vt.size();
        // slabs of all resident workgroups beyond the 256 MiB Infinity Cache: stream them with non-temporal accesses
        const size_t slab_bytes = ((size_t) (c.E + c.n) * 64 * ts + (size_t) vt.size() * 64);
        bool nt = slab_bytes * 3 * (size_t) d->cu_count > ((size_t) 256 << 20);
        if (getenv("ACG_STREAM_NT")) nt = atoi(getenv("ACG_STREAM_NT")) != 0;  // developer A/B only
        d->sring_nt = nt;
        d->sring = bp_streamed_ring_ptr((d->p.algo == ACG_LDPC_BP_MINSUM) ? 1 : 0, nt);
        HIP_OK(hipFuncSetAttribute(d->sring, hipFuncAttributeMaxDynamicSharedMemorySize, RING_LDS_BYTES));
        hb_bytes = std::max(hb_bytes, (size_t) vt.size() * 64);  // ring engine: one byte per (variable task, frame)
    }
#undef UP32S
    // per workgroup: M[E][64] + LLR[n][64] (T) + hard decisions
    t.ws_words_per_wave = (int64_t) (((size_t) (c.E + c.n) * 64 * ts + hb_bytes + 255) / 256 * 64);
    if (const char *pad = getenv("ACG_STREAM_SLAB_PAD")) t.ws_words_per_wave += (int64_t) (atol(pad) / 256 * 64);  // developer A/B: slab stride + pad bytes
    d->block = 256;
    d->frames_per_block = 64;  // one 64-frame tile per workgroup at a time
    const int algo = (d->p.algo == ACG_LDPC_BP_MINSUM) ? 1 : 0;
    d->skernel = bp_streamed_ptr(algo, d->f64);
    // 2 workgroups per CU (x 4 wavefronts = 8 waves/CU keep > 1 MB of 256-byte lines in flight per CU);
    // each resident workgroup owns one slab: M[E][64] + LLR[n][64] + HB[nwords][64]
    d->sgrid = 2 * d->cu_count;
    if (d->sring) {  // ring engine: as many workgroups per CU as their rings fit in LDS
        int per_cu = 2;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, d->sring, RING_WAVES * 64, RING_LDS_BYTES) != hipSuccess) per_cu = 2;
        d->sring_per_cu = std::max(1, std::min(per_cu, ACG_RING_MAX_PER_CU));
        d->sgrid = std::max(d->sgrid, d->sring_per_cu * d->cu_count);
    }
    const size_t ws_bytes = (size_t) d->sgrid * (size_t) t.ws_words_per_wave * 4;
    if (t.ws_words_per_wave < (int64_t) (c.E + c.n) * 64) {  // the kernels index the slab without further checks
        set_error("internal: streamed-engine slab size not set");
        return 11;
    }
    {
        // Where the slabs live decides the rate of the ring kernel once they exceed the Infinity Cache (configs[4]: 768 slabs of
        // 10.4 MB; tools/stream_bimodal.py, profiles/r03_stream_bimodal.txt: one process, same kernel instance, same virtual
        // address, a new allocation per measurement, three GPU boxes):
        //   hipDeviceMallocContiguous             181 ms per launch, every time, whatever the slab stride: a physically contiguous
        //                                         backing is the slowest one
        //   hipMalloc                             158 or 181 ms, fixed for the life of the allocation, decided anew by every
        //                                         hipMalloc (round 2's "158 or 179 ms depending on the box"); one box gave 180 only
        //   physical chunks mapped into one       149-153 ms on one box (20 of 20), 152-180 ms (mostly 157-169) on another: never
        //   virtual range (hipMemCreate/hipMemMap) worse than hipMalloc, but still a draw per allocation
        // What the draw is: how COMPACT the physical backing is.  Keeping only every K-th of K times as many chunks (the others
        // are released at once) spaces the kept ones out over a K times larger part of the device memory, and on a box whose
        // plain candidates all probed slow (20.1 ms, 180 ms per launch) K = 4 gave 158 ms and K = 16 gave 148 ms — the fast
        // mode, every time since (a compact region keeps few DRAM banks in play for 768 concurrent streams; that reading fits
        // every observation above, the physical addresses themselves are not visible).  So a workspace beyond the Infinity Cache
        // is built from 64 MiB chunks spaced out 16-fold (ACG_STREAM_WS_SPREAD; costs ~3 s of decoder creation and, for a moment,
        // 16 x the workspace in device memory — when that is not available the chunks that were obtained are used as they are).
        // ACG_STREAM_WS_TRIES > 1 additionally times several candidates with a three-sweep launch of the decoder's own kernel
        // and keeps the fastest (the probe is always taken and reported: 17 ms = fast, 20 ms = slow on configs[4]).
        // hipMalloc remains the fallback and the small-workspace path.  ACG_STREAM_WS_ALLOC = 0 / 1 / 2 / 3 forces hipMalloc /
        // contiguous / shuffled chunks / chunks in creation order (developer A/B only).
        const char *wa = getenv("ACG_STREAM_WS_ALLOC");
        const int mode = wa ? atoi(wa) : (ws_bytes >= ((size_t) 64 << 20) ? 2 : 0);
        hipError_t e = hipErrorUnknown;
        void *plain = nullptr;
        if (mode == 1) e = hipExtMallocWithFlags(&plain, ws_bytes, hipDeviceMallocContiguous);
        if (mode >= 2) {
            const char *cm = getenv("ACG_STREAM_WS_CHUNK_MB");
            const size_t chunk = (size_t) (cm ? atol(cm) : 64) << 20;
            const char *tr = getenv("ACG_STREAM_WS_TRIES");
            int tries = tr ? atoi(tr) : 1;
            // the placement only matters beyond the Infinity Cache, and the probe needs the ring kernel and room for its symbols
            const int64_t probe_frames = (int64_t) d->sgrid * 64;
            const bool big = ws_bytes > ((size_t) 512 << 20);
            const bool can_probe = d->sring && big && (size_t) probe_frames * c.n * 4 <= ws_bytes;
            if (!can_probe) tries = 1;
            tries = std::max(1, std::min(tries, 6));
            const char *sp = getenv("ACG_STREAM_WS_SPREAD");
            int spread = big ? std::max(1, std::min(sp ? atoi(sp) : 16, 64)) : 1;
            if (spread > 1) {   // never ask for more than ~80 % of the memory that is free right now
                size_t free_b = 0, total_b = 0;
                if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && ws_bytes > 0)
                    spread = (int) std::max<size_t>(1, std::min<size_t>((size_t) spread, (size_t) ((double) free_b * 0.8 / (double) ws_bytes)));
            }
            std::vector<ScatteredAlloc> cand((size_t) tries);
            int best = -1;
            float best_ms = 0;
            d->sws_probe_ms.clear();
            d->sws_spread = spread;
            for (int k = 0; k < tries; k++) {
                if (!cand[k].create(ws_bytes, chunk, d->device, mode == 2, spread)) break;
                float ms = 0;
                if (can_probe) {
                    DecodeArgs pa{};
                    pa.y = cand[k].va;           // any readable memory will do as symbols: the probe times traffic, not decoding
                    pa.y_is_f64 = 0;
                    pa.frames = probe_frames;
                    pa.inv_var2 = 1.0;
                    pa.var = 1.0;
                    pa.max_iter = 3;
                    pa.early_exit = 0;
                    pa.ms_scale = 0.75f;
                    pa.work_counter = d->work_counter(0);
                    bool okp = true;
                    for (int rep = 0; rep < 2 && okp; rep++) {   // the second launch is the one timed
                        okp = hipMemsetAsync(pa.work_counter, 0, sizeof(unsigned long long), d->stream) == hipSuccess &&
                              hipEventRecord(d->ring_ev0[0], d->stream) == hipSuccess &&
                              bp_streamed_ring_launch(d->sring, d->stab, pa, (uint32_t *) cand[k].va, d->sgrid, d->stream) == hipSuccess &&
                              hipEventRecord(d->ring_ev[0], d->stream) == hipSuccess && hipStreamSynchronize(d->stream) == hipSuccess;
                    }
                    if (!okp || hipEventElapsedTime(&ms, d->ring_ev0[0], d->ring_ev[0]) != hipSuccess) ms = 1e30f;
                    d->sws_probe_ms.push_back(ms);
                }
                if (best < 0 || ms < best_ms) {
                    best = k;
                    best_ms = ms;
                }
            }
            (void) hipGetLastError();
            if (best >= 0) {
                d->sws = std::move(cand[best]);
                e = hipSuccess;
            }
        }   // (the other candidates are released here)
        if (e != hipSuccess) {
            (void) hipGetLastError();
            HIP_OK(hipMalloc(&plain, ws_bytes));
        }
        if (plain) d->sws.adopt(plain, ws_bytes);
    }
    d->grid_cap[0] = d->grid_cap[1] = d->sgrid;
    return 0;
}

// One workgroup of L threads per frame (bp_layered_block.hip): the layered engines for codes whose frame is too large for a wavefront
// group (block: check degree <= 8), for high-rate codes (wide: a check of degree 9 ... 32, the same tables) and for fixed-point
// min-sum (q: acg_ldpc_decoder_create_quantized; check degree <= 32, int16 posteriors and one byte per edge).  The only size
// limit is the LDS of a CU: posteriors + messages + output word of ONE frame.
// L: 256, 512 or 1024 (q: also 64, 128); 0 stands for the smallest workgroup that takes the largest set in one pass, else 1024.
static int decoder_setup_layered_wg(acg_ldpc_decoder *d, const acg_ldpc_decoder::LayeredWg kind, int L) {
    using Wg = acg_ldpc_decoder::LayeredWg;
    const Code &c = d->c;
    const bool q = kind == Wg::q, f16 = d->p.precision == ACG_LDPC_PREC_F16;
    if (!bp_layered_block_build(c, d->lblay, kind == Wg::block ? 8 : 32)) return 3;
    const LayeredBlockLayout &ll = d->lblay;
    if (L == 0) {
        L = q ? 64 : 256;
        while (L < 1024 && L < ll.width) L <<= 1;
    }
    const int cell = q ? 2 : 4, msg = q ? 1 : (f16 ? 2 : 4);   // bytes of a posterior cell and of a message cell
    LayerBlockTables &t = d->lbtab;
    t.n = c.n;
    t.nwords = (c.n + 31) / 32;
    t.e = ll.e;
    t.n_sets = ll.n_sets;
    t.p_words = (int32_t) ((((size_t) c.n + 1 + 16 / cell - 1) & ~(size_t) (16 / cell - 1)) * cell / 4);   // n + the neutral cell, padded to 16 bytes
    t.r_words = (int32_t) (((size_t) ll.e * msg + 3) / 4);
    const size_t lds = ((size_t) t.p_words + (size_t) t.r_words + (size_t) t.nwords) * 4;
    const int algo = d->p.algo == ACG_LDPC_BP_MINSUM ? 1 : 0;
    const void *kp = q ? bp_layered_q_kernel_ptr(L, false) : (kind == Wg::wide ? bp_layered_wide_kernel_ptr(L, f16, algo) : bp_layered_block_kernel_ptr(L, f16, algo));
    if (!kp) {
        set_error(q ? "no quantized layered kernel instance for this lanes_per_frame" : "no layered workgroup-per-frame kernel instance for this lanes_per_frame");
        return 3;
    }
    hipFuncAttributes fa{};
    HIP_OK(hipFuncGetAttributes(&fa, kp));
    if (lds + fa.sharedSizeBytes > 160 * 1024 || c.n >= (1 << 30)) {   // (sharedSizeBytes: the kernel's few control words)
        set_error(std::string(q ? "quantized layered min-sum" : "layered schedule") + ": a frame (posteriors + messages) does not fit in LDS");
        return 3;
    }
    std::vector<int32_t> step, pos(ll.pos.size());
    bp_layered_block_steps(ll, L, step);
    for (size_t i = 0; i < ll.pos.size(); i++) pos[i] = cell * ll.pos[i];
    d->lb_step = upload(step, 8);
    d->lb_pos = upload(pos);
    if (!d->lb_step.p || !d->lb_pos.p) return 10;
    t.step = d->lb_step.as<const int32_t>();
    t.pos = d->lb_pos.as<const int32_t>();
    t.n_steps = (int) (step.size() / 8);
    d->layered_wg = kind;
    if (q) d->qargs = quant_args(d->quant);
    d->L = L;
    d->f64 = 0;
    d->block = L;
    d->frames_per_block = 1;
    d->lds_block = lds;
    // decode only: a Monte-Carlo run goes AWGN kernel -> decode -> classification kernel (acg_ldpc_mc_run)
    if (int rc = bind_kernel(d, 0, kp)) return rc;
    d->kernel[1] = nullptr;
    d->grid_cap[1] = d->grid_cap[0];
    if (q) {
        // the integer entrance's instance of the same workgroup (acg_ldpc_decode_batch_q*): its own LDS limit and occupancy
        const void *kio = bp_layered_q_kernel_ptr(L, true);
        HIP_OK(hipFuncGetAttributes(&fa, kio));
        if (lds + fa.sharedSizeBytes > 160 * 1024) {
            set_error("quantized layered min-sum: a frame (posteriors + messages) does not fit in LDS");
            return 3;
        }
        if (int rc = bind_kernel(d, kio, d->kernel_qio, d->grid_cap_qio)) return rc;
        // and the grid form of the symbol entrance (acg_ldpc_mc_run_quants)
        const void *kgrid = bp_layered_q_grid_kernel_ptr(L);
        HIP_OK(hipFuncGetAttributes(&fa, kgrid));
        if (lds + fa.sharedSizeBytes > 160 * 1024) {
            set_error("quantized layered min-sum: a frame (posteriors + messages) does not fit in LDS");
            return 3;
        }
        if (int rc = bind_kernel(d, kgrid, d->kernel_qgrid, d->grid_cap_qgrid)) return rc;
    }
    d->tab.lds_bytes_per_frame = (int32_t) lds;
    return 0;
}

// what algo = ACG_LDPC_OSD requires of the params (include/acg_ldpc.h, "OSD"); host only
static int osd_params_check(const acg_ldpc_params &p, const Code &c) {
    const char *why = nullptr;
    if (p.max_iter != 0 && p.max_iter != 1) why = "max_iter is the order and must be 0 or 1";
    else if (p.precision != ACG_LDPC_PREC_DEFAULT) why = "precision must be ACG_LDPC_PREC_DEFAULT (every value is an integer)";
    else if (p.engine != ACG_LDPC_ENGINE_AUTO && p.engine != ACG_LDPC_ENGINE_FUSED) why = "engine must be ACG_LDPC_ENGINE_AUTO or ACG_LDPC_ENGINE_FUSED (the state lives in LDS)";
    else if (p.schedule != ACG_LDPC_SCHEDULE_FLOODING) why = "schedule must be ACG_LDPC_SCHEDULE_FLOODING (there is no schedule)";
    else if (p.lanes_per_frame != 0 && p.lanes_per_frame != 64 && p.lanes_per_frame != 128 && p.lanes_per_frame != 256)
        why = "lanes_per_frame must be 0, 64, 128 or 256";
    else if (c.n > 65535) why = "n must be <= 65535 (the sort key holds the variable in 16 bits)";
    if (why) {
        set_error(std::string("OSD: ") + why);
        return 3;
    }
    return 0;
}

// algo = ACG_LDPC_OSD: one workgroup per frame, the frame's working matrix in LDS (osd.hip)
static int decoder_setup_osd(acg_ldpc_decoder *d) {
    const Code &c = d->c;
    int L = d->p.lanes_per_frame;
    if (L == 0) {
        L = 64;
        while (L < 256 && 2 * L < c.n) L <<= 1;
    }
    OsdArgs &o = d->oargs;
    o.n = c.n;
    o.m = c.m;
    o.nwords = (c.n + 31) / 32;
    o.wm = (c.m + 31) / 32;
    o.stride = o.wm | 1;
    o.order = d->p.max_iter;
    o.s_in = nullptr;
    const size_t lds = osd_lds_bytes(c.n, c.m);
    const void *kp = osd_kernel_ptr(L);
    if (!kp) {
        set_error("OSD: no kernel instance for this lanes_per_frame");
        return 3;
    }
    hipFuncAttributes fa{};
    HIP_OK(hipFuncGetAttributes(&fa, kp));
    if (lds + fa.sharedSizeBytes > 160 * 1024) {
        set_error("OSD: a frame (working matrix of " + std::to_string(c.n) + " columns x " + std::to_string(o.wm) + " words, keys, pivots, word = " +
                  std::to_string(lds) + " bytes) does not fit in LDS");
        return 3;
    }
    std::vector<uint32_t> cols;
    o.rank = code_osd_table(c, o.stride, cols);
    d->osd_cols = upload(cols);
    if (!d->osd_cols.p) return 10;
    o.cols = d->osd_cols.as<const uint32_t>();
    d->osd = true;
    d->L = L;
    d->f64 = 0;
    d->block = L;
    d->frames_per_block = 1;
    d->lds_block = lds;
    if (int rc = bind_kernel(d, 0, kp)) return rc;
    d->kernel[1] = nullptr;
    d->grid_cap[1] = d->grid_cap[0];
    d->tab.lds_bytes_per_frame = (int32_t) lds;
    return 0;
}

// acg_ldpc_quant -> what the kernel reads
QuantArgs acg::quant_args(const acg_ldpc_quant &q) {
    QuantArgs a{};
    a.inv_step = (float) (1.0 / q.llr_step);
    a.cmax = (1 << (q.ch_bits - 1)) - 1;
    a.rmax = (1 << (q.msg_bits - 1)) - 1;
    a.pmax = (1 << (q.post_bits - 1)) - 1;
    a.scale_num = q.scale_num;
    a.scale_shift = q.scale_shift;
    a.rnd = q.scale_shift > 0 ? 1 << (q.scale_shift - 1) : 0;
    a.offset = q.offset;
    return a;
}

// the rules of acg_ldpc_quant (include/acg_ldpc.h); host only
static int quant_check(const acg_ldpc_quant *q) {
    if (!q) {
        set_error("null quantiser");
        return 1;
    }
    const char *why = nullptr;
    if (!(std::isfinite(q->llr_step) && q->llr_step > 0)) why = "llr_step must be finite and > 0";
    else if (q->post_bits < 2 || q->post_bits > 16) why = "post_bits must be 2 ... 16";
    else if (q->ch_bits < 2 || q->ch_bits > q->post_bits) why = "ch_bits must be 2 ... post_bits";
    else if (q->msg_bits < 2 || q->msg_bits > 8 || q->msg_bits > q->post_bits) why = "msg_bits must be 2 ... 8 and <= post_bits";
    else if (q->scale_shift < 0 || q->scale_shift > 8) why = "scale_shift must be 0 ... 8";
    else if (q->scale_num < 1 || q->scale_num > (1 << q->scale_shift)) why = "scale_num must be 1 ... 2^scale_shift";
    else if (q->offset < 0 || q->offset > (1 << (q->msg_bits - 1)) - 1) why = "offset must be 0 ... 2^(msg_bits-1) - 1";
    if (why) {
        set_error(std::string("invalid quantiser: ") + why);
        return 3;
    }
    return 0;
}

// what acg_ldpc_decoder_create_quantized requires of the params (include/acg_ldpc.h); host only
static int quant_params_check(const acg_ldpc_params &p) {
    const char *why = nullptr;
    if (p.algo != ACG_LDPC_BP_MINSUM) why = "algo must be ACG_LDPC_BP_MINSUM";
    else if (p.schedule != ACG_LDPC_SCHEDULE_LAYERED) why = "schedule must be ACG_LDPC_SCHEDULE_LAYERED";
    else if (p.precision != ACG_LDPC_PREC_DEFAULT) why = "precision must be ACG_LDPC_PREC_DEFAULT (the number formats are the quantiser's)";
    else if (p.engine != ACG_LDPC_ENGINE_AUTO && p.engine != ACG_LDPC_ENGINE_FUSED) why = "engine must be ACG_LDPC_ENGINE_AUTO or ACG_LDPC_ENGINE_FUSED (the state lives in LDS)";
    else if (p.lanes_per_frame != 0 && p.lanes_per_frame != 64 && p.lanes_per_frame != 128 && p.lanes_per_frame != 256 && p.lanes_per_frame != 512 &&
             p.lanes_per_frame != 1024)
        why = "lanes_per_frame must be 0, 64, 128, 256, 512 or 1024";
    if (why) {
        set_error(std::string("quantized layered min-sum: ") + why);
        return 3;
    }
    return 0;
}

// what the two streamed layered engines require of the params, in the order in which a message wins.  algo_why: the engine's own
// objection to p.algo, or null; precision_why: its text for a precision other than the default.  Host only.
static int streamed_layered_params_check(const acg_ldpc_params &p, const char *what, const char *algo_why, const char *precision_why) {
    const char *why = nullptr;
    if (algo_why) why = algo_why;
    else if (p.schedule != ACG_LDPC_SCHEDULE_LAYERED) why = "schedule must be ACG_LDPC_SCHEDULE_LAYERED";
    else if (p.precision != ACG_LDPC_PREC_DEFAULT) why = precision_why;
    else if (p.engine != ACG_LDPC_ENGINE_AUTO && p.engine != ACG_LDPC_ENGINE_STREAMED) why = "engine must be ACG_LDPC_ENGINE_AUTO or ACG_LDPC_ENGINE_STREAMED (the state lives in device memory)";
    else if (p.lanes_per_frame != 0) why = "lanes_per_frame must be 0 (one lane is one frame)";
    if (why) {
        set_error(std::string(what) + why);
        return 3;
    }
    return 0;
}

// what acg_ldpc_decoder_create_quantized_streamed requires of the params (include/acg_ldpc.h)
static int streamq_params_check(const acg_ldpc_params &p) {
    return streamed_layered_params_check(p, "streamed quantized layered min-sum: ", p.algo != ACG_LDPC_BP_MINSUM ? "algo must be ACG_LDPC_BP_MINSUM" : nullptr,
                                         "precision must be ACG_LDPC_PREC_DEFAULT (the number formats are the quantiser's)");
}
// what acg_ldpc_decoder_create_layered_streamed requires of them
static int streaml_params_check(const acg_ldpc_params &p) {
    return streamed_layered_params_check(p, "streamed layered BP: ",
                                         p.algo != ACG_LDPC_BP_SUMPRODUCT && p.algo != ACG_LDPC_BP_MINSUM ? "algo must be ACG_LDPC_BP_SUMPRODUCT or ACG_LDPC_BP_MINSUM" : nullptr,
                                         "precision must be ACG_LDPC_PREC_DEFAULT (posteriors and messages are fp32)");
}

// the checks of the streamed layered engines in processing order — the sets of `ll`, set by set — as a plain CSR
static void streamed_layered_csr(const Code &c, const LayeredBlockLayout &ll, std::vector<int32_t> &row_ptr, std::vector<int32_t> &edge_var) {
    row_ptr.reserve((size_t) c.m + 1);
    edge_var.reserve((size_t) c.E);
    row_ptr.push_back(0);
    for (int k = 0; k < ll.n_sets; k++) {
        const int cnt = ll.set[3 * k + 2];
        for (int i = 0; i < cnt; i++) {
            const int r = ll.chk[(size_t) k * ll.width + i];
            edge_var.insert(edge_var.end(), c.edge_var.begin() + c.row_ptr[r], c.edge_var.begin() + c.row_ptr[r + 1]);
            row_ptr.push_back((int32_t) edge_var.size());
        }
    }
}

// Resident tiles per CU of the streamed layered engines, at most.
// The integer engine, measured on frames that never latch, 4 / 8 / 12 / 16 / 20 per CU: 386 / 576 / 762 / 780 / 770 k frames/s on the
// (3,6) 5000 x 10000, 153 / 233 / 223 / 223 from 8 on the 2050 x 41000 of degree 40; DESIGN 3h.
// The float engine at 4 / 8 / 12 / 16 per CU, 25 iterations fixed, k frames/s (tools/streamed_layered_rate.py): (3,6)
// 5000 x 10000 at +2 dB, sum-product 332 / 477 / 701 / 680, min-sum 421 / 581 / 844 / 772; 2050 x 41000 of degree 40 at 5.3 dB, where
// a quarter of the free memory holds 8.9 per CU whatever is asked beyond that, sum-product 88 / 123 / 115 / 126, min-sum 121 / 141 /
// 134 / 140 (the last two columns are one configuration).
constexpr int STREAMED_LAYERED_TILES_PER_CU = 12;

// What the two streamed layered engines set up alike: the checks — the sets of bp_layered_block_build without a degree cap, set
// by set — as a plain CSR on the device, the slab of a tile of 64 frames at bytes_per_frame (P, R and the engine's scratch), the
// tiles and their slabs, and the handle's launch shape.  Any n, m, E and any check degree.
// `what` opens the error texts; tiles_env and per_cu_env (or null) name the engine's developer switches.
static int decoder_setup_streamed_layered(acg_ldpc_decoder *d, const void *kernel, size_t bytes_per_frame, const char *what, const char *tiles_env,
                                          const char *per_cu_env) {
    const Code &c = d->c;
    if (!bp_layered_block_build(c, d->lblay, INT32_MAX)) return 3;
    std::vector<int32_t> row_ptr, edge_var;
    streamed_layered_csr(c, d->lblay, row_ptr, edge_var);
    StreamLayTables &t = d->sltab;
    if (!(t.row_ptr = upload_keep(row_ptr, d->dev_allocs))) return 10;
    if (!(t.edge_var = upload_keep(edge_var, d->dev_allocs))) return 10;
    t.m = (int32_t) row_ptr.size() - 1;
    t.n = c.n;
    t.E = (int32_t) edge_var.size();   // (= c.E, and max_deg = c.max_cdeg: every check with a variable is in one set)
    t.nwords = (c.n + 31) / 32;
    t.max_deg = 0;
    for (int i = 0; i < t.m; i++) t.max_deg = std::max(t.max_deg, row_ptr[i + 1] - row_ptr[i]);
    const int T = 64;   // one lane is one frame
    const size_t slab = (bytes_per_frame * T + 255) & ~(size_t) 255;
    t.slab_bytes = (int64_t) slab;
    // tiles: the resident wavefronts of the kernel, at most STREAMED_LAYERED_TILES_PER_CU per CU, as many as a quarter of the free
    // memory holds, and no more than tiles_env asks for (developer switch: tests force the reuse of a slab)
    int occ = 0;
    HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, 64, 0));
    int64_t per_cu = std::max(1, std::min(occ, STREAMED_LAYERED_TILES_PER_CU));
    if (const char *e = per_cu_env ? getenv(per_cu_env) : nullptr) {   // (developer switch: the sweep next to the constant)
        const long want = atol(e);
        if (want >= 1) per_cu = std::max<int64_t>(1, std::min<int64_t>(occ, want));
    }
    int64_t tiles = per_cu * d->cu_count;
    size_t free_b = 0, total_b = 0;
    HIP_OK(hipMemGetInfo(&free_b, &total_b));
    const int64_t fit = (int64_t) (free_b / 4 / slab);
    if (fit < 1) {
        set_error(what + ("not one tile of " + std::to_string(T)) + " frames (" + std::to_string(slab) +
                  " bytes) fits in a quarter of the device's free memory (" + std::to_string(free_b / 4) + " bytes)");
        return 3;
    }
    tiles = std::min(tiles, fit);
    if (const char *e = getenv(tiles_env)) {
        const long want = atol(e);
        if (want >= 1) tiles = std::min<int64_t>(tiles, want);
    }
    if (int rc = d->sl_ws.reserve((size_t) tiles * slab)) return rc;
    d->sl_tiles = (int) tiles;
    d->kernel[0] = kernel;
    d->kernel[1] = nullptr;
    d->L = 1;
    d->f64 = 0;
    d->block = 64;
    d->frames_per_block = T;
    d->lds_block = 0;
    d->grid_cap[0] = d->grid_cap[1] = (int) tiles;
    d->tab.lds_bytes_per_frame = 0;
    return 0;
}

// Streamed fixed-point layered min-sum (bp_streamed_q.hip): a quantized handle whose frames live in slabs of device memory, one
// per resident tile: 2 n + E bytes of a frame.
static int decoder_setup_streamq(acg_ldpc_decoder *d) {
    const size_t per_frame = 2 * (size_t) d->c.n + (size_t) d->c.E;
    if (int rc = decoder_setup_streamed_layered(d, bp_streamed_q_kernel_ptr(), per_frame, "streamed quantized layered min-sum: ", "ACG_STREAMQ_TILES", nullptr)) return rc;
    d->streamq = true;
    d->layered_wg = acg_ldpc_decoder::LayeredWg::q;   // a quantized handle: the integer entrances and the unfused Monte-Carlo route take it
    d->qargs = quant_args(d->quant);
    return 0;
}

// Streamed float layered BP (bp_streamed_layered.hip): sum-product or min-sum, fp32 posteriors and messages in slabs of device
// memory, one per resident tile: n + E words of a frame and the scratch of a wide sum-product check.
static int decoder_setup_streaml(acg_ldpc_decoder *d) {
    const int algo = d->p.algo == ACG_LDPC_BP_SUMPRODUCT ? 0 : 1;
    const size_t per_frame = 4 * ((size_t) d->c.n + (size_t) d->c.E + bp_streamed_layered_scratch_words(algo, d->c.max_cdeg));
    if (int rc = decoder_setup_streamed_layered(d, bp_streamed_layered_kernel_ptr(algo), per_frame, "streamed layered BP: ", "ACG_STREAML_TILES", "ACG_STREAML_PER_CU"))
        return rc;
    d->streaml = true;
    for (int k = 0; k < 2; k++) d->kernel_lio[k] = bp_streamed_layered_kernel_ptr(k, true);
    return 0;
}

// schedule = LAYERED: min-sum over conflict-free layers of checks with in-place posteriors (bp_layered.hip)
static int decoder_setup_layered(acg_ldpc_decoder *d) {
    const Code &c = d->c;
    // (sum-product with the layered schedule is the reference's check rule, bp.h:49-57, in another message order: a different
    // algorithm from BeliefPropagationDecoder — FER-level parity only — that the caller has to ask for explicitly)
    if (d->p.engine == ACG_LDPC_ENGINE_STREAMED || d->p.precision == ACG_LDPC_PREC_F64) {
        set_error("the layered schedule runs on the LDS-resident engine with fp32 posteriors (messages fp32, or fp16 with ACG_LDPC_PREC_F16)");
        return 3;
    }
    const bool lay_f16 = d->p.precision == ACG_LDPC_PREC_F16;
    // 256, 512, 1024: one workgroup per frame.  0 keeps the wavefront-group kernel for every code it accepts and falls
    // through to a workgroup of 1024 only where that kernel refuses for size (n >= 16000 here, a frame beyond LDS below)
    const int want_L = d->p.lanes_per_frame;
    // a check of degree 9 ... 32: the wide-check workgroup engine, whatever lanes_per_frame of its own (0 included) was asked for
    if (c.max_cdeg > 8) {
        if (c.max_cdeg > 32) {
            set_error("layered schedule: check degree above 32 is not supported");
            return 3;
        }
        if (want_L != 0 && want_L != 256 && want_L != 512 && want_L != 1024) {
            set_error("layered schedule: lanes_per_frame is chosen by the layering (pass 0), or 256, 512, 1024 for one workgroup per frame");
            return 3;
        }
        return decoder_setup_layered_wg(d, acg_ldpc_decoder::LayeredWg::wide, want_L);
    }
    if (want_L == 256 || want_L == 512 || want_L == 1024) return decoder_setup_layered_wg(d, acg_ldpc_decoder::LayeredWg::block, want_L);
    if (want_L == 0 && c.n >= 16000) return decoder_setup_layered_wg(d, acg_ldpc_decoder::LayeredWg::block, 1024);
    if (!bp_layered_build(c, d->llay)) return 3;
    const LayeredLayout &ll = d->llay;
    if (d->p.lanes_per_frame != 0 && d->p.lanes_per_frame != ll.G) {
        set_error("layered schedule: lanes_per_frame is chosen by the layering (pass 0), or 256, 512, 1024 for one workgroup per frame");
        return 3;
    }
    LayerTables &t = d->ltab;
    if (!(t.layer = upload_keep(ll.layer, d->dev_allocs))) return 10;
    if (ll.qc) {
        if (!(t.proto = upload_keep(ll.proto, d->dev_allocs))) return 10;
        t.pos = nullptr;
        std::vector<int32_t> packed(ll.proto.size() / 2 + 8, 0);   // (+8: the kernel's scalar loads may run a few words ahead)
        for (size_t k = 0; k + 1 < ll.proto.size(); k += 2) packed[k / 2] = (int32_t) (((uint32_t) (ll.proto[k] * ll.Z * 4) << 16) | (uint32_t) (ll.proto[k + 1] * 4));
        if (!(t.proto_packed = upload_keep(packed, d->dev_allocs))) return 10;
    } else {
        if (!(t.pos = upload_keep(ll.pos, d->dev_allocs))) return 10;
        t.proto = nullptr;
    }
    t.n_layers = ll.n_layers;
    t.Z = ll.Z;
    t.n = c.n;
    t.nwords = (c.n + 31) / 32;
    t.e_pad = ll.e_pad;
    t.p_words = (c.n + 1 + 3) & ~3;
    t.tab_lds_bytes = (int) (((size_t) ll.e_pad * 2 + 15) & ~(size_t) 15);
    // frame stride = G (mod 32) words: the lanes of the frames sharing a wavefront then fall into disjoint LDS banks
    t.r_words = lay_f16 ? (ll.e_pad + 1) / 2 : ll.e_pad;
    int words = t.p_words + t.r_words + t.nwords + 1;   // (+1: the Monte-Carlo instance's raw-channel error count)
    while (words % 32 != ll.G % 32) words++;
    t.lds_bytes_per_frame = words * 4;
    const int fpw = 64 / ll.G;
    const size_t per_wave = (size_t) t.lds_bytes_per_frame * fpw;
    // wavefronts per workgroup: the one that wastes the least LDS on the shared table while leaving >= 2 workgroups per CU
    int waves = 4;
    while (waves > 1 && (per_wave * waves + t.tab_lds_bytes) * 2 > 160 * 1024) waves >>= 1;
    {   // prefer the workgroup size that fits the most wavefronts per CU
        int best_w = waves, best_n = 0;
        for (int w : {4, 2, 1}) {
            const size_t blk = per_wave * w + t.tab_lds_bytes;
            if (blk > 160 * 1024) continue;
            const int nw = (int) ((160 * 1024) / blk) * w;
            if (nw > best_n) { best_n = nw; best_w = w; }
        }
        waves = best_w;
    }
    if (per_wave * waves + t.tab_lds_bytes > 160 * 1024) {
        if (want_L == 0) {   // the workgroup-per-frame engine keeps no table in LDS and splits a frame over 16 wavefronts
            d->ltab = LayerTables{};
            return decoder_setup_layered_wg(d, acg_ldpc_decoder::LayeredWg::block, 1024);
        }
        set_error("layered schedule: a frame (posteriors + messages) does not fit in LDS");
        return 3;
    }
    d->layered = true;
    d->L = ll.G;
    d->f64 = 0;
    d->block = waves * 64;
    d->frames_per_block = waves * fpw;
    d->lds_block = per_wave * waves + t.tab_lds_bytes;
    // positions by arithmetic in the hot loop when the block columns' byte offsets fit the packed word (n * 4 < 65536 holds: n < 16000)
    // ACG_LAY_ARITH=1 (developer A/B): compute the positions of a quasi-cyclic H in the hot loop instead of reading the table
    const int lay_algo = d->p.algo == ACG_LDPC_BP_MINSUM ? 1 : 0;
    const bool qc_arith = ll.qc && ll.G == 20 && !lay_f16 && lay_algo == 1 && getenv("ACG_LAY_ARITH") != nullptr;
    for (int mc = 0; mc < 2; mc++) {
        const void *kp = bp_layered_kernel_ptr(ll.G, waves, qc_arith && !mc, lay_f16, lay_algo, mc != 0);
        if (!kp) {
            set_error("no layered kernel instance for this group width");
            return 3;
        }
        if (int rc = bind_kernel(d, mc, kp)) return rc;
    }
    d->tab.lds_bytes_per_frame = t.lds_bytes_per_frame;
    return 0;
}

static int decoder_setup_bp(acg_ldpc_decoder *d) {
    const Code &c = d->c;
    if (d->p.schedule == ACG_LDPC_SCHEDULE_LAYERED) return decoder_setup_layered(d);
    if (d->p.schedule != ACG_LDPC_SCHEDULE_FLOODING) {
        set_error("unknown schedule");
        return 1;
    }
    if (d->p.engine != ACG_LDPC_ENGINE_AUTO && d->p.engine != ACG_LDPC_ENGINE_FUSED &&
        d->p.engine != ACG_LDPC_ENGINE_STREAMED) {
        set_error("unknown engine");
        return 1;
    }
    const bool pair = (d->p.precision == ACG_LDPC_PREC_F16);
    if (pair) {
        if (d->p.algo != ACG_LDPC_BP_MINSUM || d->p.engine == ACG_LDPC_ENGINE_STREAMED) {
            set_error("ACG_LDPC_PREC_F16 exists for the fused min-sum decoder only (the reference's sum-product needs fp32/fp64 messages)");
            return 3;
        }
        if (c.max_cdeg > 8 || c.max_vdeg > 4 || c.n > 12 * 1024) {
            set_error("ACG_LDPC_PREC_F16 needs check degree <= 8, variable degree <= 4 and n <= 12288");
            return 3;
        }
    }
    if (d->p.engine == ACG_LDPC_ENGINE_STREAMED) return decoder_setup_streamed(d);
    d->maxd = std::max(c.max_cdeg, c.max_vdeg);
    if (!pair) {
        // does one frame fit in LDS?  (message words incl. padding at the smallest group size + LLRs)
        const size_t ts0 = (d->p.precision == ACG_LDPC_PREC_F64) ? 8 : 4;
        // (LLRs sit in registers for up to 12 passes of the group size, i.e. n <= 12288 in workgroup mode)
        const size_t approx = ((size_t) c.E + 64 + ((size_t) c.n > 12 * 1024 ? (size_t) c.n : 0)) * ts0;
        const bool fits = d->maxd <= 32 && approx <= 150 * 1024 && (size_t) c.E + 16 * (size_t) d->maxd < 60000;
        if (!fits) {
            if (d->p.engine == ACG_LDPC_ENGINE_FUSED) {
                set_error("code too large (or node degree > 32) for the fused LDS engine");
                return 3;
            }
            return decoder_setup_streamed(d);
        }
    }
    d->f64 = (d->p.precision == ACG_LDPC_PREC_F64) ? 1 : 0;
    int L = d->p.lanes_per_frame;
    if (L != 0 && L != 16 && L != 32 && L != 64 && L != 256 && L != 1024) {
        set_error("lanes_per_frame must be 0, 16, 32, 64 (wavefront groups) or 256, 1024 (one workgroup per frame)");
        return 3;
    }
    // Workgroup-per-frame mode (bp_block.hip) for codes whose message array leaves room for only a few
    // wavefront-sized frames per CU: the same LDS then feeds 4-16x as many wavefronts.
    bool blockmode = (L == 256 || L == 1024);
    if (pair) {  // always one workgroup per frame pair: 256 threads when the variables fit in 12 passes of them, else 1024
        if (L != 0 && L != 256 && L != 1024) {
            set_error("ACG_LDPC_PREC_F16: lanes_per_frame must be 0, 256 or 1024");
            return 3;
        }
        if (L == 0) L = (c.n <= 12 * 256) ? 256 : 1024;
        blockmode = true;
    }
    if (!pair && L == 0) {
        L = bp_default_lanes(c, d->f64 != 0);
        if (L == 0) return 3;
        blockmode = L >= 256;
    }
    if (blockmode && (d->maxd > 8 || c.n > 12 * L)) {
        set_error("workgroup-per-frame BP needs node degree <= 8 and n <= 12 * lanes_per_frame");
        return 3;
    }
    d->L = L;
    if (!bp_layout_build(c, L, d->lay)) return 3;
    // fp32 sum-product wave-group kernels with register LLRs: degree-1 variables absorbed into their checks
    // (BpLayout::n_apass, BpPass::check_abs); taken when the absorbed layout runs that kernel variant
    if (!blockmode && !pair && !d->f64 && d->p.algo != ACG_LDPC_BP_MINSUM && d->maxd <= 8 && getenv("ACG_BP_NO_ABSORB") == nullptr) {
        if (!bp_layout_absorb(c, L, d->lay)) return 3;
    }
    BpLayout &lay = d->lay;
    const int nwords = (c.n + 31) / 32;
    // the MC path stages n symbols in the message array before clearing it
    if (lay.a_words < ((c.n + 3) & ~3)) lay.a_words = (c.n + 3) & ~3;
    const size_t ts = d->f64 ? 8 : 4;
    // wavefront groups: LLRs in registers or LDS, the index table in LDS or global, the frame's LDS bytes and the wavefronts per
    // workgroup are bp_wave_plan's decisions (code.cpp); a workgroup per frame keeps the LLRs in registers
    BpWavePlan wp;
    if (!blockmode) wp = bp_wave_plan(c, lay, d->f64 != 0);
    const bool llr_regs = blockmode || wp.llr_regs;
    const int llr_words = blockmode ? 0 : wp.llr_words;
    size_t per_frame = wp.per_frame;
    if (blockmode) {
        per_frame = (size_t) lay.a_words * ts + (size_t) nwords * 4;
        if (pair) per_frame = (size_t) lay.a_words * 4 + 2 * (size_t) nwords * 4;  // one 32-bit word per edge for TWO frames
        per_frame = (per_frame + 15) & ~(size_t) 15;
    }

    BpTables &t = d->tab;
    std::vector<int32_t> c_pass(2 * (size_t) lay.n_cpass), v_pass(2 * (size_t) lay.n_vpass);
    for (int p = 0; p < lay.n_cpass; p++) {
        c_pass[2 * p] = lay.c_maxdeg[p];
        c_pass[2 * p + 1] = lay.c_off[p];
    }
    for (int p = 0; p < lay.n_vpass; p++) {
        v_pass[2 * p] = lay.v_maxdeg[p];
        v_pass[2 * p + 1] = lay.v_idx_off[p];
    }
    std::vector<int32_t> c_cnt(34, 0), v_cnt(34, 0);
    for (size_t i = 0; i < lay.c_cnt_ge.size() && i < 34; i++) c_cnt[i] = lay.c_cnt_ge[i];
    for (size_t i = 0; i < lay.v_cnt_ge.size() && i < 34; i++) v_cnt[i] = lay.v_cnt_ge[i];
#define UP32(vec, field) \
    if (!(t.field = upload_keep(vec, d->dev_allocs))) return 10;
    UP32(c_pass, c_pass)
    UP32(c_cnt, c_cnt_ge)
    UP32(v_pass, v_pass)
    UP32(v_cnt, v_cnt_ge)
    UP32(lay.v_var, v_var)
    if (lay.n_apass > 0) {
        UP32(lay.a_var, a_var)
    }
    UP32(lay.v_apos, v_apos)
#undef UP32
    t.v_apos_len = lay.v_apos_len;
    // the variable-side index table is read by every wave in every iteration: keep a block-shared
    // copy in LDS unless it is large (then it is read through L1/L2)
    bool idxlds = wp.idxlds;
    if (blockmode) idxlds = (size_t) lay.v_apos_len * 2 <= 32 * 1024 &&
                            (((size_t) lay.v_apos_len * 2 + 15) & ~(size_t) 15) + per_frame <= 158 * 1024;
    t.idx_lds_bytes = idxlds ? (int) (((size_t) lay.v_apos_len * 2 + 15) & ~(size_t) 15) : 0;
    t.n_cpass = lay.n_cpass;
    t.n_vpass = lay.n_vpass;
    t.a_words = lay.a_words;
    t.zero_pos = lay.zero_pos;
    t.m = c.m;
    t.n = c.n;
    t.nwords = nwords;
    t.llr_words = llr_words;
    t.lds_bytes_per_frame = (int) per_frame;
    t.n_apass = lay.n_apass;

    if (blockmode) {
        if (per_frame + t.idx_lds_bytes > 160 * 1024) {
            if (d->p.engine == ACG_LDPC_ENGINE_AUTO && d->p.lanes_per_frame == 0) {
                d->dev_allocs.clear();
                return decoder_setup_streamed(d);
            }
            set_error("frame state does not fit in LDS (160 KiB per CU)");
            return 3;
        }
        d->block = L;
        d->frames_per_block = 1;
        d->lds_block = per_frame + t.idx_lds_bytes;
        if (pair) {
            d->pair = true;
            d->frames_per_block = 2;
            d->lds_block = per_frame;
            t.idx_lds_bytes = 0;
            // regular code (one check degree, one variable degree): the instance with fully unrolled passes
            const void *kp = bp_pair_kernel_ptr(L, is_regular(c));
            if (!kp) {
                set_error("no paired-frame kernel instance for this configuration");
                return 3;
            }
            if (int rc = bind_kernel(d, 0, kp)) return rc;
            d->grid_cap[1] = d->grid_cap[0];  // (kernel[1] stays null: Monte-Carlo runs go AWGN kernel -> decode -> classify kernel)
            return 0;
        }
        const int algo_b = (d->p.algo == ACG_LDPC_BP_MINSUM) ? 1 : 0;
        for (int mc = 0; mc < 2; mc++) {
            // index table too large for LDS and variable degree <= 4: keep it in registers (decode kernel only)
            const bool idxreg = !idxlds && c.max_vdeg <= 4 && lay.n_vpass <= 12 && getenv("ACG_BP_NO_IDXREG") == nullptr;
            // regular code (one check degree <= 8, one variable degree <= 4): the instance without the paths for anything else
            const bool regular_b = idxreg && c.max_cdeg <= 8 && c.max_vdeg <= 4 && getenv("ACG_BP_NO_REGULAR") == nullptr && is_regular(c);
            const void *kp = bp_block_kernel_ptr(algo_b, d->f64, L, mc != 0, idxlds, idxreg, regular_b);
            if (mc == 0) {
                d->blk_idxlds = idxlds;
                d->blk_idxreg = idxreg;
            }
            if (!kp) {
                set_error("no workgroup-per-frame kernel instance for this configuration");
                return 3;
            }
            if (int rc = bind_kernel(d, mc, kp)) return rc;
        }
        return 0;
    }
    const int fpw = 64 / L;
    const int waves = wp.waves;
    if (waves == 0) {
        if (d->p.engine == ACG_LDPC_ENGINE_AUTO) {
            d->dev_allocs.clear();
            return decoder_setup_streamed(d);
        }
        set_error("frame state does not fit in LDS (160 KiB per CU)");
        return 3;
    }
    d->block = waves * 64;
    d->frames_per_block = waves * fpw;
    d->lds_block = per_frame * fpw * waves + t.idx_lds_bytes;
    const int algo = (d->p.algo == ACG_LDPC_BP_MINSUM) ? 1 : 0;
    // fixed-work decoders: the instances with the phi fast path (BpCore::SATSKIP; fp32 sum-product, degree <= 8, register
    // LLRs); ACG_BP_NO_SATSKIP=1 keeps the plain instances (A/B runs)
    const bool sat = !d->p.early_exit && getenv("ACG_BP_NO_SATSKIP") == nullptr;
    // the phi memo of the absorbed check passes in those instances (BpPass::phi_c); ACG_BP_NO_PHIMEMO=1 turns it off (A/B runs)
    d->phi_memo = sat && getenv("ACG_BP_NO_PHIMEMO") == nullptr;
    // a latched frame of those instances stops sweeping once its state recurs (bp_fused_body, FREEZE): same outputs, fewer
    // sweeps executed; ACG_BP_NO_FREEZE=1 runs them all (A/B runs).  The cadence is in sweeps behind the latch: the first
    // snapshot, then a compare (and a new snapshot) every `period` (tools/freeze_census.cpp, profiles/r09_freeze_summary.md).
    d->freeze = sat && algo == 0 && !d->f64 && d->maxd <= 8 && idxlds && llr_regs && getenv("ACG_BP_NO_FREEZE") == nullptr;
    // a detection loads the snapshot and compares only where the lanes' checksums of their words allow a recurrence, and
    // otherwise only writes the new one; ACG_BP_FREEZE_NO_GATE=1 loads and compares at every detection behind a group's first
    d->freeze_gate = getenv("ACG_BP_FREEZE_NO_GATE") == nullptr;
    // the instances whose all-latched wavefronts evaluate one of phi's two series where that gives phi's bits (bp_fused_body,
    // SPLIT; split::).  Same results; on H05 3.2 % faster at -2 dB, 4.5 % at +2 dB, level at -3 dB
    // (profiles/r17_phisplit_summary.md).  ACG_BP_NO_PHISPLIT=1 keeps the instances without it (bit-for-bit comparison, A/B
    // runs).  Instances with the freeze path only: `fz` is what tells the kernel that a group has latched.
    // (build-time instances, and the generic ones at 16 and 32 lanes; the Monte-Carlo launches of a handle run without it)
    d->phi_split = d->freeze && getenv("ACG_BP_NO_PHISPLIT") == nullptr;
    // measured best on the headline among 3 ... 12 / 1 ... 4 (profiles/r09_freeze_summary.md), and again with the gate among
    // 1 ... 12 / 1 ... 4 (profiles/r12_freeze_gate_summary.md)
    d->freeze_first = 10;
    d->freeze_period = 1;
    if (const char *e = getenv("ACG_BP_FREEZE_CADENCE")) {  // "first,period" (tuning runs)
        int f = 0, q = 0;
        if (sscanf(e, "%d,%d", &f, &q) == 2 && f >= 1 && q >= 1 && f < (1 << 12) && q < (1 << 12)) d->freeze_first = f, d->freeze_period = q;
    }
    d->freeze_slot_words = (size_t) lay.a_words + (size_t) BP_MAX_APASS * L;
    for (int mc = 0; mc < 2; mc++) {
        const int variant = wp.variant;
        d->variant = variant;
        const void *kp = bp_kernel_ptr(algo, d->f64, d->maxd, L, mc != 0, variant, sat, d->phi_split);
        if (!kp) {
            set_error("no kernel instance for this configuration");
            return 3;
        }
        // the build-time instance with this layout's pass structure constant, where the library holds one (bp_inst_spec.hip:
        // the fixed-work fp32 sum-product instances only; equal signature, whatever the matrix); ACG_BP_NO_SPEC=1 keeps
        // the generic instance (A/B runs)
        if (sat && algo == 0 && !d->f64 && d->maxd <= 8 && variant == 2 && getenv("ACG_BP_NO_SPEC") == nullptr) {
            const char *name = nullptr, *rows = nullptr, *srows = nullptr;
            if (const void *ks = bp_spec_kernel_ptr(lay, mc != 0, &name, &rows, d->phi_split, &srows)) {
                kp = ks;
                d->spec = name;
                d->spec_sat_rows = rows;
                d->spec_split_rows = srows;
            }
        }
        if (int rc = bind_kernel(d, mc, kp)) return rc;
    }
    if (!d->spec && L > 32) d->phi_split = false;  // (the generic instance at 64 lanes has none)
    return 0;
}

int acg::acg_ldpc_decoder_create_impl(const acg_ldpc_code *code, const acg_ldpc_params *params, acg_ldpc_decoder **out,
                                      hipStream_t on_stream, const acg_ldpc_quant *quant, bool q_streamed, bool l_streamed) {
    if (!code || !params || !out) {
        set_error("null argument");
        return 1;
    }
    if (params->max_iter < 0) {
        set_error("max_iter must be >= 0");
        return 1;
    }
    if (quant) {   // (host-only refusals first: they need no device)
        if (int rc = quant_check(quant)) return rc;
        if (int rc = q_streamed ? streamq_params_check(*params) : quant_params_check(*params)) return rc;
        if (!q_streamed && code->c.max_cdeg > 32) {
            set_error("quantized layered min-sum: check degree above 32 is not supported");
            return 3;
        }
    }
    if (l_streamed) {
        if (quant) {
            set_error("internal: the streamed float layered engine takes no quantiser");
            return 11;
        }
        if (int rc = streaml_params_check(*params)) return rc;
    }
    if (!quant && params->algo == ACG_LDPC_OSD) {
        if (int rc = osd_params_check(*params, code->c)) return rc;
        if (osd_lds_bytes(code->c.n, code->c.m) > 160 * 1024) {
            set_error("OSD: a frame (working matrix of " + std::to_string(code->c.n) + " columns x " + std::to_string((code->c.m + 31) / 32) +
                      " words, keys, pivots, word) does not fit in LDS");
            return 3;
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available: libacg_ldpc_hip has no CPU fallback");
        return 20;
    }
    DecoderPtr own(new acg_ldpc_decoder());
    acg_ldpc_decoder *d = own.get();
    d->c = code->c;
    d->p = *params;
    int dev = params->device;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    }
    if (dev >= ndev) {
        set_error("device ordinal out of range");
        return 1;
    }
    d->device = dev;
    int rc = 0;
    do {
        if (hipSetDevice(dev) != hipSuccess) { set_error("hipSetDevice failed"); rc = 10; break; }
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess) { set_error("hipGetDeviceProperties failed"); rc = 10; break; }
        d->cu_count = prop.multiProcessorCount;
        if (on_stream) {
            d->stream = on_stream;
            d->own_stream = false;
        } else if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) { set_error("hipStreamCreate failed"); rc = 10; break; }
        if (d->counters.reserve(sizeof(unsigned long long) * MC_NCOUNTERS) ||
            d->work_ring.reserve(sizeof(unsigned long long) * acg_ldpc_decoder::WORK_RING)) { set_error("hipMalloc failed"); rc = 10; break; }
        {
            bool evok = true;
            for (int k = 0; k < acg_ldpc_decoder::WORK_RING; k++)
                evok = evok && hipEventCreate(&d->ring_ev0[k]) == hipSuccess && hipEventCreate(&d->ring_ev[k]) == hipSuccess;
            if (!evok) { set_error("hipEventCreate failed"); rc = 10; break; }
        }
        if (quant) {
            d->name = "QMS";
            d->quant = *quant;
            rc = q_streamed ? decoder_setup_streamq(d) : decoder_setup_layered_wg(d, acg_ldpc_decoder::LayeredWg::q, d->p.lanes_per_frame);
        } else if (l_streamed) {
            d->name = params->algo == ACG_LDPC_BP_SUMPRODUCT ? "BP" : "MS";
            rc = decoder_setup_streaml(d);
        } else if (params->algo == ACG_LDPC_QPADMM) {
            d->name = "QP-ADMM";  // qp_admm.h:189
            std::string err;
            d->admm.reset(admm_device_create(d->c, d->p, d->cu_count, err));
            if (!d->admm) { set_error(err); rc = 3; break; }
        } else if (params->algo == ACG_LDPC_BP_SUMPRODUCT || params->algo == ACG_LDPC_BP_MINSUM) {
            d->name = params->algo == ACG_LDPC_BP_SUMPRODUCT ? "BP" : "MS";  // bp.h:218
            rc = decoder_setup_bp(d);
        } else if (params->algo == ACG_LDPC_OSD) {
            d->name = "OSD";
            rc = decoder_setup_osd(d);
        } else {
            set_error("unknown algo");
            rc = 1;
        }
    } while (0);
    if (rc) return rc;
    *out = own.release();
    return 0;
}

extern "C" {

int acg_ldpc_decoder_create(const acg_ldpc_code *code, const acg_ldpc_params *params, acg_ldpc_decoder **out) {
    return guarded([&] { return acg_ldpc_decoder_create_impl(code, params, out); });
}

void acg_ldpc_quant_default(acg_ldpc_quant *q) {
    if (!q) return;
    q->llr_step = 0.5;
    q->ch_bits = 6;
    q->msg_bits = 6;
    q->post_bits = 8;
    q->scale_num = 1;
    q->scale_shift = 0;
    q->offset = 1;
}

int acg_ldpc_quant_check(const acg_ldpc_quant *q) {
    return guarded([&] { return quant_check(q); });
}

int acg_ldpc_decoder_create_quantized(const acg_ldpc_code *code, const acg_ldpc_params *params, const acg_ldpc_quant *q,
                                      acg_ldpc_decoder **out) {
    return guarded([&] {
        if (!q) {
            set_error("null argument");
            return 1;
        }
        return acg_ldpc_decoder_create_impl(code, params, out, nullptr, q);
    });
}

int acg_ldpc_decoder_create_quantized_streamed(const acg_ldpc_code *code, const acg_ldpc_params *params, const acg_ldpc_quant *q,
                                               acg_ldpc_decoder **out) {
    return guarded([&] {
        if (!q) {
            set_error("null argument");
            return 1;
        }
        return acg_ldpc_decoder_create_impl(code, params, out, nullptr, q, true);
    });
}

int acg_ldpc_decoder_create_layered_streamed(const acg_ldpc_code *code, const acg_ldpc_params *params, acg_ldpc_decoder **out) {
    return guarded([&] { return acg_ldpc_decoder_create_impl(code, params, out, nullptr, nullptr, false, true); });
}

void acg_ldpc_decoder_destroy(acg_ldpc_decoder *d) {
    if (!d) return;
    (void) hipSetDevice(d->device);
    if (d->stream) (void) hipStreamSynchronize(d->stream);
    // launches of this handle that are still in flight on CALLER streams (acg_ldpc_decode_batch_dev is asynchronous): every
    // launch recorded the stop event of its ring slot on its own stream — wait for them before the tables go (a handle can be
    // destroyed by the LRU of a host mirror while the caller's stream is still busy)
    for (int k = 0; k < acg_ldpc_decoder::WORK_RING; k++)
        if (d->ring_used[k] && d->ring_ev[k]) (void) hipEventSynchronize(d->ring_ev[k]);
    // (the device and pinned buffers belong to the members of the handle: `delete d` below releases them)
    for (int k = 0; k < acg_ldpc_decoder::WORK_RING; k++) {
        if (d->ring_ev0[k]) (void) hipEventDestroy(d->ring_ev0[k]);
        if (d->ring_ev[k]) (void) hipEventDestroy(d->ring_ev[k]);
    }
    if (d->stream && d->own_stream) (void) hipStreamDestroy(d->stream);
    delete d;
}

const char *acg_ldpc_decoder_name(const acg_ldpc_decoder *d) { return d->name.c_str(); }

void acg_ldpc_decoder_layout(const acg_ldpc_decoder *d, int32_t *lds_bytes_per_frame, int32_t *lanes_per_frame,
                             int32_t *frames_per_block, int32_t *grid_blocks) {
    if (d->admm) {
        admm_device_layout(d->admm.get(), lds_bytes_per_frame, lanes_per_frame, frames_per_block, grid_blocks);
        return;
    }
    if (lds_bytes_per_frame) *lds_bytes_per_frame = d->streamed || d->streamq || d->streaml ? 0 : d->tab.lds_bytes_per_frame;
    if (lanes_per_frame) *lanes_per_frame = d->L;
    if (frames_per_block) *frames_per_block = d->frames_per_block;
    if (grid_blocks) *grid_blocks = d->grid_cap[0];
}

// one line naming what this handle launches (diagnostics: bench.py records it next to every timed leg)
static std::string describe(const acg_ldpc_decoder *d) {
    char b[512];
    const char *algo = d->p.algo == ACG_LDPC_QPADMM ? "qpadmm" : (d->p.algo == ACG_LDPC_BP_MINSUM ? "minsum" : "sum-product");
    int slabs = 0, f32 = 0;
    int64_t slab = 0;
    if (d->osd) {
        snprintf(b, sizeof b, "osd engine=fused kernel=osd_kernel lanes_per_frame=%d block=%d frames_per_block=1 order=%d rank=%d lds_block=%zu "
                               "grid_cap=%d workgroups_per_cu=%d",
                 d->L, d->block, d->oargs.order, d->oargs.rank, d->lds_block, d->grid_cap[0], d->grid_cap[0] / std::max(d->cu_count, 1));
    } else if (d->admm && admm_device_streamed(d->admm.get(), &slabs, &slab, &f32)) {
        snprintf(b, sizeof b, "%s engine=streamed kernel=admm_streamed_kernel<%s> f64=%d slab_bytes=%lld slabs=%d workspace_bytes=%lld "
                               "workspace=hipMalloc mc_grid=per-point",
                 algo, f32 ? "float" : "double", f32 ? 0 : 1, (long long) slab, slabs, (long long) slab * slabs);
    } else if (d->admm) {
        int lds = 0, L = 0, fpb = 0, grid = 0;
        admm_device_layout(d->admm.get(), &lds, &L, &fpb, &grid);
        snprintf(b, sizeof b, "%s engine=lds lanes_per_frame=%d frames_per_block=%d lds_bytes_per_frame=%d grid_cap=%d mc_grid=%s", algo, L, fpb, lds, grid,
                 admm_device_has_grid_kernel(d->admm.get()) ? "single-launch" : "per-point");
    } else if (d->streamed) {
        const size_t slab = (size_t) d->stab.ws_words_per_wave * 4;
        snprintf(b, sizeof b, "%s engine=streamed kernel=%s%s f64=%d slab_bytes=%zu slabs=%d workspace_bytes=%zu workspace_base=%p "
                               "workgroups_per_cu=%d schedule=%s",
                 algo, d->sring ? "bp_streamed_ring_kernel" : "bp_streamed_kernel", d->sring ? (d->sring_nt ? "<NT>" : "<default-policy>") : "",
                 d->f64, slab, d->sgrid, slab * (size_t) d->sgrid, d->sws.va, d->sring ? d->sring_per_cu : 2,
                 !d->sws.plain ? "flooding workspace=mapped-chunks" : "flooding workspace=hipMalloc");
        if (!d->sws_probe_ms.empty()) {
            std::string t = b;
            t += " workspace_spread=" + std::to_string(d->sws_spread) + " workspace_probe_ms=";
            for (size_t i = 0; i < d->sws_probe_ms.size(); i++) {
                char q[32];
                snprintf(q, sizeof q, "%s%.2f", i ? "/" : "", d->sws_probe_ms[i]);
                t += q;
            }
            return t;
        }
    } else if (d->streaml) {
        const size_t scratch = bp_streamed_layered_scratch_words(d->p.algo == ACG_LDPC_BP_SUMPRODUCT ? 0 : 1, d->sltab.max_deg);
        snprintf(b, sizeof b, "%s engine=streamed kernel=bp_streamed_layered_kernel<%s> schedule=layered messages=fp32 posteriors=fp32 T=%d tiles=%d "
                               "state_bytes_per_frame=%zu scratch_bytes_per_frame=%zu wide_mag=%s slab_bytes=%lld workspace_bytes=%zu "
                               "workspace=hipMalloc sets=%d checks=%d max_check_degree=%d io=llr,post",
                 algo, algo, d->frames_per_block, d->sl_tiles, 4 * ((size_t) d->c.n + (size_t) d->sltab.E), 4 * scratch,
                 scratch == 0 ? "none" : (bp_streamed_layered_stores_mag() ? "stored" : "recomputed"), (long long) d->sltab.slab_bytes,
                 (size_t) d->sl_tiles * (size_t) d->sltab.slab_bytes, d->lblay.n_sets, d->sltab.m, d->sltab.max_deg);
    } else if (d->streamq) {
        const acg_ldpc_quant &q = d->quant;
        snprintf(b, sizeof b, "%s engine=streamed kernel=bp_streamed_q_kernel schedule=layered T=%d tiles=%d state_bytes_per_frame=%zu "
                               "slab_bytes=%lld workspace_bytes=%zu workspace=hipMalloc sets=%d checks=%d messages=int8 posteriors=int16 "
                               "quant=llr_step:%.9g,ch_bits:%d,msg_bits:%d,post_bits:%d,scale_num:%d,scale_shift:%d,offset:%d mc_quants=refused",
                 algo, d->frames_per_block, d->sl_tiles, 2 * (size_t) d->c.n + (size_t) d->sltab.E, (long long) d->sltab.slab_bytes,
                 (size_t) d->sl_tiles * (size_t) d->sltab.slab_bytes, d->lblay.n_sets, d->sltab.m, q.llr_step, q.ch_bits, q.msg_bits, q.post_bits,
                 q.scale_num, q.scale_shift, q.offset);
    } else if (d->layered_wg == acg_ldpc_decoder::LayeredWg::q) {
        const acg_ldpc_quant &q = d->quant;
        snprintf(b, sizeof b, "%s engine=fused kernel=bp_layered_q_kernel lanes_per_frame=%d f64=0 block=%d frames_per_block=1 lds_block=%zu "
                               "grid_cap=%d sets=%d steps=%d largest_set=%d schedule=layered messages=int8 posteriors=int16 "
                               "quant=llr_step:%.9g,ch_bits:%d,msg_bits:%d,post_bits:%d,scale_num:%d,scale_shift:%d,offset:%d mc_quants=single-launch",
                 algo, d->L, d->block, d->lds_block, d->grid_cap[0], d->lbtab.n_sets, d->lbtab.n_steps, d->lblay.width, q.llr_step, q.ch_bits, q.msg_bits,
                 q.post_bits, q.scale_num, q.scale_shift, q.offset);
    } else if (d->layered_wg != acg_ldpc_decoder::LayeredWg::none) {
        snprintf(b, sizeof b, "%s engine=fused kernel=%s lanes_per_frame=%d f64=0 block=%d frames_per_block=1 lds_block=%zu "
                               "grid_cap=%d sets=%d steps=%d largest_set=%d schedule=layered messages=%s",
                 algo, d->layered_wg == acg_ldpc_decoder::LayeredWg::wide ? "bp_layered_wide_kernel" : "bp_layered_block_kernel", d->L, d->block, d->lds_block, d->grid_cap[0], d->lbtab.n_sets, d->lbtab.n_steps, d->lblay.width,
                 d->p.precision == ACG_LDPC_PREC_F16 ? "fp16" : "fp32");
    } else {
        snprintf(b, sizeof b, "%s engine=fused kernel=%s lanes_per_frame=%d f64=%d block=%d frames_per_block=%d lds_block=%zu grid_cap=%d "
                               "idx_lds=%d idx_reg=%d schedule=%s",
                 algo, d->layered ? "bp_layered_kernel" : (d->pair ? "bp_pair_kernel" : (d->variant < 0 ? "bp_block_kernel" : "bp_fused_kernel")), d->L, d->f64, d->block,
                 d->frames_per_block, d->lds_block, d->grid_cap[0], d->variant < 0 ? (int) d->blk_idxlds : (d->variant > 0), (int) d->blk_idxreg,
                 d->p.schedule == ACG_LDPC_SCHEDULE_LAYERED ? (d->p.precision == ACG_LDPC_PREC_F16 ? "layered messages=fp16" : "layered messages=fp32")
                                                            : "flooding");
        if (d->variant >= 0 && !d->layered && !d->pair) {
            std::string t = b;
            if (!d->p.early_exit) {
                // fixed-work decoders: whether latched frames whose state recurs stop sweeping, and on which cadence
                if (d->freeze) t += " freeze=1 freeze_cadence=" + std::to_string(d->freeze_first) + "," + std::to_string(d->freeze_period) +
                                        " freeze_gate=" + (d->freeze_gate ? "1" : "0");
                else t += " freeze=0";
                t += d->phi_split ? " phi_split=1" : " phi_split=0";
            }
            // the build-time instance with the code's pass structure constant that this handle runs (bp_inst_spec.hip), or 0; in
            // front of it the rows of that instance that keep their phi fast-path test
            if (d->spec && d->phi_split && d->spec_split_rows) t += std::string(" split_rows=") + d->spec_split_rows;
            if (d->spec && d->spec_sat_rows) t += std::string(" sat_rows=") + d->spec_sat_rows;
            t += std::string(" spec=") + (d->spec ? d->spec : "0");
            return t;
        }
    }
    return b;
}

int32_t acg_ldpc_decoder_describe(const acg_ldpc_decoder *d, char *buf, int32_t cap) {
    if (!d) return 0;
    return copy_text(describe(d), buf, cap);
}

}  // extern "C"
