// Streamed ("HBM") QP-ADMM engine — DecodeQPADMM (algo/qp_admm.h:104-178) for codes whose per-frame state does not fit
// in LDS (e.g. the 5000 x 10000 (3,6)-regular stress code of BASELINE configs[4]: 80 000 constraint rows, 25 000
// variables), and, when forced (ACG_LDPC_ENGINE_STREAMED), for any other code.
//
// Mapping of the streamed BP engine (bp_streamed.hip): ONE LANE = ONE FRAME.  A workgroup of 4 wavefronts owns a tile of
// 64 frames and a private slab of HBM, every array laid out [row][64]:
//     W[C][64]      w_j = r_j - yl_j, one word per constraint row (z_j and yl_j are its positive and negative part,
//                   exactly — see the header of admm_kernels.hip)
//     V[n_var][64]  v
//     Q[n][64]      q_i = llr(y_i) of the original variables (auxiliaries have q = 0, qp_admm.h:24), copied in once per
//                   tile because y is stored frame-major
// so every wave instruction moves whole lines, the graph indices are wave-uniform (scalar loads) and no lane needs
// another lane's data.  One sweep (qp_admm.h:132-163):
//   1. v-update: the waves split the variables; B = q_i + alpha/2, then B += cf * (yl_j + mu*(z_j - b_j)) over A[i] in
//      construction order, v_i = clamp(B * inv_coef_i, 0, 1).  Barrier.
//   2. row update: the waves split the constraint groups; r_j = b_j - sum cf * v with the members in ascending variable
//      id, the new w, and each lane's partial residual sum.  Barrier, the four partial sums combined through LDS.
// Per frame and sweep that reads nnz + n + n_var (phase 1; Q only for original variables) and sum of group sizes + C
// words (phase 2) and writes n_var + C words: (nnz + n + n_var + sum of group sizes + 2C) * b bytes.
// Same arithmetic and rounding order as the LDS kernels (this file is built with -ffp-contract=off); the residual is
// reduced in another order (per wavefront, then over the four wavefronts), as the LDS kernels do: it is compared with
// eps_stop and never fed back.  A lane whose residual drops below eps_stop stops changing its state; its outputs are
// written from that frozen state when the tile ends (early exit: all 64 lanes done; fixed work: max_iter sweeps).
// No node-degree limit: list lengths are loop bounds read at run time.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <string>

#include "device_mem.hpp"
#include "launchers.hpp"

namespace acg {

namespace {

template <typename T>
__device__ __forceinline__ T sload_c(const T *p, int64_t i) {
    return ((const T __attribute__((address_space(4))) *) p)[i];  // wave-uniform table: scalar load
}

constexpr int ADMM_ST_WAVES = 4;

}  // namespace

struct AdmmStreamDev {
    const int32_t *var_ptr;   // [n_var+1]
    const uint32_t *var_ent;  // first row | wpos << 28 | type << 30 (AdmmStreamTables)
    const uint32_t *grp;      // [n_grp][4]
    const void *inv_coef;     // [n_var] T
    int32_t n, n_var, n_con, n_grp, nwords;
    int64_t slab_bytes;
};

template <typename T>
__global__ void __launch_bounds__(ADMM_ST_WAVES * 64) admm_streamed_kernel(const AdmmStreamDev t, const DecodeArgs a, const T alpha,
                                                                           const T mu, const T eps_stop, unsigned char *ws) {
    __shared__ T part[ADMM_ST_WAVES][64];
    __shared__ unsigned long long tile_lds;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    T *__restrict__ W = reinterpret_cast<T *>(ws + (size_t) blockIdx.x * (size_t) t.slab_bytes);
    T *__restrict__ V = W + (size_t) t.n_con * 64;
    T *__restrict__ Q = V + (size_t) t.n_var * 64;
    const T *inv_coef = reinterpret_cast<const T *>(t.inv_coef);
    const T half_alpha = alpha / 2;
    const int64_t n_tiles = (a.frames + 63) / 64;

    for (;;) {
        // dynamic tile hand-out (as bp_streamed_kernel): a launch with more tiles than slabs loops
        __syncthreads();
        if (threadIdx.x == 0) tile_lds = atomicAdd(a.work_counter, 1ull);
        __syncthreads();
        const int64_t tile = (int64_t) tile_lds;
        if (tile >= n_tiles) break;
        const int64_t frame = tile * 64 + lane;
        const bool valid = frame < a.frames;
        // ---- channel term (CalculateCoef, algo/algo.h:13-20) and z = yl = 0 (qp_admm.h:120-121) ----
        for (int i = w; i < t.n; i += ADMM_ST_WAVES) {
            T q = (T) 0;
            if (valid) {
                if (a.y_is_f64) q = (T) (2 * reinterpret_cast<const double *>(a.y)[(size_t) frame * t.n + i] / a.var);
                else q = (T) (2 * (double) reinterpret_cast<const float *>(a.y)[(size_t) frame * t.n + i] / a.var);
            }
            Q[(size_t) i * 64 + lane] = q;
        }
        for (int j = w; j < t.n_con; j += ADMM_ST_WAVES) W[(size_t) j * 64 + lane] = (T) 0;
        __syncthreads();

        bool live = valid;  // identical in every wavefront: all of them combine the same partial sums in the same order
        int iters = 0;
        for (int it = 0; it < a.max_iter; ++it) {
            // ---- v-update (qp_admm.h:132-142) ----
            for (int i = w; i < t.n_var; i += ADMM_ST_WAVES) {
                T B = (i < t.n ? Q[(size_t) i * 64 + lane] : (T) 0) + half_alpha;
                const int k0 = sload_c(t.var_ptr, i), k1 = sload_c(t.var_ptr, i + 1);
                for (int k = k0; k < k1; ++k) {
                    const uint32_t e = sload_c(t.var_ent, k);
                    const int j0 = (int) (e & 0x0FFFFFFFu), wp = (int) ((e >> 28) & 3u), ty = (int) (e >> 30);
                    const T *Wj = W + (size_t) j0 * 64 + lane;
                    T wv[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) wv[r] = (r < admm_group_rows(ty)) ? Wj[r * 64] : (T) 0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (r < admm_group_rows(ty)) {
                            const T z = ((T) 0 < wv[r]) ? wv[r] : (T) 0;
                            const T nw = -wv[r];
                            const T yl = ((T) 0 < nw) ? nw : (T) 0;
                            const T term = yl + mu * (z - (T) admm_row_b(ty, r));
                            B += admm_row_plus(ty, r, wp) ? term : -term;
                        }
                    }
                }
                T v = B * sload_c(inv_coef, i);
                v = (v < (T) 0) ? (T) 0 : v;  // std::max(v, 0.0)
                v = ((T) 1 < v) ? (T) 1 : v;  // std::min(v, 1.0)
                if (live) V[(size_t) i * 64 + lane] = v;
            }
            __syncthreads();
            // ---- residual, multiplier and slack update (qp_admm.h:144-159) ----
            T sum2 = (T) 0;
            for (int g = w; g < t.n_grp; g += ADMM_ST_WAVES) {
                const uint32_t hdr = sload_c(t.grp, (int64_t) g * 4);
                const int j0 = (int) (hdr & 0x0FFFFFFFu), ty = (int) (hdr >> 30);
                T vm[3];
                int wp[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const uint32_t m = (k < ty) ? sload_c(t.grp, (int64_t) g * 4 + 1 + k) : 0u;
                    wp[k] = (int) (m >> 30);
                    vm[k] = (k < ty) ? V[(size_t) (m & 0x3FFFFFFFu) * 64 + lane] : (T) 0;
                }
                T *Wj = W + (size_t) j0 * 64 + lane;
                T wo[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) wo[r] = (r < admm_group_rows(ty)) ? Wj[r * 64] : (T) 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (r < admm_group_rows(ty)) {
                        T rr = (T) admm_row_b(ty, r);
#pragma unroll
                        for (int k = 0; k < 3; ++k)
                            if (k < ty) rr = rr - (admm_row_plus(ty, r, wp[k]) ? vm[k] : -vm[k]);
                        const T nwo = -wo[r];
                        const T ylo = ((T) 0 < nwo) ? nwo : (T) 0;
                        const T wn = rr - ylo;
                        const T z = ((T) 0 < wn) ? wn : (T) 0;
                        if (live) Wj[r * 64] = wn;
                        const T d = z - rr;
                        sum2 += d * d;
                    }
                }
            }
            part[w][lane] = sum2;
            __syncthreads();
            T s = part[0][lane];
#pragma unroll
            for (int k = 1; k < ADMM_ST_WAVES; ++k) s += part[k][lane];
            if (live) {
                iters = it + 1;
                if (s < eps_stop) live = false;  // qp_admm.h:161-163: this frame's state is final
            }
            if (a.early_exit && __ballot(live) == 0ull) break;  // uniform over the workgroup (see `live`)
        }
        // ---- outputs (qp_admm.h:166-177) ----
        if (valid) {
            if (w == 0) {
                if (a.out_ok) a.out_ok[frame] = 1;
                if (a.out_iters) a.out_iters[frame] = iters;
            }
            if (a.out_bits)
                for (int k = w; k < t.nwords; k += ADMM_ST_WAVES) {
                    uint32_t word = 0;
                    const int vend = min(32, t.n - 32 * k);
                    for (int b = 0; b < vend; ++b) {
                        const T val = V[(size_t) (32 * k + b) * 64 + lane];
                        word |= (val <= (T) 0.5 ? 0u : 1u) << b;
                    }
                    a.out_bits[(size_t) frame * t.nwords + k] = word;
                }
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------

struct AdmmStream {
    AdmmStreamDev t{};
    std::vector<DeviceBuf> allocs;
    DeviceBuf ws;
    int slabs = 0, f32 = 0;
    double alpha = 0, mu = 0, eps = 0;
    std::vector<double> e;  // [n_var] (admm_stream_set_point)
};

void admm_stream_destroy(AdmmStream *s) { delete s; }

// Workspace: one slab per workgroup, (C + n_var + n) x 64 words, plain hipMalloc when the decoder is created.
// Slabs = min(2 x CUs, what fits in a quarter of the free device memory), at least one; none fitting is an error.
AdmmStream *admm_stream_create(const Code &c, const acg_ldpc_params &p, int cu_count, std::string &err) {
    AdmmStreamTables h;
    if (!admm_stream_tables_build(c, h)) {
        err = "code too large for the streamed QP-ADMM engine (2^28 constraint rows, 2^30 variables)";
        return nullptr;
    }
    std::unique_ptr<AdmmStream> s(new AdmmStream());
    s->f32 = (p.precision == ACG_LDPC_PREC_F32) ? 1 : 0;
    s->alpha = p.alpha;
    s->mu = p.mu;
    s->eps = p.eps_stop;
    s->e = c.admm.e;
    AdmmStreamDev &t = s->t;
    t.n = h.n;
    t.n_var = h.n_var;
    t.n_con = h.n_con;
    t.n_grp = h.n_grp;
    t.nwords = (c.n + 31) / 32;
    std::vector<double> inv64(h.n_var);
    for (int i = 0; i < h.n_var; i++) {
        const double Acoef = (p.mu * c.admm.e[i] - p.alpha) / 2;  // qp_admm.h:125
        inv64[i] = -1.0 / (2 * Acoef);                           // qp_admm.h:126
    }
    t.var_ptr = upload_keep(h.var_ptr, s->allocs);
    t.var_ent = upload_keep(h.var_ent, s->allocs);
    t.grp = upload_keep(h.grp, s->allocs);
    if (s->f32) t.inv_coef = upload_keep(std::vector<float>(inv64.begin(), inv64.end()), s->allocs);
    else t.inv_coef = upload_keep(inv64, s->allocs);
    if (!t.var_ptr || !t.var_ent || !t.grp || !t.inv_coef) {
        err = "hipMalloc / hipMemcpy of the streamed QP-ADMM tables failed";
        return nullptr;
    }
    const size_t ts = s->f32 ? 4 : 8;
    t.slab_bytes = (int64_t) ((((size_t) h.n_con + h.n_var + h.n) * 64 * ts + 255) & ~(size_t) 255);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
        err = "hipMemGetInfo failed";
        return nullptr;
    }
    const size_t budget = free_b / 4;
    const size_t fit = budget / (size_t) t.slab_bytes;
    if (fit < 1) {
        err = "streamed QP-ADMM engine: one slab of " + std::to_string(t.slab_bytes) + " bytes exceeds a quarter of the free device memory (" +
              std::to_string(free_b) + " bytes)";
        return nullptr;
    }
    s->slabs = (int) std::min<size_t>((size_t) 2 * std::max(cu_count, 1), fit);
    if (s->ws.reserve((size_t) s->slabs * (size_t) t.slab_bytes)) {
        err = "hipMalloc of the streamed QP-ADMM workspace (" + std::to_string((size_t) s->slabs * (size_t) t.slab_bytes) + " bytes) failed";
        return nullptr;
    }
    return s.release();
}

// Re-parameterise in place (parameter grids, acg_ldpc_mc_run_grid): alpha, mu and the inv_coef table, built as in
// admm_stream_create.  No launch of this engine may be in flight.
bool admm_stream_set_point(AdmmStream *s, double alpha, double mu) {
    s->alpha = alpha;
    s->mu = mu;
    std::vector<double> inv64(s->e.size());
    for (size_t i = 0; i < s->e.size(); i++) {
        const double Acoef = (mu * s->e[i] - alpha) / 2;  // qp_admm.h:125
        inv64[i] = -1.0 / (2 * Acoef);                    // qp_admm.h:126
    }
    if (inv64.empty()) return true;
    void *dst = const_cast<void *>(s->t.inv_coef);
    if (s->f32) {
        const std::vector<float> inv32(inv64.begin(), inv64.end());
        return hipMemcpy(dst, inv32.data(), inv32.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
    }
    return hipMemcpy(dst, inv64.data(), inv64.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
}

void admm_stream_info(const AdmmStream *s, int *slabs, int64_t *slab_bytes, int *f32) {
    if (slabs) *slabs = s->slabs;
    if (slab_bytes) *slab_bytes = s->t.slab_bytes;
    if (f32) *f32 = s->f32;
}

// sweeps only: the guard, a sweep budget of 0 and Monte-Carlo mode are dispatched by admm_launch before this is called
hipError_t admm_stream_launch(AdmmStream *s, const DecodeArgs &a, hipStream_t st) {
    const int64_t tiles = (a.frames + 63) / 64;
    const int grid = (int) std::min<int64_t>(tiles, s->slabs);
    if (grid <= 0) return hipSuccess;
    AdmmStreamDev tt = s->t;
    DecodeArgs aa = a;
    unsigned char *ws = s->ws.as<unsigned char>();
    if (s->f32) {
        float alpha = (float) s->alpha, mu = (float) s->mu, eps = (float) s->eps;
        void *args[6] = {&tt, &aa, &alpha, &mu, &eps, &ws};
        return hipLaunchKernel((const void *) admm_streamed_kernel<float>, dim3(grid), dim3(ADMM_ST_WAVES * 64), args, 0, st);
    }
    double alpha = s->alpha, mu = s->mu, eps = s->eps;
    void *args[6] = {&tt, &aa, &alpha, &mu, &eps, &ws};
    return hipLaunchKernel((const void *) admm_streamed_kernel<double>, dim3(grid), dim3(ADMM_ST_WAVES * 64), args, 0, st);
}

}  // namespace acg
