// Fused belief-propagation kernels for gfx950 (MI355X).
//
// Replaces, for a whole batch of frames per launch, the reference's per-frame
//   BeliefPropagation::decode            algo/bp.h:183-199
//   c_receive_messages / VNode::message  algo/bp.h:160-169, 77-83   (variable -> check)
//   v_receive_messages / CNode::message  algo/bp.h:171-181, 49-57   (check -> variable)
//   VNode::estimate + IsCodeword         algo/bp.h:85-90, 191-196 ; utils/codeword.h:90-95
// and, in Monte-Carlo mode, transmit (utils/channel.h:18-26) and the per-frame classification
// of exp() (experiment.h:109-120).
//
// Mapping: L lanes of a 64-wide wavefront (L = 64, 32 or 16) cooperate on ONE
// frame; the frame's E messages live in LDS for all iterations, updated in place, so HBM sees
// only the channel symbols in and the packed hard decisions out.  The Tanner graph is shared by
// every frame of the launch, so all graph indices are either implicit in the layout (check side:
// unit-stride, bank-conflict-free) or small read-only tables (variable side).  No cross-lane
// traffic is needed inside a phase: each lane owns whole nodes and forms the exclude-self sums
// (bp.h:50-55, 78-81) with a prefix/suffix scan in registers.  The per-check parity of the hard
// decisions rides in the LSB of each v->c magnitude, so the syndrome test costs one XOR per edge
// and a wave ballot.
//
// Source layout: bp_core.inc holds the kernel; bp_inst_{spa,ms}_{f32,f64}.hip instantiate it (parallel
// compilation); this file holds the dispatcher, the launcher and the stand-alone debug/AWGN kernels.
//
// A wavefront is a persistent worker: each L-lane group walks frames g, g+G, g+2G, ... and
// restarts on a new frame the moment its current one reaches a zero syndrome (the reference's
// early exit, bp.h:195-196), independently of the other groups in the wave.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "launchers.hpp"

namespace acg {
#include "bp_core.inc"

const void *bp_kernel_ptr_dbg(int f64, int L) {
#ifdef ACG_FAST_BUILD
    return f64 ? nullptr : bp_kernel_ptr_spa_f32_dbg(L);
#else
    return f64 ? bp_kernel_ptr_spa_f64_dbg(L) : bp_kernel_ptr_spa_f32_dbg(L);
#endif
}

// algo: 0 sum-product, 1 min-sum; f64: 0/1; sat: the phi fast path where an instance has it (fp32 sum-product)
const void *bp_kernel_ptr(int algo, int f64, int maxd, int L, bool mc, int variant, bool sat) {
#ifdef ACG_FAST_BUILD
    if (f64 || algo) return nullptr;
    return bp_kernel_ptr_spa_f32(maxd, L, mc, variant, sat);
#else
    if (algo == 0) return f64 ? bp_kernel_ptr_spa_f64(maxd, L, mc, variant) : bp_kernel_ptr_spa_f32(maxd, L, mc, variant, sat);
    return f64 ? bp_kernel_ptr_ms_f64(maxd, L, mc, variant) : bp_kernel_ptr_ms_f32(maxd, L, mc, variant);
#endif
}

hipError_t bp_launch(const void *kernel, const BpTables &t, const DecodeArgs &a, int grid, int block, size_t lds,
                     hipStream_t s) {
    BpTables tt = t;
    DecodeArgs aa = a;
    void *args[2] = {&tt, &aa};
    return hipLaunchKernel(kernel, dim3(grid), dim3(block), args, lds, s);
}

// ------------------------------------------------------------------------------------------
// debug / test kernels
__global__ void phi_debug_kernel(const float *x, float *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    // the fp32 kernels evaluate phi in the log2(e)-scaled domain: report it back in natural units
    if (i < n) out[i] = (float) ((double) Dom<float>::phi((float) ((double) x[i] * Dom<float>::scale)) / Dom<float>::scale);
}
__global__ void phi_debug_kernel_f64(const double *x, double *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = phi_f(x[i]);
}

// the phi fast path of the fp32 sum-product sweeps against the full evaluation, raw bits in the scaled domain:
// out[3i] = Dom<float>::phi(x), out[3i+1] = BpPass::phi_c(x) (check side), out[3i+2] = BpPass::phi_v(|x|) (variable side)
__global__ void phi_sat_debug_kernel(const float *x, uint32_t *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    using P = BpPass<float, 1, 64, 0, true>;
    if (i < n) {
        out[3 * i] = __float_as_uint(Dom<float>::phi(x[i]));
        out[3 * i + 1] = __float_as_uint(P::phi_c(x[i]));
        out[3 * i + 2] = __float_as_uint(P::phi_v(__builtin_fabsf(x[i])));
    }
}

hipError_t phi_sat_debug_launch(const float *x, uint32_t *out, int n, hipStream_t s) {
    hipLaunchKernelGGL(phi_sat_debug_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x, out, n);
    return hipGetLastError();
}

hipError_t phi_debug_launch(const void *x, void *out, int n, int f64, hipStream_t s) {
    if (f64)
        hipLaunchKernelGGL(phi_debug_kernel_f64, dim3((n + 255) / 256), dim3(256), 0, s, (const double *) x, (double *) out, n);
    else
        hipLaunchKernelGGL(phi_debug_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const float *) x, (float *) out, n);
    return hipGetLastError();
}

// standalone AWGN generator (utils/channel.h:18-26 with Philox): y[frame][v] natural order
__global__ void awgn_kernel(float *y, int64_t frames, int n, int nwords, int64_t first_frame, uint64_t seed,
                            const uint32_t *cw_packed, int64_t n_cw, float sigma) {
    const int nq = (n + 3) >> 2;
    const int64_t total = frames * nq;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t) gridDim.x * blockDim.x) {
        const int64_t f = i / nq;
        const int q = (int) (i - f * nq);
        const int64_t gf = first_frame + f;
        uint32_t r[4];
        philox4x32_10((uint32_t) gf, (uint32_t) (gf >> 32), (uint32_t) q, 0u, (uint32_t) seed, (uint32_t) (seed >> 32), r);
        float z[4];
        box_muller(r[0], r[1], z[0], z[1]);
        box_muller(r[2], r[3], z[2], z[3]);
        const uint32_t *cw = cw_packed ? cw_packed + (size_t) (gf % n_cw) * nwords : nullptr;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int v = 4 * q + e;
            if (v < n) {
                const uint32_t bit = cw ? ((cw[v >> 5] >> (v & 31)) & 1u) : 0u;
                y[(size_t) f * n + v] = __builtin_fmaf(sigma, z[e], bit ? -1.0f : 1.0f);  // explicit fma: same symbol in every kernel
            }
        }
    }
}

// Classification of ONE frame by one wavefront (experiment.h:109-120): raw-channel Hamming count from y, and
// correct <=> ok and the word equals the sent one.  bits == null stands for the all-zero word.
template <typename Y>
__device__ __forceinline__ void classify_frame(const Y *y, const uint32_t *bits, bool okf, const uint32_t *cw, int n, int nwords,
                                               const int32_t *row_ptr, const int32_t *edge_var, int m, int lane, int &ham,
                                               bool &correct, bool &pseudo) {
    ham = 0;
    for (int v = lane; v < n; v += 64) {
        const uint32_t bit = cw ? ((cw[v >> 5] >> (v & 31)) & 1u) : 0u;
        const Y yv = y[v];
        ham += ((!bit && yv <= (Y) 0) || (bit && yv > (Y) 0)) ? 1 : 0;
    }
    bool neq = false;
    for (int w = lane; w < nwords; w += 64) neq |= ((bits ? bits[w] : 0u) != (cw ? cw[w] : 0u));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ham += __shfl_xor(ham, o, 64);
    const bool differ = __ballot(neq) != 0ull;
    if (row_ptr) {  // decoders that always report ok (QP-ADMM, qp_admm.h:177): IsCodeword here (experiment.h:111)
        bool sbad = false;
        for (int c = lane; c < m; c += 64) {
            uint32_t sy = 0;
            for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e) {
                const int v = edge_var[e];
                sy ^= bits ? (bits[v >> 5] >> (v & 31)) & 1u : 0u;
            }
            sbad |= (sy != 0u);
        }
        okf = okf && (__ballot(sbad) == 0ull);
    }
    correct = okf && !differ;
    pseudo = okf && differ;
}

// Per-frame classification of exp() (experiment.h:109-120) for engines without an in-kernel generator:
// one wavefront per frame.
__global__ void classify_kernel(const float *y, const uint32_t *bits, const uint8_t *ok, const int32_t *iters,
                                int64_t frames, int n, int nwords, int64_t first_frame, const uint32_t *cw_packed,
                                int64_t n_cw, unsigned long long *counters, const int32_t *row_ptr,
                                const int32_t *edge_var, int m) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nw = (int64_t) gridDim.x * (blockDim.x >> 6);
    unsigned long long c_ok = 0, c_ps = 0, c_tot = 0, c_h = 0, c_hok = 0, c_hw = 0, c_it = 0;
    for (int64_t f = wid; f < frames; f += nw) {
        const uint32_t *cw = cw_packed ? cw_packed + (size_t) ((first_frame + f) % n_cw) * nwords : nullptr;
        int ham;
        bool correct, pseudo;
        classify_frame(y + (size_t) f * n, bits + (size_t) f * nwords, ok[f] != 0, cw, n, nwords, row_ptr, edge_var, m, lane, ham,
                       correct, pseudo);
        c_ok += correct;
        c_ps += pseudo;
        c_tot += 1;
        c_h += ham;
        c_hok += correct ? ham : 0;
        c_hw += correct ? 0 : ham;
        c_it += iters ? iters[f] : 0;
    }
    if (lane == 0 && c_tot) {
        atomicAdd(&counters[MC_CORRECT], c_ok);
        atomicAdd(&counters[MC_PSEUDO], c_ps);
        atomicAdd(&counters[MC_TOTAL], c_tot);
        atomicAdd(&counters[MC_HAM], c_h);
        atomicAdd(&counters[MC_HAM_OK], c_hok);
        atomicAdd(&counters[MC_HAM_WRONG], c_hw);
        atomicAdd(&counters[MC_ITERS], c_it);
    }
}

// The same for a parameter grid (acg_ldpc_mc_run_grid): virtual frame g = point * frames + f carries the outputs of frame
// f decoded with the parameters of `point`; its symbols and sent word are those of frame f, its counters row is
// counters[point].  bits == null (then ok and iters are null too): guard points — all-zero words, ok = false, no sweeps.
// A wavefront takes a contiguous run of virtual frames, so it changes point (and flushes its sums) rarely.
template <typename Y>
__global__ void classify_grid_kernel(const Y *y, const uint32_t *bits, const uint8_t *ok, const int32_t *iters, int64_t frames,
                                     int64_t points, int n, int nwords, int64_t first_frame, const uint32_t *cw_packed, int64_t n_cw,
                                     unsigned long long *counters, const int32_t *row_ptr, const int32_t *edge_var, int m) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nw = (int64_t) gridDim.x * (blockDim.x >> 6);
    const int64_t total = frames * points, per = (total + nw - 1) / nw;
    const int64_t g0 = wid * per, g1 = g0 + per < total ? g0 + per : total;
    unsigned long long c_ok = 0, c_ps = 0, c_tot = 0, c_h = 0, c_hok = 0, c_hw = 0, c_it = 0;
    auto flush = [&](int64_t point) {
        if (lane == 0 && c_tot) {
            unsigned long long *row = counters + (size_t) point * MC_NCOUNTERS;
            atomicAdd(&row[MC_CORRECT], c_ok);
            atomicAdd(&row[MC_PSEUDO], c_ps);
            atomicAdd(&row[MC_TOTAL], c_tot);
            atomicAdd(&row[MC_HAM], c_h);
            atomicAdd(&row[MC_HAM_OK], c_hok);
            atomicAdd(&row[MC_HAM_WRONG], c_hw);
            atomicAdd(&row[MC_ITERS], c_it);
        }
        c_ok = c_ps = c_tot = c_h = c_hok = c_hw = c_it = 0;
    };
    int64_t point = g0 < g1 ? g0 / frames : 0;
    for (int64_t g = g0; g < g1; ++g) {
        if (g >= (point + 1) * frames) {
            flush(point);
            point = g / frames;
        }
        const int64_t f = g - point * frames;
        const uint32_t *cw = cw_packed ? cw_packed + (size_t) ((first_frame + f) % n_cw) * nwords : nullptr;
        int ham;
        bool correct, pseudo;
        classify_frame(y + (size_t) f * n, bits ? bits + (size_t) g * nwords : nullptr, bits ? ok[g] != 0 : false, cw, n, nwords, row_ptr,
                       edge_var, m, lane, ham, correct, pseudo);
        c_ok += correct;
        c_ps += pseudo;
        c_tot += 1;
        c_h += ham;
        c_hok += correct ? ham : 0;
        c_hw += correct ? 0 : ham;
        c_it += (bits && iters) ? iters[g] : 0;
    }
    flush(point);
}

hipError_t classify_grid_launch(const void *y, int y_is_f64, const uint32_t *bits, const uint8_t *ok, const int32_t *iters,
                                int64_t frames, int64_t points, int n, int nwords, int64_t first_frame, const uint32_t *cw_packed,
                                int64_t n_cw, unsigned long long *counters, const int32_t *row_ptr, const int32_t *edge_var, int m,
                                hipStream_t s) {
    int grid = (int) std::min<int64_t>((frames * points + 3) / 4, 256 * 8);
    if (grid < 1) grid = 1;
    if (y_is_f64)
        hipLaunchKernelGGL(classify_grid_kernel<double>, dim3(grid), dim3(256), 0, s, (const double *) y, bits, ok, iters, frames, points,
                           n, nwords, first_frame, cw_packed, n_cw, counters, row_ptr, edge_var, m);
    else
        hipLaunchKernelGGL(classify_grid_kernel<float>, dim3(grid), dim3(256), 0, s, (const float *) y, bits, ok, iters, frames, points, n,
                           nwords, first_frame, cw_packed, n_cw, counters, row_ptr, edge_var, m);
    return hipGetLastError();
}

// The same for a batch of codes (acg_ldpc_mc_run_codes): virtual frame g = code * frames + f carries the outputs of frame f
// decoded with code `code`; its symbols are y[g] (every code transmits its own words), its sent word, CSR and counters row are
// refs[code]'s.  bits == null (then ok and iters are null too): guard codes — all-zero words, ok = false, no sweeps.
template <typename Y>
__global__ void classify_codes_kernel(const Y *y, const uint32_t *bits, const uint8_t *ok, const int32_t *iters, int64_t frames,
                                      int64_t codes, int n, int nwords, int64_t first_frame, const CodeRef *refs, int m) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nw = (int64_t) gridDim.x * (blockDim.x >> 6);
    const int64_t total = frames * codes, per = (total + nw - 1) / nw;
    const int64_t g0 = wid * per, g1 = g0 + per < total ? g0 + per : total;
    unsigned long long c_ok = 0, c_ps = 0, c_tot = 0, c_h = 0, c_hok = 0, c_hw = 0, c_it = 0;
    auto flush = [&](int64_t code) {
        if (lane == 0 && c_tot) {
            unsigned long long *row = refs[code].counters;
            atomicAdd(&row[MC_CORRECT], c_ok);
            atomicAdd(&row[MC_PSEUDO], c_ps);
            atomicAdd(&row[MC_TOTAL], c_tot);
            atomicAdd(&row[MC_HAM], c_h);
            atomicAdd(&row[MC_HAM_OK], c_hok);
            atomicAdd(&row[MC_HAM_WRONG], c_hw);
            atomicAdd(&row[MC_ITERS], c_it);
        }
        c_ok = c_ps = c_tot = c_h = c_hok = c_hw = c_it = 0;
    };
    int64_t code = g0 < g1 ? g0 / frames : 0;
    for (int64_t g = g0; g < g1; ++g) {
        if (g >= (code + 1) * frames) {
            flush(code);
            code = g / frames;
        }
        const int64_t f = g - code * frames;
        const CodeRef r = refs[code];
        const uint32_t *cw = r.cw_packed ? r.cw_packed + (size_t) ((first_frame + f) % r.n_cw) * nwords : nullptr;
        int ham;
        bool correct, pseudo;
        classify_frame(y + (size_t) g * n, bits ? bits + (size_t) g * nwords : nullptr, bits ? ok[g] != 0 : false, cw, n, nwords,
                       bits ? r.row_ptr : nullptr, r.edge_var, m, lane, ham, correct, pseudo);
        c_ok += correct;
        c_ps += pseudo;
        c_tot += 1;
        c_h += ham;
        c_hok += correct ? ham : 0;
        c_hw += correct ? 0 : ham;
        c_it += (bits && iters) ? iters[g] : 0;
    }
    flush(code);
}

hipError_t classify_codes_launch(const void *y, int y_is_f64, const uint32_t *bits, const uint8_t *ok, const int32_t *iters,
                                 int64_t frames, int64_t codes, int n, int nwords, int64_t first_frame, const CodeRef *refs, int m,
                                 hipStream_t s) {
    int grid = (int) std::min<int64_t>((frames * codes + 3) / 4, 256 * 8);
    if (grid < 1) grid = 1;
    if (y_is_f64)
        hipLaunchKernelGGL(classify_codes_kernel<double>, dim3(grid), dim3(256), 0, s, (const double *) y, bits, ok, iters, frames, codes,
                           n, nwords, first_frame, refs, m);
    else
        hipLaunchKernelGGL(classify_codes_kernel<float>, dim3(grid), dim3(256), 0, s, (const float *) y, bits, ok, iters, frames, codes, n,
                           nwords, first_frame, refs, m);
    return hipGetLastError();
}

// Host-noise symbols of a batch of codes: y[code][f][v] = (+-1 of the code's sent word) + noise[f][v], in double — the one
// IEEE addition of utils/channel.h:24 with the normal deviate the host drew for global frame first_frame + f, which is the
// same for every code (the generator is seeded by the frame alone, experiment.h:90-99).
__global__ void codes_symbols_kernel(const double *noise, double *y, int64_t frames, int64_t codes, int n, int nwords, int64_t first_frame,
                                     const CodeRef *refs) {
    const int64_t per = frames * n, total = per * codes;
    for (int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t) gridDim.x * blockDim.x) {
        const int64_t code = i / per, r = i - code * per, f = r / n;
        const int v = (int) (r - f * n);
        const CodeRef c = refs[code];
        const uint32_t bit = c.cw_packed ? (c.cw_packed[(size_t) ((first_frame + f) % c.n_cw) * nwords + (v >> 5)] >> (v & 31)) & 1u : 0u;
        y[i] = (bit ? -1.0 : 1.0) + noise[r];
    }
}

hipError_t codes_symbols_launch(const double *noise, double *y, int64_t frames, int64_t codes, int n, int nwords, int64_t first_frame,
                                const CodeRef *refs, hipStream_t s) {
    const int64_t total = frames * codes * n;
    int grid = (int) std::min<int64_t>((total + 255) / 256, 256 * 16);
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(codes_symbols_kernel, dim3(grid), dim3(256), 0, s, noise, y, frames, codes, n, nwords, first_frame, refs);
    return hipGetLastError();
}

hipError_t classify_launch(const float *y, const uint32_t *bits, const uint8_t *ok, const int32_t *iters, int64_t frames,
                           int n, int nwords, int64_t first_frame, const uint32_t *cw_packed, int64_t n_cw,
                           unsigned long long *counters, const int32_t *row_ptr, const int32_t *edge_var, int m,
                           hipStream_t s) {
    int grid = (int) std::min<int64_t>((frames + 3) / 4, 256 * 8);
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(classify_kernel, dim3(grid), dim3(256), 0, s, y, bits, ok, iters, frames, n, nwords, first_frame,
                       cw_packed, n_cw, counters, row_ptr, edge_var, m);
    return hipGetLastError();
}

// ---- detail run (acg_ldpc_mc_run_detail) --------------------------------------------------------------------------------
// What one wavefront adds to classify_frame for the detail run: d_H(word, sent) with the bits >= n of the last word masked
// off, and, for decoders that pass a CSR (QP-ADMM), the number of unsatisfied checks.  Both are wave-uniform on return.
__device__ __forceinline__ void frame_detail(const uint32_t *bits, const uint32_t *cw, int n, int nwords, const int32_t *row_ptr,
                                             const int32_t *edge_var, int m, int lane, int &dist, int &synw) {
    const uint32_t last_mask = (n & 31) ? ((1u << (n & 31)) - 1u) : 0xFFFFFFFFu;
    dist = 0;
    for (int w = lane; w < nwords; w += 64) {
        const uint32_t x = (bits[w] ^ (cw ? cw[w] : 0u)) & (w == nwords - 1 ? last_mask : 0xFFFFFFFFu);
        dist += __popc(x);
    }
    synw = 0;
    if (row_ptr) {
        for (int c = lane; c < m; c += 64) {
            uint32_t sy = 0;
            for (int e = row_ptr[c]; e < row_ptr[c + 1]; ++e) {
                const int v = edge_var[e];
                sy ^= (bits[v >> 5] >> (v & 31)) & 1u;
            }
            synw += (int) sy;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        dist += __shfl_xor(dist, o, 64);
        synw += __shfl_xor(synw, o, 64);
    }
}

// ACG_LDPC_EVENT_* of a frame, 0 for a correct one (experiment.h:109-120 extended: the frames that are not correct, split by
// what the decoder returned)
__device__ __forceinline__ int frame_kind(bool flag, bool correct, bool pseudo) {
    if (correct) return 0;
    if (pseudo) return ACG_LDPC_EVENT_PSEUDO;
    return flag ? ACG_LDPC_EVENT_NONCODEWORD : ACG_LDPC_EVENT_NO_WORD;
}

// classify_kernel plus the detail counters: one wavefront per frame, sums kept per wavefront, one set of atomics at the end.
// counters: DET_NCOUNTERS words; [0, MC_NCOUNTERS) are classify_kernel's.  kind[f] = the frame's ACG_LDPC_EVENT_* or 0.
// counters[DET_MIN_PSEUDO] = min over the pseudo frames of (weight << 32 | chunk-relative frame): the lowest frame wins ties.
__global__ void classify_detail_kernel(const float *y, const uint32_t *bits, const uint8_t *ok, const int32_t *iters,
                                       int64_t frames, int n, int nwords, int64_t first_frame, const uint32_t *cw_packed,
                                       int64_t n_cw, unsigned long long *counters, uint8_t *kind, const int32_t *row_ptr,
                                       const int32_t *edge_var, int m) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nw = (int64_t) gridDim.x * (blockDim.x >> 6);
    unsigned long long c_ok = 0, c_ps = 0, c_tot = 0, c_h = 0, c_hok = 0, c_hw = 0, c_it = 0;
    unsigned long long c_word = 0, c_be = 0, c_ncw = 0, c_syn = 0, c_minp = ~0ull;
    for (int64_t f = wid; f < frames; f += nw) {
        const uint32_t *cw = cw_packed ? cw_packed + (size_t) ((first_frame + f) % n_cw) * nwords : nullptr;
        const uint32_t *b = bits + (size_t) f * nwords;
        const bool flag = ok[f] != 0;
        int ham;
        bool correct, pseudo;
        classify_frame(y + (size_t) f * n, b, flag, cw, n, nwords, row_ptr, edge_var, m, lane, ham, correct, pseudo);
        c_ok += correct;
        c_ps += pseudo;
        c_tot += 1;
        c_h += ham;
        c_hok += correct ? ham : 0;
        c_hw += correct ? 0 : ham;
        c_it += iters ? iters[f] : 0;
        const int k = frame_kind(flag, correct, pseudo);
        if (lane == 0) kind[f] = (uint8_t) k;
        if (flag && !correct) {   // (a correct frame has distance 0 and no unsatisfied check)
            int dist, synw;
            frame_detail(b, cw, n, nwords, row_ptr, edge_var, m, lane, dist, synw);
            c_be += (unsigned long long) dist;
            if (k == ACG_LDPC_EVENT_NONCODEWORD) {
                c_ncw += 1;
                c_syn += (unsigned long long) synw;
            } else {
                const unsigned long long key = ((unsigned long long) (uint32_t) dist << 32) | (unsigned long long) (uint32_t) f;
                c_minp = key < c_minp ? key : c_minp;
            }
        }
        c_word += flag;
    }
    if (lane == 0 && c_tot) {
        atomicAdd(&counters[MC_CORRECT], c_ok);
        atomicAdd(&counters[MC_PSEUDO], c_ps);
        atomicAdd(&counters[MC_TOTAL], c_tot);
        atomicAdd(&counters[MC_HAM], c_h);
        atomicAdd(&counters[MC_HAM_OK], c_hok);
        atomicAdd(&counters[MC_HAM_WRONG], c_hw);
        atomicAdd(&counters[MC_ITERS], c_it);
        atomicAdd(&counters[DET_WORD_FRAMES], c_word);
        if (c_be) atomicAdd(&counters[DET_BIT_ERRORS], c_be);
        if (c_ncw) {
            atomicAdd(&counters[DET_NONCODEWORD], c_ncw);
            atomicAdd(&counters[DET_SYNDROME], c_syn);
        }
        if (c_minp != ~0ull) atomicMin(&counters[DET_MIN_PSEUDO], c_minp);
    }
}

// The records and XOR rows of the selected frames of a chunk (sel[k] = chunk-relative frame, ascending), from the chunk's
// still-resident symbols and decode outputs: one wavefront per event.  words == null: records only.
__global__ void gather_events_kernel(const int32_t *sel, int n_sel, const float *y, const uint32_t *bits, const uint8_t *ok,
                                     const int32_t *iters, const uint8_t *kind, int n, int nwords, int64_t first_frame,
                                     const uint32_t *cw_packed, int64_t n_cw, const int32_t *row_ptr, const int32_t *edge_var, int m,
                                     acg_ldpc_mc_event *events, uint32_t *words) {
    const int lane = threadIdx.x & 63;
    const int wid = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int nw = gridDim.x * (blockDim.x >> 6);
    const uint32_t last_mask = (n & 31) ? ((1u << (n & 31)) - 1u) : 0xFFFFFFFFu;
    for (int k = wid; k < n_sel; k += nw) {
        const int64_t f = sel[k];
        const uint32_t *cw = cw_packed ? cw_packed + (size_t) ((first_frame + f) % n_cw) * nwords : nullptr;
        const uint32_t *b = bits + (size_t) f * nwords;
        const bool flag = ok[f] != 0;
        int ham;
        bool correct, pseudo;
        classify_frame(y + (size_t) f * n, b, flag, cw, n, nwords, nullptr, nullptr, 0, lane, ham, correct, pseudo);  // (for ham)
        int dist = 0, synw = 0;
        if (flag) frame_detail(b, cw, n, nwords, row_ptr, edge_var, m, lane, dist, synw);
        if (lane == 0) {
            acg_ldpc_mc_event ev;
            ev.frame = first_frame + f;
            ev.kind = kind[f];
            ev.iters = iters ? iters[f] : 0;
            ev.raw_errors = ham;
            ev.bit_errors = dist;
            ev.syndrome_weight = ev.kind == ACG_LDPC_EVENT_NONCODEWORD ? synw : 0;
            ev.reserved = 0;
            events[k] = ev;
        }
        if (words)
            for (int w = lane; w < nwords; w += 64)
                words[(size_t) k * nwords + w] = flag ? (b[w] ^ (cw ? cw[w] : 0u)) & (w == nwords - 1 ? last_mask : 0xFFFFFFFFu) : 0u;
    }
}

hipError_t classify_detail_launch(const float *y, const uint32_t *bits, const uint8_t *ok, const int32_t *iters, int64_t frames,
                                  int n, int nwords, int64_t first_frame, const uint32_t *cw_packed, int64_t n_cw,
                                  unsigned long long *counters, uint8_t *kind, const int32_t *row_ptr, const int32_t *edge_var, int m,
                                  hipStream_t s) {
    int grid = (int) std::min<int64_t>((frames + 3) / 4, 256 * 8);
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(classify_detail_kernel, dim3(grid), dim3(256), 0, s, y, bits, ok, iters, frames, n, nwords, first_frame,
                       cw_packed, n_cw, counters, kind, row_ptr, edge_var, m);
    return hipGetLastError();
}

hipError_t gather_events_launch(const int32_t *sel, int n_sel, const float *y, const uint32_t *bits, const uint8_t *ok,
                                const int32_t *iters, const uint8_t *kind, int n, int nwords, int64_t first_frame,
                                const uint32_t *cw_packed, int64_t n_cw, const int32_t *row_ptr, const int32_t *edge_var, int m,
                                acg_ldpc_mc_event *events, uint32_t *words, hipStream_t s) {
    int grid = std::min((n_sel + 3) / 4, 256 * 8);
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(gather_events_kernel, dim3(grid), dim3(256), 0, s, sel, n_sel, y, bits, ok, iters, kind, n, nwords,
                       first_frame, cw_packed, n_cw, row_ptr, edge_var, m, events, words);
    return hipGetLastError();
}

hipError_t awgn_launch(float *y, int64_t frames, int n, int nwords, int64_t first_frame, uint64_t seed,
                       const uint32_t *cw_packed, int64_t n_cw, float sigma, hipStream_t s) {
    const int64_t total = frames * ((n + 3) >> 2);
    int grid = (int) ((total + 255) / 256);
    if (grid > 256 * 16) grid = 256 * 16;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(awgn_kernel, dim3(grid), dim3(256), 0, s, y, frames, n, nwords, first_frame, seed, cw_packed,
                       n_cw, sigma);
    return hipGetLastError();
}

}  // namespace acg
