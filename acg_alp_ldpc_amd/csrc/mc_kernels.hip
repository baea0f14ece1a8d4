// Stand-alone Monte-Carlo kernels for gfx950 (MI355X), for what has no in-kernel generator and classifier: the AWGN generator,
// the classification of exp() (experiment.h:109-120) for one decoder, a parameter grid or a batch of codes, the detail run's
// classifier and event gatherer, the host-noise symbols of a batch of codes.  Philox / Box-Muller are bp_core.inc's own.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "launchers.hpp"

namespace acg {
#include "bp_core.inc"

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

#include "mc_tally.inc"  // struct Tally: the seven sums of acg_ldpc_mc_result as one wavefront keeps them

// Unit-source policies (DESIGN.md §4c').  A launch classifies units x frames virtual frames; g = u * frames + f carries the
// decode outputs of frame f of unit u.  A policy says which frame of y that was decoded from, and what unit u is: its sent
// words, its CSR (null = the decoder's ok flag already means IsCodeword) and its counters row, as one CodeRef.
// the points of a parameter grid (acg_ldpc_mc_run_grid), or the one decoder of acg_ldpc_mc_run: every unit decodes the SAME
// symbols and sent words with the same code; unit u counts into counters[u]
struct PointUnits {
    CodeRef common;  // .counters = row of unit 0
    __device__ int64_t symbols(int64_t f, int64_t g) const { return f; }
    __device__ CodeRef unit(int64_t u) const {
        return {common.cw_packed, common.n_cw, common.row_ptr, common.edge_var, common.counters + (size_t) u * MC_NCOUNTERS};
    }
};

// a batch of codes (acg_ldpc_mc_run_codes): every code transmits its own words, so its symbols are y[g]; all else is refs[u]'s
struct CodeUnits {
    const CodeRef *refs;
    __device__ int64_t symbols(int64_t f, int64_t g) const { return g; }
    __device__ CodeRef unit(int64_t u) const { return refs[u]; }
};

// Per-frame classification of exp() (experiment.h:109-120) for engines without an in-kernel classifier: one wavefront per
// virtual frame.  bits == null (then ok and iters are null too): guard units — all-zero words, ok = false, no sweeps, no CSR
// walk.  A wavefront takes a contiguous run of virtual frames, so it changes unit (and flushes its sums) rarely.
template <typename Y, class Units>
__global__ void classify_kernel(const Y *y, const uint32_t *bits, const uint8_t *ok, const int32_t *iters, int64_t frames,
                                int64_t units, int n, int nwords, int64_t first_frame, int m, Units src) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nw = (int64_t) gridDim.x * (blockDim.x >> 6);
    const int64_t total = frames * units, per = (total + nw - 1) / nw;
    const int64_t g0 = wid * per, g1 = g0 + per < total ? g0 + per : total;
    int64_t u = g0 < g1 ? g0 / frames : 0;
    CodeRef r = src.unit(u);
    Tally t;
    for (int64_t g = g0; g < g1; ++g) {
        if (g >= (u + 1) * frames) {
            t.flush(r.counters);
            u = g / frames;
            r = src.unit(u);
        }
        const int64_t f = g - u * frames;
        const uint32_t *cw = r.cw_packed ? r.cw_packed + (size_t) ((first_frame + f) % r.n_cw) * nwords : nullptr;
        const uint32_t *b = bits ? bits + (size_t) g * nwords : nullptr;
        int ham;
        bool correct, pseudo;
        classify_frame(y + (size_t) src.symbols(f, g) * n, b, b ? ok[g] != 0 : false, cw, n, nwords, b ? r.row_ptr : nullptr, r.edge_var,
                       m, lane, ham, correct, pseudo);
        t.add(correct, pseudo, ham, (b && iters) ? iters[g] : 0);
    }
    t.flush(r.counters);
}

template <class Units>
static hipError_t classify_units_launch(const void *y, int y_is_f64, const uint32_t *bits, const uint8_t *ok, const int32_t *iters,
                                        int64_t frames, int64_t units, int n, int nwords, int64_t first_frame, int m, Units src,
                                        hipStream_t s) {
    int grid = (int) std::min<int64_t>((frames * units + 3) / 4, 256 * 8);
    if (grid < 1) grid = 1;
    if (y_is_f64)
        hipLaunchKernelGGL((classify_kernel<double, Units>), dim3(grid), dim3(256), 0, s, (const double *) y, bits, ok, iters, frames,
                           units, n, nwords, first_frame, m, src);
    else
        hipLaunchKernelGGL((classify_kernel<float, Units>), dim3(grid), dim3(256), 0, s, (const float *) y, bits, ok, iters, frames, units,
                           n, nwords, first_frame, m, src);
    return hipGetLastError();
}

hipError_t classify_grid_launch(const void *y, int y_is_f64, const uint32_t *bits, const uint8_t *ok, const int32_t *iters,
                                int64_t frames, int64_t points, int n, int nwords, int64_t first_frame, const uint32_t *cw_packed,
                                int64_t n_cw, unsigned long long *counters, const int32_t *row_ptr, const int32_t *edge_var, int m,
                                hipStream_t s) {
    const PointUnits src{{cw_packed, n_cw, row_ptr, edge_var, counters}};
    return classify_units_launch(y, y_is_f64, bits, ok, iters, frames, points, n, nwords, first_frame, m, src, s);
}

hipError_t classify_codes_launch(const void *y, int y_is_f64, const uint32_t *bits, const uint8_t *ok, const int32_t *iters,
                                 int64_t frames, int64_t codes, int n, int nwords, int64_t first_frame, const CodeRef *refs, int m,
                                 hipStream_t s) {
    return classify_units_launch(y, y_is_f64, bits, ok, iters, frames, codes, n, nwords, first_frame, m, CodeUnits{refs}, s);
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

// ---- detail run (acg_ldpc_mc_run_detail) --------------------------------------------------------------------------------
// the bits < n of the last packed word of a frame
__device__ __forceinline__ uint32_t last_word_mask(int n) { return (n & 31) ? ((1u << (n & 31)) - 1u) : 0xFFFFFFFFu; }

// What one wavefront adds to classify_frame for the detail run: d_H(word, sent) with the bits >= n of the last word masked
// off, and, for decoders that pass a CSR (QP-ADMM), the number of unsatisfied checks.  Both are wave-uniform on return.
__device__ __forceinline__ void frame_detail(const uint32_t *bits, const uint32_t *cw, int n, int nwords, const int32_t *row_ptr,
                                             const int32_t *edge_var, int m, int lane, int &dist, int &synw) {
    const uint32_t last_mask = last_word_mask(n);
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

// classify_kernel for one unit plus the detail counters: one wavefront per frame, sums kept per wavefront, one set of atomics
// at the end.  counters: DET_NCOUNTERS words; [0, MC_NCOUNTERS) are the Tally's.  kind[f] = the frame's ACG_LDPC_EVENT_* or 0.
// counters[DET_MIN_PSEUDO] = min over the pseudo frames of (weight << 32 | chunk-relative frame): the lowest frame wins ties.
__global__ void classify_detail_kernel(const float *y, const uint32_t *bits, const uint8_t *ok, const int32_t *iters,
                                       int64_t frames, int n, int nwords, int64_t first_frame, const uint32_t *cw_packed,
                                       int64_t n_cw, unsigned long long *counters, uint8_t *kind, const int32_t *row_ptr,
                                       const int32_t *edge_var, int m) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nw = (int64_t) gridDim.x * (blockDim.x >> 6);
    Tally t;
    unsigned long long c_word = 0, c_be = 0, c_ncw = 0, c_syn = 0, c_minp = ~0ull;
    for (int64_t f = wid; f < frames; f += nw) {
        const uint32_t *cw = cw_packed ? cw_packed + (size_t) ((first_frame + f) % n_cw) * nwords : nullptr;
        const uint32_t *b = bits + (size_t) f * nwords;
        const bool flag = ok[f] != 0;
        int ham;
        bool correct, pseudo;
        classify_frame(y + (size_t) f * n, b, flag, cw, n, nwords, row_ptr, edge_var, m, lane, ham, correct, pseudo);
        t.add(correct, pseudo, ham, iters ? iters[f] : 0);
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
    if (lane == 0 && t.tot) {
        atomicAdd(&counters[DET_WORD_FRAMES], c_word);
        if (c_be) atomicAdd(&counters[DET_BIT_ERRORS], c_be);
        if (c_ncw) {
            atomicAdd(&counters[DET_NONCODEWORD], c_ncw);
            atomicAdd(&counters[DET_SYNDROME], c_syn);
        }
        if (c_minp != ~0ull) atomicMin(&counters[DET_MIN_PSEUDO], c_minp);
    }
    t.flush(counters);
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
    const uint32_t last_mask = last_word_mask(n);
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
