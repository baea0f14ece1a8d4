// Monte-Carlo kernels for punctured and shortened codes on gfx950 (MI355X; acg_ldpc_mc_run_rm, include/acg_ldpc.h): the generator
// of channel values — noise, symbol, LLR or quantised value and the frame's raw-error count in one pass, no symbol buffer — and
// the classifier that takes that count in place of a Hamming count over symbols.  Philox / Box-Muller are bp_core.inc's own,
// the sums of a wavefront mc_tally.inc's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "launchers.hpp"

namespace acg {
#include "bp_core.inc"
#include "mc_tally.inc"

constexpr float RM_LLR_KNOWN = 1048576.0f;  // a shortened position on a float handle: the LLR entrance's clamp, 2^20

// the symbol entrance's channel LLR of a float symbol (bp_streamed_layered.hip, bp_layered_q.hip: quantize_symbol)
__device__ __forceinline__ float rm_llr(const float y, const double inv_var2) { return (float) ((double) y * inv_var2); }

// the channel value of one position.  state: ACG_LDPC_RM_*; bit: the sent bit
template <typename Out>
__device__ __forceinline__ Out rm_value(float y, uint32_t state, uint32_t bit, double inv_var2, const QuantArgs &qa);
template <>
__device__ __forceinline__ float rm_value<float>(const float y, const uint32_t state, const uint32_t bit, const double inv_var2,
                                                 const QuantArgs &) {
    if (state == ACG_LDPC_RM_SENT) return rm_llr(y, inv_var2);
    if (state == ACG_LDPC_RM_PUNCTURED) return 0.0f;
    return bit ? -RM_LLR_KNOWN : RM_LLR_KNOWN;
}
template <>
__device__ __forceinline__ int16_t rm_value<int16_t>(const float y, const uint32_t state, const uint32_t bit, const double inv_var2,
                                                     const QuantArgs &qa) {
    if (state == ACG_LDPC_RM_PUNCTURED) return 0;
    if (state != ACG_LDPC_RM_SENT) return (int16_t) (bit ? -qa.cmax : qa.cmax);
    // quantize_symbol (bp_layered_q.hip) on a float symbol: ONE fp32 multiply, round half to even, NaN -> 0, clamp
    const float t = rm_llr(y, inv_var2) * qa.inv_step;
    if (__builtin_isnan(t)) return 0;
    const float cm = (float) qa.cmax;
    return (int16_t) (int) __builtin_fminf(__builtin_fmaxf(__builtin_rintf(t), -cm), cm);
}

template <typename Out>
struct RmQuad;  // the four values of a quad as one store
template <>
struct RmQuad<float> {
    typedef float type __attribute__((ext_vector_type(4)));
};
template <>
struct RmQuad<int16_t> {
    typedef short type __attribute__((ext_vector_type(4)));
};

// A lane takes quad q of frame f, as awgn_kernel does: the same Philox call, the same fma, the same store addresses, with the
// symbol kept in a register.  VEC (n % 4 == 0 and `out` aligned to a quad): the four values leave as one 16- or 8-byte store;
// otherwise one scalar store per position < n.  pattern == null: every position sent.  raw != null (zeroed by the launcher): the
// errors of the sent positions are counted per frame.  The lanes of a wavefront hold consecutive quads, so the frames it
// touches are runs of lanes: four ballots give every lane the error bits of the whole wavefront, the first lane of a run
// counts those of its run and adds them to raw[f] with ONE atomic per (wavefront, frame); an integer sum, so the order of the
// wavefronts that share a frame does not show.
template <typename Out, bool VEC>
__global__ void __launch_bounds__(256) rm_channel_kernel(Out *__restrict__ out, int32_t *__restrict__ raw, const int64_t frames, const int n,
                                                         const int nwords, const int64_t first_frame, const uint64_t seed,
                                                         const uint32_t *__restrict__ cw_packed, const int64_t n_cw, const float sigma,
                                                         const double inv_var2, const uint8_t *__restrict__ pattern, const QuantArgs qa) {
    const int nq = (n + 3) >> 2;
    const int64_t total = frames * nq;
    const int lane = threadIdx.x & 63;
    // (every lane of a wavefront runs the same number of rounds: the ballots below need them all)
    for (int64_t base = (int64_t) blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < total; base += (int64_t) gridDim.x * blockDim.x) {
        const int64_t i = base + lane;
        const bool active = i < total;
        const int64_t f = active ? i / nq : -1;
        uint32_t err = 0;  // bit e: position 4q + e was sent and arrived on the wrong side of 0
        if (active) {
            const int q = (int) (i - f * nq);
            const int64_t gf = first_frame + f;
            uint32_t r[4];
            philox4x32_10((uint32_t) gf, (uint32_t) (gf >> 32), (uint32_t) q, 0u, (uint32_t) seed, (uint32_t) (seed >> 32), r);
            float z[4];
            box_muller(r[0], r[1], z[0], z[1]);
            box_muller(r[2], r[3], z[2], z[3]);
            // the quad's four sent bits lie in one packed word (4q % 32 <= 28), its four states in one aligned word where VEC
            const uint32_t bits4 = cw_packed ? (cw_packed[(size_t) (gf % n_cw) * nwords + (q >> 3)] >> ((q & 7) * 4)) & 0xFu : 0u;
            uint32_t st4 = 0;
            if (pattern) {
                if (VEC) {
                    st4 = reinterpret_cast<const uint32_t *>(pattern)[q];
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (4 * q + e < n) st4 |= (uint32_t) pattern[4 * q + e] << (8 * e);
                }
            }
            Out val[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t bit = (bits4 >> e) & 1u, state = (st4 >> (8 * e)) & 0xFFu;
                const float y = __builtin_fmaf(sigma, z[e], bit ? -1.0f : 1.0f);  // awgn_kernel's symbol, bit for bit
                val[e] = rm_value<Out>(y, state, bit, inv_var2, qa);
                const bool wrong = bit ? y > 0.0f : y <= 0.0f;   // classify_frame's rule
                if (state == ACG_LDPC_RM_SENT && wrong && (VEC || 4 * q + e < n)) err |= 1u << e;
            }
            Out *o = out + (size_t) f * n + 4 * q;
            if (VEC) {
                typename RmQuad<Out>::type v4 = {val[0], val[1], val[2], val[3]};
                *reinterpret_cast<typename RmQuad<Out>::type *>(o) = v4;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * q + e < n) o[e] = val[e];
            }
        }
        if (raw) {
            const unsigned long long e0 = __ballot(err & 1u), e1 = __ballot(err & 2u), e2 = __ballot(err & 4u), e3 = __ballot(err & 8u);
            const int f_low = (int) f, f_prev = __shfl_up(f_low, 1, 64);   // (neighbouring lanes: equal frames or consecutive ones)
            const bool head = active && (lane == 0 || f_low != f_prev);
            const unsigned long long heads = __ballot(head);
            if (head) {
                // this run: lanes [lane, next head); lanes past `total` carry no error bits
                const unsigned long long above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
                const unsigned long long upto = above ? (above & (0ull - above)) - 1ull : ~0ull;   // the lanes below the next head
                const unsigned long long run = upto & (~0ull << lane);
                const int cnt = __popcll(e0 & run) + __popcll(e1 & run) + __popcll(e2 & run) + __popcll(e3 & run);
                if (cnt) atomicAdd(&raw[f], cnt);
            }
        }
    }
}

template <typename Out>
static hipError_t rm_channel_launch_as(Out *out, const QuantArgs &qa, int32_t *raw, int64_t frames, int n, int nwords, int64_t first_frame,
                                       uint64_t seed, const uint32_t *cw_packed, int64_t n_cw, float sigma, double inv_var2,
                                       const uint8_t *pattern, hipStream_t s) {
    const int64_t total = frames * ((n + 3) >> 2);
    int grid = (int) std::min<int64_t>((total + 255) / 256, 256 * 16);   // awgn_launch's
    if (grid < 1) grid = 1;
    const bool vec = n % 4 == 0 && reinterpret_cast<uintptr_t>(out) % (4 * sizeof(Out)) == 0 && reinterpret_cast<uintptr_t>(pattern) % 4 == 0;
    if (vec)
        hipLaunchKernelGGL((rm_channel_kernel<Out, true>), dim3(grid), dim3(256), 0, s, out, raw, frames, n, nwords, first_frame, seed, cw_packed,
                           n_cw, sigma, inv_var2, pattern, qa);
    else
        hipLaunchKernelGGL((rm_channel_kernel<Out, false>), dim3(grid), dim3(256), 0, s, out, raw, frames, n, nwords, first_frame, seed, cw_packed,
                           n_cw, sigma, inv_var2, pattern, qa);
    return hipGetLastError();
}

hipError_t rm_channel_launch(void *out, const QuantArgs *q, int32_t *raw, int64_t frames, int n, int nwords, int64_t first_frame,
                             uint64_t seed, const uint32_t *cw_packed, int64_t n_cw, float sigma, double inv_var2, const uint8_t *pattern,
                             hipStream_t s) {
    if (frames <= 0) return hipSuccess;
    if (raw) {
        const hipError_t e = hipMemsetAsync(raw, 0, (size_t) frames * sizeof(int32_t), s);
        if (e != hipSuccess) return e;
    }
    if (q) return rm_channel_launch_as(static_cast<int16_t *>(out), *q, raw, frames, n, nwords, first_frame, seed, cw_packed, n_cw, sigma, inv_var2, pattern, s);
    return rm_channel_launch_as(static_cast<float *>(out), QuantArgs{}, raw, frames, n, nwords, first_frame, seed, cw_packed, n_cw, sigma, inv_var2, pattern, s);
}

// Classification for a rate-matched run: one wavefront per frame and a contiguous run of frames per wavefront, as classify_kernel
// with PointUnits and one unit, but the raw-channel figure is raw[f] (rm_channel_kernel's count over the sent positions) and no
// symbol is read.  correct <=> ok and the word equals the sent one on all n positions (the bits >= n of the last word do not count).
__global__ void __launch_bounds__(256) classify_rm_kernel(const int32_t *__restrict__ raw, const uint32_t *__restrict__ bits,
                                                          const uint8_t *__restrict__ ok, const int32_t *__restrict__ iters, const int64_t frames,
                                                          const int n, const int nwords, const int64_t first_frame,
                                                          const uint32_t *__restrict__ cw_packed, const int64_t n_cw,
                                                          unsigned long long *counters) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t) blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t nw = (int64_t) gridDim.x * (blockDim.x >> 6);
    const int64_t per = (frames + nw - 1) / nw;
    const int64_t f0 = wid * per, f1 = f0 + per < frames ? f0 + per : frames;
    const uint32_t last_mask = (n & 31) ? ((1u << (n & 31)) - 1u) : 0xFFFFFFFFu;
    Tally t;
    for (int64_t f = f0; f < f1; ++f) {
        const uint32_t *cw = cw_packed ? cw_packed + (size_t) ((first_frame + f) % n_cw) * nwords : nullptr;
        const uint32_t *b = bits + (size_t) f * nwords;
        bool neq = false;
        for (int w = lane; w < nwords; w += 64) neq |= ((b[w] ^ (cw ? cw[w] : 0u)) & (w == nwords - 1 ? last_mask : 0xFFFFFFFFu)) != 0u;
        const bool differ = __ballot(neq) != 0ull;
        const bool okf = ok[f] != 0;
        t.add(okf && !differ, okf && differ, raw[f], iters ? iters[f] : 0);
    }
    t.flush(counters);
}

hipError_t classify_rm_launch(const int32_t *raw, const uint32_t *bits, const uint8_t *ok, const int32_t *iters, int64_t frames, int n,
                              int nwords, int64_t first_frame, const uint32_t *cw_packed, int64_t n_cw, unsigned long long *counters,
                              hipStream_t s) {
    if (frames <= 0) return hipSuccess;
    const int grid = (int) std::min<int64_t>((frames + 3) / 4, 256 * 8);   // classify_units_launch's
    hipLaunchKernelGGL(classify_rm_kernel, dim3(grid), dim3(256), 0, s, raw, bits, ok, iters, frames, n, nwords, first_frame, cw_packed, n_cw,
                       counters);
    return hipGetLastError();
}

}  // namespace acg
