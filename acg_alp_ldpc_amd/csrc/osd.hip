// Ordered-statistics decoding (Fossorier–Lin), order 0 and 1, on int16 soft values: one workgroup of L = 64, 128 or 256
// threads owns a frame, and everything the frame needs lives in LDS.  Every value is an integer, so tests/osd_ref.py restates
// the algorithm and word, flag and iters of every frame are equal.  The algorithm (include/acg_ldpc.h, ACG_LDPC_OSD):
//
//   z_v = (s_v < 0), r_v = min(|s_v|, 32767), key_v = r_v << 16 | v.  The variables are scanned in ascending key; v joins the
//   pivot set B iff column v of H is independent of the columns already in B.  With H reduced so that the pivot columns are unit
//   vectors, sigma = H_red z, and the codeword that agrees with z on the complement I of B except on T (empty, or one j of I)
//   has metric M = [T = {j}] r_j + sum_r (sigma_r ^ [T = {j}] H_red[r][j]) r_piv(r).  Order 0 returns T = {}, order 1 the
//   minimiser over {} and every j of I (ties: {} first, then the lowest j).
//
// LDS of the workgroup (32-bit words): W[n][stride] the working matrix, column-major, stride = ceil(m / 32) made odd, so lane j
// reading word w of column j meets no bank conflict | K[n] the keys | PERM[n] the variables in ascending key | PROW[n] the pivot
// row of a column, -1 for a column of I | RROW[32 Wm] r of the pivot column of a row, 0 for a row without pivot | FR[2][Wm]
// the rows not yet used, double-buffered over the pivots | SG[Wm] sigma | Z[nwords] the hard decisions | OB[nwords] the word.
//
// The matrix comes per frame from one packed table in device memory (OsdArgs::cols, n * stride words: every workgroup reads the
// same table, it stays in L2).  The order is total, so rank-by-counting (n^2 compares of LDS words that every lane reads at the
// same address) gives the one permutation.  Elimination walks the columns in that order: a column whose words, masked by the
// free rows, are all zero is dependent — every lane reads the same words, the decision is uniform and costs no barrier; else
// its lowest free bit p is the pivot row, every other column with bit p set XORs in the pivot column with bit p cleared (one
// thread per column), and ONE barrier ends the pivot: the free-row mask of the next pivot is written to the other buffer in the
// same phase.  The pivot columns themselves are left as they are until the walk is over (nothing reads them again) and are
// then set to their unit vectors.  Every loop bound is known at launch: n columns, rank pivots, Wm words.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "launchers.hpp"

namespace acg {

// the symbol entrance's quantiser: clamp(truncf((float) y * 4096), +-32767), NaN -> 0
__device__ __forceinline__ int osd_soft_value(const void *y, const int y_is_f64, const size_t i) {
    const float y32 = y_is_f64 ? (float) reinterpret_cast<const double *>(y)[i] : reinterpret_cast<const float *>(y)[i];
    const float t = y32 * 4096.0f;
    if (t != t) return 0;
    return (int) fminf(fmaxf(t, -32767.0f), 32767.0f);   // (the conversion truncates toward zero)
}

template <int L>
__global__ void __launch_bounds__(L) osd_kernel(const OsdArgs o, const DecodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned long long fr_lds, best_lds;
    __shared__ uint32_t m0_lds;
    const int l = threadIdx.x, lane = l & 63;
    const int n = o.n, m = o.m, wm = o.wm, stride = o.stride, nwords = o.nwords;
    uint32_t *W = reinterpret_cast<uint32_t *>(smem);
    uint32_t *K = W + (size_t) n * stride;
    uint32_t *PERM = K + n;
    int32_t *PROW = reinterpret_cast<int32_t *>(PERM + n);
    uint32_t *RROW = reinterpret_cast<uint32_t *>(PROW + n);
    uint32_t *FR = RROW + 32 * wm;
    uint32_t *SG = FR + 2 * wm;
    uint32_t *Z = SG + wm;
    uint32_t *OB = Z + nwords;

    for (;;) {
        __syncthreads();
        if (l == 0) {
            fr_lds = atomicAdd(a.work_counter, 1ull);
            best_lds = ~0ull;
            m0_lds = 0u;
        }
        __syncthreads();
        const int64_t frame = (int64_t) fr_lds;
        if (frame >= a.frames) break;
        // ---- the frame's soft values -> keys and hard decisions; the matrix; the bookkeeping -------------------------------
        // (64 variables per wavefront and trip: the wavefronts' chunks are 64-aligned, so no two write the same word of Z)
        for (int v0 = l & ~63; v0 < n; v0 += L) {
            const int v = v0 + lane;
            int s = 0;
            if (v < n) s = o.s_in ? (int) o.s_in[(size_t) frame * n + v] : osd_soft_value(a.y, a.y_is_f64, (size_t) frame * n + v);
            const unsigned long long b = __ballot(v < n && s < 0);
            if (v < n) {
                const int r = min(s < 0 ? -s : s, 32767);
                K[v] = (uint32_t) r << 16 | (uint32_t) v;
                PROW[v] = -1;
            }
            if (lane == 0) {
                Z[v0 >> 5] = (uint32_t) b;
                if ((v0 >> 5) + 1 < nwords) Z[(v0 >> 5) + 1] = (uint32_t) (b >> 32);
            }
        }
        for (int i = l; i < n * stride; i += L) W[i] = o.cols[i];
        for (int i = l; i < 32 * wm; i += L) RROW[i] = 0u;
        for (int w = l; w < wm; w += L) {
            const int left = m - 32 * w;   // rows of word w: >= 1
            FR[w] = left >= 32 ? 0xFFFFFFFFu : (1u << left) - 1u;
            SG[w] = 0u;
        }
        __syncthreads();
        // ---- PERM: rank by counting -------------------------------------------------------------------------------------------
        for (int v = l; v < n; v += L) {
            const uint32_t kv = K[v];
            int cnt = 0;
            for (int u = 0; u < n; ++u) cnt += K[u] < kv ? 1 : 0;
            PERM[cnt] = (uint32_t) v;
        }
        __syncthreads();
        // ---- the pivot set: at most `rank` pivots, one barrier each ---------------------------------------------------------------
        int k = 0, buf = 0;
        for (int t = 0; t < n && k < o.rank; ++t) {
            const int c = (int) PERM[t];
            const uint32_t *col = W + (size_t) c * stride;
            const uint32_t *fr = FR + buf * wm;
            int p = -1;
            for (int w = 0; w < wm; ++w) {
                const uint32_t x = col[w] & fr[w];
                if (x) {
                    p = 32 * w + __builtin_ctz(x);
                    break;
                }
            }
            p = __builtin_amdgcn_readfirstlane(p);   // (every lane read the same words)
            if (p < 0) continue;
            const int pw = p >> 5;
            const uint32_t pb = 1u << (p & 31);
            for (int j = l; j < n; j += L) {
                uint32_t *cj = W + (size_t) j * stride;
                if (j != c && (cj[pw] & pb)) {
                    for (int w = 0; w < wm; ++w) cj[w] ^= w == pw ? col[w] & ~pb : col[w];
                }
            }
            for (int w = l; w < wm; w += L) FR[(buf ^ 1) * wm + w] = fr[w] & (w == pw ? ~pb : 0xFFFFFFFFu);
            if (l == 0) {
                PROW[c] = p;
                RROW[p] = K[c] >> 16;
            }
            buf ^= 1;
            k += 1;
            __syncthreads();
        }
        // ---- the pivot columns become their unit vectors ------------------------------------------------------------------------
        for (int v = l; v < n; v += L) {
            const int p = PROW[v];
            if (p >= 0)
                for (int w = 0; w < wm; ++w) W[(size_t) v * stride + w] = w == (p >> 5) ? 1u << (p & 31) : 0u;
        }
        __syncthreads();
        // ---- sigma = H_red z ------------------------------------------------------------------------------------------------------
        for (int v = l; v < n; v += L) {
            if ((Z[v >> 5] >> (v & 31)) & 1u)
                for (int w = 0; w < wm; ++w) {
                    const uint32_t x = W[(size_t) v * stride + w];
                    if (x) atomicXor(&SG[w], x);
                }
        }
        __syncthreads();
        // ---- M(x_{}) = sum of the pivot reliabilities of the rows of sigma (a row without pivot has RROW = 0) --------------------
        {
            uint32_t part = 0;
            for (int r = l; r < 32 * wm; r += L) part += ((SG[r >> 5] >> (r & 31)) & 1u) ? RROW[r] : 0u;
            for (int d = 32; d > 0; d >>= 1) part += __shfl_down(part, d, 64);
            if (lane == 0 && part) atomicAdd(&m0_lds, part);
        }
        __syncthreads();
        // ---- order 1: the minimum of metric << 32 | (j + 1), 0 in the low half standing for T = {} --------------------------------
        unsigned long long best = (unsigned long long) m0_lds << 32;
        if (o.order >= 1) {
            for (int j = l; j < n; j += L) {
                if (PROW[j] >= 0) continue;
                uint32_t M = K[j] >> 16;
                for (int w = 0; w < wm; ++w) {
                    uint32_t x = SG[w] ^ W[(size_t) j * stride + w];
                    while (x) {
                        M += RROW[32 * w + __builtin_ctz(x)];
                        x &= x - 1u;
                    }
                }
                const unsigned long long key = (unsigned long long) M << 32 | (uint32_t) (j + 1);
                best = key < best ? key : best;
            }
            for (int d = 32; d > 0; d >>= 1) {
                const unsigned long long other = __shfl_down(best, d, 64);
                best = other < best ? other : best;
            }
            if (lane == 0) atomicMin(&best_lds, best);
            __syncthreads();
            best = best_lds;
        }
        const int jstar = (int) (uint32_t) (best & 0xFFFFFFFFull) - 1;   // -1: T = {}
        // ---- the word: z on I (with j* flipped), z ^ sigma ^ H_red[.][j*] on the pivots ---------------------------------------------
        for (int v0 = l & ~63; v0 < n; v0 += L) {
            const int v = v0 + lane;
            uint32_t bit = 0;
            if (v < n) {
                bit = (Z[v >> 5] >> (v & 31)) & 1u;
                const int p = PROW[v];
                if (p < 0) {
                    bit ^= v == jstar ? 1u : 0u;
                } else {
                    bit ^= (SG[p >> 5] >> (p & 31)) & 1u;
                    if (jstar >= 0) bit ^= (W[(size_t) jstar * stride + (p >> 5)] >> (p & 31)) & 1u;
                }
            }
            const unsigned long long b = __ballot(bit != 0u);
            if (lane == 0) {
                OB[v0 >> 5] = (uint32_t) b;
                if ((v0 >> 5) + 1 < nwords) OB[(v0 >> 5) + 1] = (uint32_t) (b >> 32);
            }
        }
        __syncthreads();
        if (a.out_bits)
            for (int w = l; w < nwords; w += L) a.out_bits[(size_t) frame * nwords + w] = OB[w];
        if (l == 0) {
            if (a.out_ok) a.out_ok[frame] = 1;
            if (a.out_iters) a.out_iters[frame] = jstar >= 0 ? 1 : 0;
        }
    }
}

const void *osd_kernel_ptr(int L) {
    switch (L) {
        case 64: return (const void *) osd_kernel<64>;
        case 128: return (const void *) osd_kernel<128>;
        case 256: return (const void *) osd_kernel<256>;
        default: return nullptr;
    }
}

size_t osd_lds_bytes(int n, int m) {
    const size_t wm = (size_t) (m + 31) / 32, stride = wm | 1, nwords = (size_t) (n + 31) / 32;
    return 4 * ((size_t) n * stride + 3 * (size_t) n + 32 * wm + 3 * wm + 2 * nwords);
}

hipError_t osd_launch(const void *kernel, const OsdArgs &o, const DecodeArgs &a, int grid, int block, size_t lds, hipStream_t s) {
    OsdArgs oo = o;
    DecodeArgs aa = a;
    void *args[2] = {&oo, &aa};
    return hipLaunchKernel(kernel, dim3(grid), dim3(block), args, lds, s);
}

// acg_ldpc_debug_osd_soft: the device function the kernel calls, on a plain array of symbols
__global__ void __launch_bounds__(256) osd_soft_debug_kernel(const void *y, const int y_is_f64, const int64_t count, int16_t *__restrict__ out) {
    for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t) gridDim.x * 256) out[i] = (int16_t) osd_soft_value(y, y_is_f64, (size_t) i);
}

hipError_t osd_soft_debug_launch(const void *y, int y_is_f64, int64_t count, int16_t *out, hipStream_t s) {
    const int grid = (int) std::max<int64_t>(1, std::min<int64_t>((count + 255) / 256, 4096));
    hipLaunchKernelGGL(osd_soft_debug_kernel, dim3(grid), dim3(256), 0, s, y, y_is_f64, count, out);
    return hipGetLastError();
}

}  // namespace acg
