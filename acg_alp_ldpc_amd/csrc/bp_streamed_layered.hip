// Streamed float layered BP: sum-product and normalised min-sum with fp32 posteriors and fp32 messages, the per-check arithmetic
// of the workgroup-per-frame layered engines (bp_layer_math.inc; wide_layer_step of bp_layered_wide.hip) in the engine shape of
// bp_streamed_q.hip, so neither the size of a frame nor the degree of a check is bounded.  Reached through
// acg_ldpc_decoder_create_layered_streamed only.  tests/layered_ref.py restates it (layered_minsum, layered_sumproduct_exact).
//
// Mapping, as in bp_streamed_q.hip: ONE LANE IS ONE FRAME.  A wavefront — a workgroup of 64 threads — owns a tile of T = 64 frames
// and a slab of device memory:
//     P[v][T] fp32 posteriors | R[e][T] fp32 messages, edges in processing order | scratch of a wide sum-product check (below)
// so a wavefront's access to one variable or one edge is 256 consecutive bytes, and no lane reads another lane's data.
// The graph is a plain CSR of the checks in processing order — the sets of bp_layered_block_build without a degree cap, set by
// set — read through wave-uniform scalar loads.  The degree of a check is a loop bound.  Tiles are dealt by the launch's work
// counter; a slab belongs to a resident workgroup.
//
// A check of up to LMAXD = 8 variables is worked off in one pass with its cells in registers: layer_back / layer_back_spa of
// bp_layer_math.inc, the very functions of the LDS engines, with a message stride of T cells (16 bytes per edge and frame).  A
// wider one takes two passes in chunks of 8 edges, as wide_layer_step does, with any number of chunks:
//   pass 1, chunks ascending: q_j = p_j - r_j and the reductions over the whole check — min-sum: m1, m2; sum-product: mag_j =
//           phi(|q_j|) and ONE ascending sum of them, whose value at the start of every chunk goes to the scratch area; both: the
//           XOR of the signs of q and of p.  Nothing of P or R is written.
//   pass 2, chunks descending: p_j and r_j read again (the same bits: nothing of the check was written before all of it was
//           read, and what pass 2 writes belongs to chunks it has finished), q_j recomputed, the new message, p'_j = q_j + r'_j.
//           Sum-product: pre_j restarts from the chunk's saved prefix and adds the same mag in the same order as pass 1 did, so
//           it has the bits of one ascending sum over all D edges; suf runs on from chunk to chunk in descending edge order.
// mag_j of pass 2 is formed again from q_j — the same bits, phi being a pure function, at three phi per edge — so the scratch
// area holds the prefixes alone, base[ceil(Dmax / 8)][T].  Reading it back from a scratch area mag[Dmax][T] that pass 1 fills (two
// phi, 8 bytes more per edge; ACG_SL_STORE_MAG=1) was measured and was 12 to 18 % slower: DESIGN 3i.
//
// The tile loop — the claim of a tile, the iterations and the latch, the syndrome pass, the outputs — is streamed_tile_loop of
// bp_streamed_tile.inc, shared with bp_streamed_q.hip; "Control" and "No stale state" are written there.  Of this engine's own:
// a scratch cell is written by pass 1 of the check whose pass 2 reads it.
//
// The IO instances (acg_ldpc_decode_batch_llr*; StreamLayIo behind ws) differ in the two ends of a tile and in nothing between:
//   fill   a frame is n fp32 LLRs, positive = bit 0.  Per value: NaN -> +0; clamp to +-2^20 (exact in fp32, and +-inf stays out of
//          p - r); min-sum takes that, sum-product multiplies it ONCE by (float) Dom<float>::scale — the multiply the symbol
//          entrance applies to the LLR it forms.  So an LLR of at most 2^20 that the symbol entrance would have formed itself gives
//          the same slab, bit for bit, and with it the same word, flag and iteration.
//   drain  where post_out is set, the slab's P of the frames that exist, [n][T] -> [frame][n] through X: min-sum as it is,
//          sum-product times (float) ln 2 in ONE multiply, back to natural-log units.  The sign bit survives, -0 included.  A latched
//          lane writes nothing of P (the tile loop), so a frame that latched hands out the posteriors of the round boundary at which
//          its word was formed, whatever early_exit says; one that failed, those after max_iter iterations; max_iter = 0, the clamped
//          LLR (sum-product: scaled and scaled back, which need not be the input's bits).
// The symbol entrance's instances read no StreamLayIo and compile to what they compiled to without it.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "launchers.hpp"

namespace acg {
#include "bp_core.inc"   // Dom<float>::phi for the sum-product instance
#include "bp_layer_math.inc"
#include "bp_streamed_tile.inc"

// sum-product, wide checks: pass 2 forms mag_j again (0) or reads it back (1; make EXTRA=-DACG_SL_STORE_MAG=1, the build that
// tools/streamed_layered_rate.py measured this one against: DESIGN 3i)
#ifndef ACG_SL_STORE_MAG
#define ACG_SL_STORE_MAG 0
#endif
constexpr bool SL_STORE_MAG = ACG_SL_STORE_MAG != 0;

__device__ __forceinline__ uint32_t sl_bits(const float x) { return __float_as_uint(x); }
__device__ __forceinline__ float sl_abs(const float x) { return __uint_as_float(__float_as_uint(x) & 0x7FFFFFFFu); }

constexpr uint32_t SL_LLR_CLAMP = 0x49800000u;   // 2^20 as fp32 bits: the largest magnitude of an LLR of the IO instances

// ALGO: 1 = normalised min-sum, 0 = sum-product.  IO: the LLR entrance (io.llr_in in, io.post_out out) instead of the symbol
// entrance (a->y in, hard outputs only)
template <int ALGO, bool IO = false>
struct SlTile {
    float *P;            // this lane's posterior of variable v: P[(size_t) v * TILE_T]
    float *R;            // this lane's message of edge e: R[(size_t) e * TILE_T]
    float *M;            // this lane's scratch: mag of the j-th edge of the wide check under way, M[(size_t) j * TILE_T]
    float *B;            // ... and its prefix sum at the start of chunk c, B[(size_t) c * TILE_T]
    const int32_t *ev;
    float *X;            // the workgroup's transposing buffer: XV variables x T frames, rows of XS words
    const DecodeArgs *a; // the channel values and terms of fill()
    StreamLayIo io;      // IO: the LLRs of fill() and the posteriors of drain(); neither set nor read otherwise
    int n;
    float scale;
    static constexpr int XV = 32;           // variables of a trip through the transposing buffer
    static constexpr int XS = TILE_T + 1;   // words per row of it: rows an odd number of words apart
    bool first;     // the tile's first iteration: every message is 0 and R is not read
    bool live;       // the frame is updated: it exists and has not latched
    uint32_t loud;   // bit 0: some step of the iteration was not quiet for this frame

    // N edges from e: the addresses of this lane's posteriors, their values, and q = p - r
    template <int N>
    __device__ __forceinline__ void load(const size_t e, float *(&addr)[LMAXD], float (&p)[LMAXD], float (&q)[LMAXD]) const {
        float r[LMAXD];
#pragma unroll
        for (int j = 0; j < N; ++j) addr[j] = P + (size_t) lsload(ev, e + j) * TILE_T;
#pragma unroll
        for (int j = 0; j < N; ++j) p[j] = *addr[j];
#pragma unroll
        for (int j = 0; j < N; ++j) r[j] = first ? 0.0f : R[(e + j) * TILE_T];
#pragma unroll
        for (int j = 0; j < N; ++j) q[j] = p[j] - r[j];
    }

    // a check of D <= 8 edges from e: the step of the LDS engines
    template <int D>
    __device__ __forceinline__ void small_check(const size_t e) {
        float *addr[LMAXD];
        float p[LMAXD], q[LMAXD];
        load<D>(e, addr, p, q);
        uint32_t noisy;
        if constexpr (ALGO == 0) noisy = layer_back_spa<D, TILE_T, float>(R + e * TILE_T, addr, p, q, live);
        else noisy = layer_back<D, TILE_T, float>(R + e * TILE_T, addr, p, q, live, scale);
        loud |= noisy >> 31;
    }

    // what pass 1 hands to pass 2 in registers
    struct Wide {
        uint32_t S = 0, parity = 0, flipped = 0;
        float m1 = INFINITY, m2 = INFINITY;   // min-sum
        uint32_t m1s = 0, m2s = 0;
        float s = 0.0f, suf = 0.0f;           // sum-product: the ascending sum so far, the descending one
    };

    // chunk c of a wide check: its N edges from e, the first of them edge number j0 = 8 c of the check
    template <int N>
    __device__ __forceinline__ void pass1(Wide &w, const size_t e, const int c) const {
        float *addr[LMAXD];
        float p[LMAXD], q[LMAXD];
        load<N>(e, addr, p, q);
        if constexpr (ALGO == 0) B[(size_t) c * TILE_T] = w.s;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            w.parity ^= sl_bits(p[j]);                      // parity of the hard decisions this check sees
            w.S ^= sl_bits(q[j]);
            const float a = sl_abs(q[j]);
            if constexpr (ALGO == 0) {
                const float m = Dom<float>::phi(a);
                if constexpr (SL_STORE_MAG) M[(size_t) (c * LMAXD + j) * TILE_T] = m;
                w.s += m;
            } else {
                w.m2 = __builtin_amdgcn_fmed3f(a, w.m1, w.m2);
                w.m1 = __builtin_fminf(w.m1, a);
            }
        }
    }
    template <int N>
    __device__ __forceinline__ void pass2(Wide &w, const size_t e, const int c) {
        float *addr[LMAXD];
        float p[LMAXD], q[LMAXD];
        load<N>(e, addr, p, q);
        float mag[LMAXD], pre[LMAXD];
        if constexpr (ALGO == 0) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                if constexpr (SL_STORE_MAG) mag[j] = M[(size_t) (c * LMAXD + j) * TILE_T];
                else mag[j] = Dom<float>::phi(sl_abs(q[j]));
            }
            float t = B[(size_t) c * TILE_T];
#pragma unroll
            for (int j = 0; j < N; ++j) {
                pre[j] = t;
                t += mag[j];
            }
        }
        float rn[LMAXD], pn[LMAXD];
#pragma unroll
        for (int j = N - 1; j >= 0; --j) {
            uint32_t mg;
            if constexpr (ALGO == 0) {
                const float out = __builtin_fminf(Dom<float>::phi(pre[j] + w.suf), LAYERED_SPA_SATURATION);
                w.suf += mag[j];
                mg = sl_bits(out) & 0x7FFFFFFFu;
            } else {
                mg = (sl_abs(q[j]) == w.m1) ? w.m2s : w.m1s;     // a tie makes m2 == m1: either answer is the same
            }
            rn[j] = __uint_as_float(mg | ((w.S ^ sl_bits(q[j])) & 0x80000000u));
            pn[j] = q[j] + rn[j];
            w.flipped |= sl_bits(pn[j]) ^ sl_bits(p[j]);         // a hard decision flipped
        }
        if (live) {
#pragma unroll
            for (int j = 0; j < N; ++j) *addr[j] = pn[j];
#pragma unroll
            for (int j = 0; j < N; ++j) R[(e + j) * TILE_T] = rn[j];
        }
    }

    // the check of the edges [e0, e1), e1 > e0 (wave-uniform)
    __device__ __forceinline__ void check(const size_t e0, const size_t e1) {
        const int D = (int) (e1 - e0);
        if (D <= LMAXD) {
#define ACG_CALL(N) small_check<N>(e0)
            ACG_LAYER_SWITCH(D, ACG_CALL)
#undef ACG_CALL
            return;
        }
        Wide w;
        const int full = D / LMAXD, tail = D - full * LMAXD;   // chunks of 8 edges, and the edges of the last, shorter one
        const size_t et = e0 + (size_t) full * LMAXD;
        for (int c = 0; c < full; ++c) pass1<LMAXD>(w, e0 + (size_t) c * LMAXD, c);
#define ACG_CALL(N) pass1<N>(w, et, full)
        ACG_TILE_TAIL(tail, ACG_CALL)
#undef ACG_CALL
        // the two minima are scaled once per check (layer_back; D > 8, so no one-variable check here)
        if constexpr (ALGO == 1) {
            w.m1s = sl_bits(scale * w.m1) & 0x7FFFFFFFu;
            w.m2s = sl_bits(scale * w.m2) & 0x7FFFFFFFu;
            asm volatile("" : "+v"(w.m1s), "+v"(w.m2s));
        }
#define ACG_CALL(N) pass2<N>(w, et, full)
        ACG_TILE_TAIL(tail, ACG_CALL)
#undef ACG_CALL
        for (int c = full - 1; c >= 0; --c) pass2<LMAXD>(w, e0 + (size_t) c * LMAXD, c);
        loud |= (w.parity | w.flipped) >> 31;
    }

    __device__ __forceinline__ uint32_t sign(const int v) const { return sl_bits(P[(size_t) v * TILE_T]); }

    // start of the tile: P = channel LLR (channel.h:14-16), [frame][n] -> [n][T] through LDS, 32 variables at a time; a lane takes
    // one variable of every second frame
    __device__ __forceinline__ void fill(const int64_t frame0, const int nf) {
        constexpr int T = TILE_T;
        const int l = threadIdx.x;
        for (int v0 = 0; v0 < n; v0 += XV) {
            const int vl = l & (XV - 1), h = l / XV;
            const bool mine = v0 + vl < n;
            const size_t y0 = (size_t) frame0 * n + v0 + vl;
#pragma unroll 8
            for (int k = 0; k < T / 2; ++k) {
                const int fr = 2 * k + h;
                float x = 0.0f;
                if (fr < nf && mine) {
                    float llr;
                    if constexpr (IO) {
                        // NaN -> +0, then clamp to +-2^20, both on the bits: no rounding and no floating-point mode takes part
                        const uint32_t u = sl_bits(io.llr_in[y0 + (size_t) fr * n]), m = u & 0x7FFFFFFFu;
                        llr = __uint_as_float(m > 0x7F800000u ? 0u : (m > SL_LLR_CLAMP ? (u & 0x80000000u) | SL_LLR_CLAMP : u));
                    } else if (a->y_is_f64) llr = (float) (2 * reinterpret_cast<const double *>(a->y)[y0 + (size_t) fr * n] / a->var);
                    else llr = (float) ((double) reinterpret_cast<const float *>(a->y)[y0 + (size_t) fr * n] * a->inv_var2);
                    x = (ALGO == 0) ? llr * (float) Dom<float>::scale : llr;
                }
                X[vl * XS + fr] = x;
            }
            __syncthreads();
            const int nv = n - v0 < XV ? n - v0 : XV;
            for (int vv = 0; vv < nv; ++vv) P[(size_t) (v0 + vv) * T] = X[vv * XS + l];
            __syncthreads();
        }
    }
    // end of the tile.  IO: its posteriors, [n][T] -> [frame][n] through LDS, the mirror image of fill(): the same cells of X
    // written by rows and read by columns, so neither side meets a bank conflict; frames that exist and variables below n only
    __device__ __forceinline__ void drain(const int64_t frame0, const int nf) {
        if constexpr (IO) {
            constexpr int T = TILE_T;
            const int l = threadIdx.x;
            if (!io.post_out) return;
            for (int v0 = 0; v0 < n; v0 += XV) {
                const int nv = n - v0 < XV ? n - v0 : XV;
                for (int vv = 0; vv < nv; ++vv) X[vv * XS + l] = P[(size_t) (v0 + vv) * T];
                __syncthreads();
                const int vl = l & (XV - 1), h = l / XV;
                const bool mine = v0 + vl < n;
                const size_t y0 = (size_t) frame0 * n + v0 + vl;
#pragma unroll 8
                for (int k = 0; k < T / 2; ++k) {
                    const int fr = 2 * k + h;
                    if (fr < nf && mine) {
                        const float p = X[vl * XS + fr];
                        io.post_out[y0 + (size_t) fr * n] = (ALGO == 0) ? p * (float) 0.6931471805599453 : p;
                    }
                }
                __syncthreads();
            }
        }
        // (otherwise: hard outputs only)
    }
};

// grid <= the slabs behind ws.  Io: nothing (the symbol entrance's instances), or one StreamLayIo (the IO instances)
template <int ALGO, typename... Io>
__global__ void __launch_bounds__(64) bp_streamed_layered_kernel(const StreamLayTables t, const DecodeArgs a, unsigned char *__restrict__ ws, const Io... io) {
    constexpr int T = TILE_T;
    constexpr bool IO = sizeof...(Io) != 0;
    static_assert(!IO || (sizeof...(Io) == 1 && (std::is_same<Io, StreamLayIo>::value && ...)), "the IO instances: one StreamLayIo behind ws");
    using Tile = SlTile<ALGO, IO>;
    __shared__ float X[Tile::XV * Tile::XS];
    const int l = threadIdx.x;
    float *const slab = reinterpret_cast<float *>(ws + (size_t) blockIdx.x * (size_t) t.slab_bytes);
    Tile tl;
    tl.P = slab + l;
    tl.R = tl.P + (size_t) t.n * T;
    tl.M = tl.R + (size_t) t.E * T;
    tl.B = SL_STORE_MAG ? tl.M + (size_t) t.max_deg * T : tl.M;
    tl.ev = t.edge_var;
    tl.X = X;
    tl.a = &a;
    tl.n = t.n;
    tl.scale = a.ms_scale;
    if constexpr (IO) tl.io = (io, ...);
    streamed_tile_loop(t, a, tl);
}

// algo: 0 sum-product, 1 min-sum
const void *bp_streamed_layered_kernel_ptr(int algo, bool io) {
    if (io) return algo == 0 ? (const void *) bp_streamed_layered_kernel<0, StreamLayIo> : (const void *) bp_streamed_layered_kernel<1, StreamLayIo>;
    return algo == 0 ? (const void *) bp_streamed_layered_kernel<0> : (const void *) bp_streamed_layered_kernel<1>;
}

// floats per frame behind P and R: the scratch of a wide sum-product check (0: the code has none, or min-sum)
size_t bp_streamed_layered_scratch_words(int algo, int max_deg) {
    if (algo != 0 || max_deg <= LMAXD) return 0;
    return (size_t) (SL_STORE_MAG ? max_deg : 0) + (size_t) (max_deg + LMAXD - 1) / LMAXD;
}
bool bp_streamed_layered_stores_mag() { return SL_STORE_MAG; }

hipError_t bp_streamed_layered_launch(const void *kernel, const StreamLayTables &t, const DecodeArgs &a, const QuantArgs *q, unsigned char *ws,
                                      int grid, hipStream_t s, const StreamLayIo *io) {
    void *args[5];
    int k = 0;
    args[k++] = (void *) &t;
    args[k++] = (void *) &a;
    if (q) args[k++] = (void *) q;
    args[k++] = (void *) &ws;
    if (io) args[k++] = (void *) io;
    return hipLaunchKernel(kernel, dim3((unsigned) grid), dim3(64), args, 0, s);
}

}  // namespace acg
