// Streamed fixed-point layered min-sum: the arithmetic and the control of bp_layered_q.hip (acg_ldpc_quant, include/acg_ldpc.h;
// quant_arith.hpp) with a frame's state in device memory instead of LDS, so neither the size of a frame nor the degree of a
// check is bounded.  Reached through acg_ldpc_decoder_create_quantized_streamed only.  tests/streamed_q_ref.py restates it.
//
// Mapping, as in bp_streamed.hip: ONE LANE IS ONE FRAME.  A wavefront — a workgroup of 64 threads — owns a tile of T = 64 frames
// and a slab of device memory:
//     P[v][T] int16 posteriors | R[e][T] int8 messages, edges in processing order
// so a wavefront's access to one variable or one edge is 128 or 64 consecutive bytes, and no lane reads another lane's data.
// (Lanes that move two or four neighbouring frames as one word — 256 contiguous bytes and more per wave instruction — were
// measured and were 1.5 x slower: DESIGN 3h.)
// The graph is a plain CSR of the checks in processing order — the sets of bp_layered_block_build, set by set, which is an
// order equivalent to the LDS engine's since the checks of a set share no variable — read through wave-uniform scalar loads.
// The degree of a check is a loop bound.  Tiles are dealt by the launch's work counter; a slab belongs to a resident workgroup.
//
// A check of up to Q_SMALL variables is worked off in one pass with its cells in registers (each cell read once, written
// once: 6 bytes per edge and frame).  A wider one takes two passes in chunks of Q_SMALL edges: pass 1 forms the two minima, the
// XOR of the signs and the parity and writes nothing; pass 2 reads P and R again and writes R' and P' (9 bytes per edge).  The
// loads of a chunk are issued together.  Both forms are the four functions of quant_arith.hpp.
//
// Control: layered_ref._run_layered.  A frame latches after the first iteration in which every check was quiet; from then on
// its lane computes on but writes nothing, so its P stays the latched posterior.  Frames out of iterations get one
// syndrome pass.  early_exit = 1 ends the tile when every frame of it has latched; early_exit = 0 runs max_iter rounds; the
// outputs are the same.
//
// No stale state: a tile writes every P cell of its slab at its start (tail frames: 0), and in its first iteration takes every
// message as 0 WITHOUT reading R and writes it, so every R cell a live frame reads later was written by that frame in this
// tile.  (A frame that is not live — the tail of the last tile — reads whatever the slab holds; nothing of it is written or
// leaves.)
#include <hip/hip_runtime.h>

#include "launchers.hpp"
#include "quant_arith.hpp"

namespace acg {

typedef const int32_t __attribute__((address_space(4))) *sqconst_i32;
__device__ __forceinline__ int sq_sload(const int32_t *p, size_t i) { return ((sqconst_i32) (p))[i]; }

constexpr int Q_SMALL = 8;
constexpr int SQ_T = 64;   // frames of a tile: one per lane

struct SqTile {
    short *P;            // this lane's posterior of variable v: P[(size_t) v * SQ_T]
    signed char *R;      // this lane's message of edge e: R[(size_t) e * SQ_T]
    const int32_t *ev;
    bool first;      // the tile's first iteration: every message is 0 and R is not read
    bool live;       // the frame is updated: it exists and has not latched
    uint32_t loud;

    // N edges from e: the variables, and this lane's cells
    template <int N>
    __device__ __forceinline__ void load(const size_t e, int (&v)[N], int (&p)[N], int (&r)[N]) const {
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = sq_sload(ev, e + j);
#pragma unroll
        for (int j = 0; j < N; ++j) p[j] = P[(size_t) v[j] * SQ_T];
#pragma unroll
        for (int j = 0; j < N; ++j) r[j] = first ? 0 : (int) R[(e + j) * SQ_T];
    }
    template <int N>
    __device__ __forceinline__ void reduce(QCheck &ck, const int (&p)[N], const int (&r)[N], const QuantArgs &qa) const {
#pragma unroll
        for (int j = 0; j < N; ++j) q_reduce(ck, p[j], p[j] - r[j], qa);
    }
    // new cells of N edges from e; a frame that is not live writes nothing
    template <int N>
    __device__ __forceinline__ void update(const QCheck &ck, const size_t e, const int (&v)[N], const int (&p)[N], const int (&r)[N],
                                           const QuantArgs &qa) {
        int rn[N], pn[N];
        uint32_t flipped = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            q_update(ck, p[j] - r[j], qa, rn[j], pn[j]);
            flipped |= ((uint32_t) pn[j] >> 31) ^ ((uint32_t) p[j] >> 31);
        }
        loud |= (ck.parity | flipped) & 1u;
        if (live) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                P[(size_t) v[j] * SQ_T] = (short) pn[j];
                R[(e + j) * SQ_T] = (signed char) rn[j];
            }
        }
    }

    template <int N>
    __device__ __forceinline__ void small_check(const size_t e, const QuantArgs &qa) {
        int v[N], p[N], r[N];
        load<N>(e, v, p, r);
        QCheck ck;
        q_open(ck, qa);
        reduce<N>(ck, p, r, qa);
        q_close(ck, qa);
        update<N>(ck, e, v, p, r, qa);
    }
    template <int N>
    __device__ __forceinline__ void pass1(QCheck &ck, const size_t e, const QuantArgs &qa) const {
        int v[N], p[N], r[N];
        load<N>(e, v, p, r);
        reduce<N>(ck, p, r, qa);
    }
    template <int N>
    __device__ __forceinline__ void pass2(const QCheck &ck, const size_t e, const QuantArgs &qa) {
        int v[N], p[N], r[N];
        load<N>(e, v, p, r);
        update<N>(ck, e, v, p, r, qa);
    }

    // the check of the edges [e0, e1), e1 > e0 (wave-uniform)
    __device__ __forceinline__ void check(const size_t e0, const size_t e1, const QuantArgs &qa) {
        const int D = (int) (e1 - e0);
        if (D <= Q_SMALL) {
            switch (D) {
                case 1: small_check<1>(e0, qa); break;
                case 2: small_check<2>(e0, qa); break;
                case 3: small_check<3>(e0, qa); break;
                case 4: small_check<4>(e0, qa); break;
                case 5: small_check<5>(e0, qa); break;
                case 6: small_check<6>(e0, qa); break;
                case 7: small_check<7>(e0, qa); break;
                case 8: small_check<8>(e0, qa); break;
                default: break;
            }
            return;
        }
        QCheck ck;
        q_open(ck, qa);
        size_t e = e0;
        for (; e + Q_SMALL <= e1; e += Q_SMALL) pass1<Q_SMALL>(ck, e, qa);
        switch ((int) (e1 - e)) {
            case 1: pass1<1>(ck, e, qa); break;
            case 2: pass1<2>(ck, e, qa); break;
            case 3: pass1<3>(ck, e, qa); break;
            case 4: pass1<4>(ck, e, qa); break;
            case 5: pass1<5>(ck, e, qa); break;
            case 6: pass1<6>(ck, e, qa); break;
            case 7: pass1<7>(ck, e, qa); break;
            default: break;
        }
        q_close(ck, qa);
        for (e = e0; e + Q_SMALL <= e1; e += Q_SMALL) pass2<Q_SMALL>(ck, e, qa);
        switch ((int) (e1 - e)) {
            case 1: pass2<1>(ck, e, qa); break;
            case 2: pass2<2>(ck, e, qa); break;
            case 3: pass2<3>(ck, e, qa); break;
            case 4: pass2<4>(ck, e, qa); break;
            case 5: pass2<5>(ck, e, qa); break;
            case 6: pass2<6>(ck, e, qa); break;
            case 7: pass2<7>(ck, e, qa); break;
            default: break;
        }
    }
};

// grid <= the slabs behind ws.  qa.c_in: frames * n channel values; qa.post_out: frames * n posteriors or null.
__global__ void __launch_bounds__(64) bp_streamed_q_kernel(const StreamQTables t, const DecodeArgs a, const QuantArgs qa, unsigned char *__restrict__ ws) {
    constexpr int T = SQ_T;
    constexpr int XS = T + 2;   // shorts per row of the transposing buffer: rows an odd number of words apart
    __shared__ short X[64 * XS];   // 64 variables x T frames
    const int l = threadIdx.x;
    unsigned char *const slab = ws + (size_t) blockIdx.x * (size_t) t.slab_bytes;
    SqTile tl;
    tl.P = reinterpret_cast<short *>(slab) + l;
    tl.R = reinterpret_cast<signed char *>(slab + (size_t) t.n * T * 2) + l;
    tl.ev = t.edge_var;
    const int n = t.n;

    for (;;) {
        unsigned long long tv = 0;
        if (l == 0) tv = atomicAdd(a.work_counter, 1ull);
        const int64_t tile = (int64_t) (((unsigned long long) (uint32_t) __builtin_amdgcn_readfirstlane((int) (tv >> 32)) << 32) |
                                        (uint32_t) __builtin_amdgcn_readfirstlane((int) tv));
        const int64_t frame0 = tile * T;
        if (frame0 >= a.frames) break;
        const int nf = (int) (a.frames - frame0 < T ? a.frames - frame0 : T);   // frames of this tile (wave-uniform)
        const bool exists = l < nf;
        const size_t frame = (size_t) frame0 + l;

        // ---- start of the tile: P = clamped channel values, [frame][n] -> [n][T] through LDS, 64 variables at a time ---------
        for (int v0 = 0; v0 < n; v0 += 64) {
            const bool mine = v0 + l < n;
            const int16_t *const c = qa.c_in + (size_t) frame0 * n + v0 + l;
#pragma unroll 8
            for (int fr = 0; fr < T; ++fr) {
                int x = 0;
                if (fr < nf && mine) x = min(max((int) c[(size_t) fr * n], -qa.cmax), qa.cmax);
                X[l * XS + fr] = (short) x;
            }
            __syncthreads();
            const int nv = n - v0 < 64 ? n - v0 : 64;
            for (int vv = 0; vv < nv; ++vv) tl.P[(size_t) (v0 + vv) * T] = X[vv * XS + l];
            __syncthreads();
        }

        bool latched = false;
        int iters = a.max_iter;
        tl.live = exists;
        // ---- the iterations ------------------------------------------------------------------------------------------------------
        for (int it = 1; it <= a.max_iter; ++it) {
            if (a.early_exit && __ballot(tl.live) == 0ull) break;
            tl.loud = 0;
            tl.first = it == 1;
            size_t e0 = (size_t) sq_sload(t.row_ptr, 0);
            for (int i = 0; i < t.m; ++i) {
                const size_t e1 = (size_t) sq_sload(t.row_ptr, (size_t) i + 1);
                tl.check(e0, e1, qa);
                e0 = e1;
            }
            if (tl.live && tl.loud == 0u) {
                latched = true;
                iters = it;
                tl.live = false;
            }
        }
        // ---- frames out of iterations: one syndrome pass over the posteriors' signs ---------------------------------------------
        bool good = latched;
        if (a.max_iter > 0 && __ballot(tl.live) != 0ull) {
            int bad = 0;
            size_t e0 = (size_t) sq_sload(t.row_ptr, 0);
            for (int i = 0; i < t.m; ++i) {
                const size_t e1 = (size_t) sq_sload(t.row_ptr, (size_t) i + 1);
                int S = 0;
#pragma unroll 4
                for (size_t e = e0; e < e1; ++e) S ^= (int) tl.P[(size_t) sq_sload(t.edge_var, e) * T];
                bad |= S;
                e0 = e1;
            }
            if (tl.live) good = bad >= 0;
        }
        // ---- the tile's outputs: packed words (zeros for a failed frame), flags, iterations -------------------------------------
        if (exists) {
            if (a.out_ok) a.out_ok[frame] = good ? 1 : 0;
            if (a.out_iters) a.out_iters[frame] = iters;
        }
        if (a.out_bits) {
            for (int w = 0; w < t.nwords; ++w) {
                uint32_t word = 0;
                const int nb = n - 32 * w < 32 ? n - 32 * w : 32;
#pragma unroll 8
                for (int b = 0; b < nb; ++b) word |= ((uint32_t) (int) tl.P[(size_t) (32 * w + b) * T] >> 31) << b;
                if (exists) a.out_bits[frame * t.nwords + w] = good ? word : 0u;
            }
        }
        // ---- and its posteriors, [n][T] -> [frame][n] through LDS -------------------------------------------------------------------
        if (qa.post_out) {
            for (int v0 = 0; v0 < n; v0 += 64) {
                const int nv = n - v0 < 64 ? n - v0 : 64;
                for (int vv = 0; vv < nv; ++vv) X[vv * XS + l] = tl.P[(size_t) (v0 + vv) * T];
                __syncthreads();
                if (v0 + l < n) {
                    int16_t *const po = qa.post_out + (size_t) frame0 * n + v0 + l;
                    for (int fr = 0; fr < nf; ++fr) po[(size_t) fr * n] = X[l * XS + fr];
                }
                __syncthreads();
            }
        }
    }
}

const void *bp_streamed_q_kernel_ptr() { return (const void *) bp_streamed_q_kernel; }

hipError_t bp_streamed_q_launch(const void *kernel, const StreamQTables &t, const DecodeArgs &a, const QuantArgs &q, unsigned char *ws,
                                int grid, hipStream_t s) {
    void *args[] = {(void *) &t, (void *) &a, (void *) &q, (void *) &ws};
    return hipLaunchKernel(kernel, dim3((unsigned) grid), dim3(64), args, 0, s);
}

}  // namespace acg
