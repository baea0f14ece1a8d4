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
// The tile loop — the claim of a tile, the iterations and the latch, the syndrome pass, the outputs — is streamed_tile_loop of
// bp_streamed_tile.inc, shared with bp_streamed_layered.hip; "Control" and "No stale state" are written there.
#include <hip/hip_runtime.h>

#include "launchers.hpp"
#include "quant_arith.hpp"

namespace acg {
#include "bp_core.inc"         // (what bp_layer_math.inc stands behind; none of its float arithmetic is used here)
#include "bp_layer_math.inc"   // lsload, LMAXD, ACG_LAYER_SWITCH
#include "bp_streamed_tile.inc"

constexpr int Q_SMALL = LMAXD;   // edges of a chunk: the cells of a check a lane holds in registers

struct SqTile {
    short *P;            // this lane's posterior of variable v: P[(size_t) v * TILE_T]
    signed char *R;      // this lane's message of edge e: R[(size_t) e * TILE_T]
    const int32_t *ev;
    short *X;            // the workgroup's transposing buffer: 64 variables x T frames, rows of XS shorts
    int n;
    QuantArgs qa;        // c_in: frames * n channel values; post_out: frames * n posteriors or null
    bool first;      // the tile's first iteration: every message is 0 and R is not read
    bool live;       // the frame is updated: it exists and has not latched
    uint32_t loud;   // bit 0: some check of the iteration was not quiet for this frame
    static constexpr int XS = TILE_T + 2;   // rows an odd number of words apart

    // N edges from e: the variables, and this lane's cells
    template <int N>
    __device__ __forceinline__ void load(const size_t e, int (&v)[N], int (&p)[N], int (&r)[N]) const {
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = lsload(ev, e + j);
#pragma unroll
        for (int j = 0; j < N; ++j) p[j] = P[(size_t) v[j] * TILE_T];
#pragma unroll
        for (int j = 0; j < N; ++j) r[j] = first ? 0 : (int) R[(e + j) * TILE_T];
    }
    template <int N>
    __device__ __forceinline__ void reduce(QCheck &ck, const int (&p)[N], const int (&r)[N]) const {
#pragma unroll
        for (int j = 0; j < N; ++j) q_reduce(ck, p[j], p[j] - r[j], qa);
    }
    // new cells of N edges from e; a frame that is not live writes nothing
    template <int N>
    __device__ __forceinline__ void update(const QCheck &ck, const size_t e, const int (&v)[N], const int (&p)[N], const int (&r)[N]) {
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
                P[(size_t) v[j] * TILE_T] = (short) pn[j];
                R[(e + j) * TILE_T] = (signed char) rn[j];
            }
        }
    }

    template <int N>
    __device__ __forceinline__ void small_check(const size_t e) {
        int v[N], p[N], r[N];
        load<N>(e, v, p, r);
        QCheck ck;
        q_open(ck, qa);
        reduce<N>(ck, p, r);
        q_close(ck, qa);
        update<N>(ck, e, v, p, r);
    }
    template <int N>
    __device__ __forceinline__ void pass1(QCheck &ck, const size_t e) const {
        int v[N], p[N], r[N];
        load<N>(e, v, p, r);
        reduce<N>(ck, p, r);
    }
    template <int N>
    __device__ __forceinline__ void pass2(const QCheck &ck, const size_t e) {
        int v[N], p[N], r[N];
        load<N>(e, v, p, r);
        update<N>(ck, e, v, p, r);
    }

    // the check of the edges [e0, e1), e1 > e0 (wave-uniform)
    __device__ __forceinline__ void check(const size_t e0, const size_t e1) {
        const int D = (int) (e1 - e0);
        if (D <= Q_SMALL) {
#define ACG_CALL(N) small_check<N>(e0)
            ACG_LAYER_SWITCH(D, ACG_CALL)
#undef ACG_CALL
            return;
        }
        QCheck ck;
        q_open(ck, qa);
        size_t e = e0;
        for (; e + Q_SMALL <= e1; e += Q_SMALL) pass1<Q_SMALL>(ck, e);
#define ACG_CALL(N) pass1<N>(ck, e)
        ACG_TILE_TAIL((int) (e1 - e), ACG_CALL)
#undef ACG_CALL
        q_close(ck, qa);
        for (e = e0; e + Q_SMALL <= e1; e += Q_SMALL) pass2<Q_SMALL>(ck, e);
#define ACG_CALL(N) pass2<N>(ck, e)
        ACG_TILE_TAIL((int) (e1 - e), ACG_CALL)
#undef ACG_CALL
    }

    __device__ __forceinline__ uint32_t sign(const int v) const { return (uint32_t) (int) P[(size_t) v * TILE_T]; }

    // start of the tile: P = clamped channel values, [frame][n] -> [n][T] through LDS, 64 variables at a time
    __device__ __forceinline__ void fill(const int64_t frame0, const int nf) {
        constexpr int T = TILE_T;
        const int l = threadIdx.x;
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
            for (int vv = 0; vv < nv; ++vv) P[(size_t) (v0 + vv) * T] = X[vv * XS + l];
            __syncthreads();
        }
    }
    // end of the tile: its posteriors, [n][T] -> [frame][n] through LDS
    __device__ __forceinline__ void drain(const int64_t frame0, const int nf) {
        constexpr int T = TILE_T;
        const int l = threadIdx.x;
        if (qa.post_out) {
            for (int v0 = 0; v0 < n; v0 += 64) {
                const int nv = n - v0 < 64 ? n - v0 : 64;
                for (int vv = 0; vv < nv; ++vv) X[vv * XS + l] = P[(size_t) (v0 + vv) * T];
                __syncthreads();
                if (v0 + l < n) {
                    int16_t *const po = qa.post_out + (size_t) frame0 * n + v0 + l;
                    for (int fr = 0; fr < nf; ++fr) po[(size_t) fr * n] = X[l * XS + fr];
                }
                __syncthreads();
            }
        }
    }
};

// grid <= the slabs behind ws.  qa.c_in: frames * n channel values; qa.post_out: frames * n posteriors or null.
__global__ void __launch_bounds__(64) bp_streamed_q_kernel(const StreamLayTables t, const DecodeArgs a, const QuantArgs qa, unsigned char *__restrict__ ws) {
    constexpr int T = TILE_T;
    __shared__ short X[64 * SqTile::XS];
    const int l = threadIdx.x;
    unsigned char *const slab = ws + (size_t) blockIdx.x * (size_t) t.slab_bytes;
    SqTile tl;
    tl.P = reinterpret_cast<short *>(slab) + l;
    tl.R = reinterpret_cast<signed char *>(slab + (size_t) t.n * T * 2) + l;
    tl.ev = t.edge_var;
    tl.X = X;
    tl.n = t.n;
    tl.qa = qa;
    streamed_tile_loop(t, a, tl);
}

const void *bp_streamed_q_kernel_ptr() { return (const void *) bp_streamed_q_kernel; }

}  // namespace acg
