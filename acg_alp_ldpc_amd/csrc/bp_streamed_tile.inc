// The tile loop of the streamed layered engines, shared by the fixed-point kernel (bp_streamed_q.hip) and the float kernels
// (bp_streamed_layered.hip): both include this file inside namespace acg, behind bp_layer_math.inc (lsload, LMAXD,
// ACG_LAYER_SWITCH).  Device only.  One definition, so the latch rule of the engines cannot drift apart.
//
// ONE LANE IS ONE FRAME: a wavefront — a workgroup of 64 threads — owns a tile of TILE_T = 64 frames and a slab of device memory
// that holds P[v][T] and R[e][T] in the engine's cell type.  What an engine brings is its Tile:
//     first, live, loud       the three flags below, which check() reads and this loop sets
//     fill(frame0, nf)        start of a tile: every P cell of the slab from the channel values (tail frames: 0)
//     check(e0, e1)           the check of the edges [e0, e1), e1 > e0 (wave-uniform); ORs bit 0 of loud if it was not quiet
//     sign(v)                 a word whose bit 31 is the sign of this lane's posterior of variable v
//     drain(frame0, nf)       end of a tile: what the engine hands out beyond the hard decisions
//
// Control: layered_ref._run_layered.  A frame latches after the first iteration in which every check was quiet; from then on
// its lane computes on but writes nothing of P or R, so its P stays the latched posterior.  Frames out of iterations get one
// syndrome pass.  early_exit = 1 ends the tile when every frame of it has latched; early_exit = 0 runs max_iter rounds; the
// outputs are the same.
//
// No stale state: a tile writes every P cell of its slab at its start (tail frames: 0), and in its first iteration takes every
// message as 0 WITHOUT reading R and writes it, so every R cell a live frame reads later was written by that frame in this
// tile.  (A frame that is not live — the tail of the last tile — reads whatever the slab holds; nothing of it is written or
// leaves.)

constexpr int TILE_T = 64;   // frames of a tile: one per lane

// the last, shorter chunk of a wide check: 1 ... LMAXD - 1 edges
#define ACG_TILE_TAIL(n, CALL)  \
    switch (n) {                \
        case 1: CALL(1); break; \
        case 2: CALL(2); break; \
        case 3: CALL(3); break; \
        case 4: CALL(4); break; \
        case 5: CALL(5); break; \
        case 6: CALL(6); break; \
        case 7: CALL(7); break; \
        default: break;         \
    }
static_assert(LMAXD == 8, "ACG_TILE_TAIL covers the remainders of a chunk of 8 edges");

// the for (;;) of a kernel: tiles are dealt by the launch's work counter until none is left
template <class Tile>
__device__ __forceinline__ void streamed_tile_loop(const StreamLayTables &t, const DecodeArgs &a, Tile &tl) {
    constexpr int T = TILE_T;
    const int l = threadIdx.x;
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

        tl.fill(frame0, nf);

        bool latched = false;
        int iters = a.max_iter;
        // live is held here and copied into the tile for check(): read back from the member, which the compiler keeps as a byte,
        // the latch cost bp_streamed_q_kernel a VGPR (79 for 78) and 0.5 % on the (3,6) 5000 x 10000
        bool live = exists;
        tl.live = live;
        // ---- the iterations ------------------------------------------------------------------------------------------------------
        for (int it = 1; it <= a.max_iter; ++it) {
            if (a.early_exit && __ballot(live) == 0ull) break;
            tl.loud = 0;
            tl.first = it == 1;
            size_t e0 = (size_t) lsload(t.row_ptr, 0);
            for (int i = 0; i < t.m; ++i) {
                const size_t e1 = (size_t) lsload(t.row_ptr, (size_t) i + 1);
                tl.check(e0, e1);
                e0 = e1;
            }
            // quiet: check() of either engine only ever sets bit 0 of loud, so the word is 0 exactly when that bit is
            if (live && tl.loud == 0u) {
                latched = true;
                iters = it;
                live = false;
            }
            tl.live = live;
        }
        // ---- frames out of iterations: one syndrome pass over the posteriors' signs ---------------------------------------------
        bool good = latched;
        if (a.max_iter > 0 && __ballot(live) != 0ull) {
            uint32_t bad = 0;
            size_t e0 = (size_t) lsload(t.row_ptr, 0);
            for (int i = 0; i < t.m; ++i) {
                const size_t e1 = (size_t) lsload(t.row_ptr, (size_t) i + 1);
                uint32_t S = 0;
#pragma unroll 4
                for (size_t e = e0; e < e1; ++e) S ^= tl.sign(lsload(t.edge_var, e));
                bad |= S;
                e0 = e1;
            }
            if (live) good = (bad >> 31) == 0u;
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
                for (int b = 0; b < nb; ++b) word |= (tl.sign(32 * w + b) >> 31) << b;
                if (exists) a.out_bits[frame * t.nwords + w] = good ? word : 0u;
            }
        }
        tl.drain(frame0, nf);
    }
}
