// Fixed-point layered min-sum, one workgroup per frame — the schedule, sets, steps and control flow of bp_layered_block.hip /
// bp_layered_wide.hip (conflict-free same-degree sets of checks of degree 1 ... 32, posteriors updated in place after every set,
// the quiet-round stopping rule, latching, the final syndrome pass) with every value an integer: channel values of ch_bits,
// check-to-variable messages of msg_bits <= 8, posteriors of post_bits <= 16, normalisation scale_num / 2^scale_shift rounded
// half up and an offset (acg_ldpc_quant, include/acg_ldpc.h).  No transcendental, no fma question: tests/layered_q_ref.py
// restates it and word, flag and exit iteration of every frame are equal.  Reached through acg_ldpc_decoder_create_quantized
// only.
//
// LDS of the workgroup: P int16[n] + the neutral cell (0; padded to 16 bytes) | R: one byte per edge (padded to 4) | the packed
// output word.  Nothing else: (3,6) 5000 x 10 000 is 20 016 + 30 000 + 1 252 = 51 268 bytes, three workgroups per CU by LDS.
//
// Message cells: a PLANE per edge index inside every set — the byte of edge j of the check in slot s of a set of cnt checks
// that starts at cell `off` is R[off + j * cnt + s].  That is the index of the same edge's entry in the position table
// (LayerBlockTables::pos), so a step needs one offset for both.  A wavefront's access to edge j covers 64 consecutive bytes =
// 16 consecutive dwords: 16 banks, four lanes per dword.  Modelled: reads of one dword by four lanes broadcast (one LDS cycle per
// 32-lane group); byte stores of four lanes into one dword are four addresses on one bank, 4-way, which the store's own
// register transfer (4 cycles for a one-dword store) covers up to 2-way: about 2 x on the message stores.  Rows per check
// (R[check][edge], the float kernels' layout) would put the lanes deg bytes apart: for deg = 32 every lane of a 32-lane group
// on banks 0, 8, 16, 24 — 8-way on reads and writes.  Posterior cells are reached through the position table as in the float
// kernels: two lanes may share a dword (different halves, different variables), which is a broadcast for reads and a 2-way
// store.
//
// A check of degree 9 ... 32 is worked off in two passes over its edges in chunks of 8 (bp_layered_wide.hip: the degree is a
// run-time value, uniform over the workgroup, so the chunks sit behind scalar branches and every register array is indexed by
// constants): pass 1 forms m1, m2, the XOR of the signs and the parity of the hard decisions and writes nothing; pass 2 reads P
// and R again, writes R' and P'.  The checks of a set share no variable, so nobody else touches those cells in between.  A check
// of degree <= 8 keeps the p and q of its one chunk in registers instead of reading them twice.  ONE definition of the
// arithmetic (q_open / q_reduce / q_close / q_edge) under both forms.  The 8 position entries of the chunk that follows — of the
// same pass, of pass 2, or chunk 0 of the next step — are fetched before the arithmetic of the current chunk.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "launchers.hpp"
#include "quant_arith.hpp"

namespace acg {

typedef const int32_t __attribute__((address_space(4))) *qconst_i32;
__device__ __forceinline__ int qsload(const int32_t *p, int i) { return ((qconst_i32) (p))[i]; }

constexpr int Q_CHUNK = 8;
constexpr int Q_MAXD = 32;
constexpr int Q_CHUNKS = Q_MAXD / Q_CHUNK;

// The quantiser: symbol i of a.y -> channel value.  llr is the fp32 channel LLR of the float layered kernels
// (bp_layered_block.hip), t ONE fp32 multiply, rounding half to even (v_rndne_f32), NaN -> 0, +-inf -> +-cmax by the clamp.
__device__ __forceinline__ int quantize_symbol(const DecodeArgs &a, const QuantArgs &qa, const size_t i) {
    float llr;
    if (a.y_is_f64) llr = (float) (2 * reinterpret_cast<const double *>(a.y)[i] / a.var);
    else llr = (float) ((double) reinterpret_cast<const float *>(a.y)[i] * a.inv_var2);
    const float t = llr * qa.inv_step;
    if (__builtin_isnan(t)) return 0;
    const float cm = (float) qa.cmax;
    return (int) __builtin_fminf(__builtin_fmaxf(__builtin_rintf(t), -cm), cm);
}

// The arithmetic of a check (quant_arith.hpp: QCheck, q_open / q_reduce / q_close / q_update) is ONE definition for both forms
// of q_layer_step, and for the streamed engine (bp_streamed_q.hip).
// the edge with posterior p and q = p - r: new message and posterior into their cells -> bit 0: its hard decision flipped
__device__ __forceinline__ uint32_t q_edge(const QCheck &c, const int p, const int q, const QuantArgs &qa, short *const pc, signed char *const rc) {
    int rn, pn;
    q_update(c, q, qa, rn, pn);
    *pc = (short) pn;
    *rc = (signed char) rn;
    return ((uint32_t) pn >> 31) ^ ((uint32_t) p >> 31);
}

// One step of a frame for this thread's check of degree D = 1 ... 32.  Rl: the byte of (edge 0, this thread); `stride`: bytes
// between consecutive edges (the checks of the whole set).  posn: the positions of chunk 0 on entry, those of chunk 0 of the
// next step kn on return; fetch(k, c, posn) is the kernel's position fetch.  `active`: this thread has a check in the step
// (the others only keep the position pipeline going).  -> 1 <=> the step was not quiet for this thread
// Two forms around the same four functions: D <= 8 keeps p and q of the one chunk in registers between the reductions and the
// stores (each cell and each position entry is read once); D = 9 ... 32 makes two passes over the cells in chunks of 8.
template <typename Fetch>
__device__ __forceinline__ uint32_t q_layer_step(unsigned char *__restrict__ Pb, signed char *__restrict__ Rl, const int stride, const int D,
                                                 const bool active, int (&posn)[Q_CHUNK], const Fetch fetch, const int k, const int kn,
                                                 const QuantArgs &qa) {
    QCheck ck;
    q_open(ck, qa);
    uint32_t flipped = 0;
    if (D <= Q_CHUNK) {   // (workgroup-uniform)
        int pos[Q_CHUNK];
#pragma unroll
        for (int j = 0; j < Q_CHUNK; ++j) pos[j] = posn[j];
        fetch(kn, 0, posn);
        if (active) {
            int p[Q_CHUNK], q[Q_CHUNK];
#pragma unroll
            for (int j = 0; j < Q_CHUNK; ++j) {
                if (j < D) {
                    p[j] = *reinterpret_cast<const short *>(Pb + pos[j]);
                    q[j] = p[j] - (int) Rl[(size_t) j * stride];
                    q_reduce(ck, p[j], q[j], qa);
                }
            }
            q_close(ck, qa);
#pragma unroll
            for (int j = 0; j < Q_CHUNK; ++j)
                if (j < D) flipped |= q_edge(ck, p[j], q[j], qa, reinterpret_cast<short *>(Pb + pos[j]), Rl + (size_t) j * stride);
        }
        return (ck.parity | flipped) & 1u;
    }
    const int nc = (D + Q_CHUNK - 1) / Q_CHUNK;
    // ---- pass 1: the reductions over the whole check; nothing is written ----------------------------------------------------
#pragma unroll
    for (int c = 0; c < Q_CHUNKS; ++c) {
        if (c < nc) {
            int pos[Q_CHUNK];
#pragma unroll
            for (int j = 0; j < Q_CHUNK; ++j) pos[j] = posn[j];
            if (c + 1 < nc) fetch(k, c + 1, posn);   // (the last chunk of pass 1 is the first of pass 2: its positions stay)
            if (active) {
#pragma unroll
                for (int j = 0; j < Q_CHUNK; ++j) {
                    if (c * Q_CHUNK + j < D) {
                        const int p = *reinterpret_cast<const short *>(Pb + pos[j]);
                        q_reduce(ck, p, p - (int) Rl[(size_t) (c * Q_CHUNK + j) * stride], qa);
                    }
                }
            }
        }
    }
    q_close(ck, qa);
    // ---- pass 2: new messages and posteriors, chunk by chunk from the last ---------------------------------------------------
#pragma unroll
    for (int c = Q_CHUNKS - 1; c >= 0; --c) {
        if (c < nc) {
            int pos[Q_CHUNK];
#pragma unroll
            for (int j = 0; j < Q_CHUNK; ++j) pos[j] = posn[j];
            if (c > 0) fetch(k, c - 1, posn);
            else fetch(kn, 0, posn);
            if (active) {
#pragma unroll
                for (int j = 0; j < Q_CHUNK; ++j) {
                    if (c * Q_CHUNK + j < D) {
                        short *const pc = reinterpret_cast<short *>(Pb + pos[j]);
                        signed char *const rc = Rl + (size_t) (c * Q_CHUNK + j) * stride;
                        const int p = *pc;
                        flipped |= q_edge(ck, p, p - (int) *rc, qa, pc, rc);
                    }
                }
            }
        }
    }
    return (ck.parity | flipped) & 1u;
}

// Two workgroups of 1024 threads per CU are 8 wavefronts per SIMD: at most 96 scalar and 64 vector registers.  Without the bound
// the compiler takes 106 scalar registers — 7 wavefronts per SIMD, ONE workgroup of 1024 per CU.  The smaller workgroups reach their
// residency (three of 512 per CU: 6 wavefronts per SIMD) without it and keep the registers.
//
// IO: the integer entrance (acg_ldpc_decode_batch_q*).  A frame starts from qa.c_in — int16 channel values, clamped to +-cmax, no
// quantiser — and, where qa.post_out is set, its int16 posteriors leave with its word.  The symbol entrance's instances (IO =
// false) read neither pointer and compile to what they compiled to without them.  Left to itself the compiler gives the IO
// instances 77-80 vector registers where their siblings take 68-71: 6 wavefronts per SIMD instead of 7.  For L <= 256 that is a
// workgroup per SIMD fewer (24 / (L / 64) per CU instead of 28 / (L / 64)), so those are bound to 7 (72 registers, 4-5 of them in
// scratch, reloaded once per FRAME: no scratch access inside a round); for L = 512 both figures are three workgroups per CU
// and the instance keeps its registers.
//
// Grid: the third form (acg_ldpc_mc_run_quants) — frames of DIFFERENT quantisers in one launch.  Grid is empty for the two
// forms above, whose argument list is the three blocks, or the one type QuantGridArgs: a fourth argument block that only this
// form has.  The work counter deals virtual frames vf in [0, points * g.fc): point vf / g.fc decodes frame vf % g.fc of the
// shared symbol buffer a.y with the eight quantiser words at g.tab + 8 * point, and word, flag and iteration go to index vf.
// The point index is formed from the first lane's copy of vf (a launch covers fewer than 2^30 virtual frames), so the table is
// read by scalar loads and the frame's quantiser lies in scalar registers as the kernel argument of the other forms does:
// everything below sees a QuantArgs and is the same code.  One division per frame.  Under the symbol entrance's bounds it has
// that one's residency: 67-70 vector registers (7 wavefronts per SIMD) for L <= 512, 64 and 8 for L = 1024.  (Bound to 7 as the
// IO instances are, L <= 256 drops from 106 to 94 scalar registers and spills 50-52 of them instead of 38-40: 1 % slower.)
template <int L, bool IO, typename... Grid>
__global__ void __launch_bounds__(L) __attribute__((amdgpu_waves_per_eu(L >= 1024 ? 8 : (IO && L <= 256 ? 7 : 6)))) bp_layered_q_kernel(const LayerBlockTables t, const DecodeArgs a, const QuantArgs qa_arg, const Grid... grid) {
    constexpr bool GRID = sizeof...(Grid) != 0;
    static_assert(!GRID || (sizeof...(Grid) == 1 && !IO), "the grid form: one QuantGridArgs behind the symbol entrance's arguments");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned long long fr_lds;
    const int l = threadIdx.x;
    unsigned char *Pb = smem;
    short *P = reinterpret_cast<short *>(smem);                            // P[n] + neutral cell (+ padding): 4 * p_words bytes
    signed char *R = reinterpret_cast<signed char *>(smem) + 4 * (size_t) t.p_words;   // one byte per edge: 4 * r_words bytes
    uint32_t *OB = reinterpret_cast<uint32_t *>(smem) + t.p_words + t.r_words;
    const int NS = t.n_steps;
    const int neutral = 2 * t.n;

    // positions of chunk c (edges 8 c ... 8 c + 7) of step k for this thread (the neutral cell where it has no such edge)
    auto fetch = [tstep = t.step, tpos = t.pos, l, neutral](const int k, const int c, int (&pos)[Q_CHUNK]) {
        const int deg = qsload(tstep, 8 * k), toff = qsload(tstep, 8 * k + 3), cnt = qsload(tstep, 8 * k + 4), stride = qsload(tstep, 8 * k + 5);
        const int32_t *T = tpos + toff + (size_t) (c * Q_CHUNK) * stride;   // (scalar: the lane is the vector offset of every load)
#pragma unroll
        for (int j = 0; j < Q_CHUNK; ++j) pos[j] = (c * Q_CHUNK + j < deg && l < cnt) ? (T + (size_t) j * stride)[l] : neutral;
    };
    // explicit syndrome of the posteriors' signs (frames that ran out of iterations without a quiet round)
    auto syndrome_bad = [&]() -> bool {
        uint32_t acc = 0;
        for (int k = 0; k < NS; ++k) {
            const int deg = qsload(t.step, 8 * k), toff = qsload(t.step, 8 * k + 3), cnt = qsload(t.step, 8 * k + 4), stride = qsload(t.step, 8 * k + 5);
            if (l < cnt) {
                const int32_t *T = t.pos + toff + l;
                uint32_t S = 0;
                for (int j = 0; j < deg; ++j) S ^= (uint32_t) (int) *reinterpret_cast<const short *>(Pb + T[(size_t) j * stride]);
                acc |= S;
            }
        }
        return __syncthreads_or((acc >> 31) != 0u ? 1 : 0) != 0;
    };

    for (;;) {
        __syncthreads();
        if (l == 0) fr_lds = atomicAdd(a.work_counter, 1ull);
        __syncthreads();
        const int64_t frame = (int64_t) fr_lds;
        if (frame >= a.frames) break;
        // ---- the frame's quantiser and its row of a.y: the argument and `frame`, or the point's table row and frame % fc -------------
        QuantArgs qg;
        size_t sym_frame = (size_t) frame;
        if constexpr (GRID) {
            const QuantGridArgs &g = (grid, ...);
            const uint32_t vf = (uint32_t) __builtin_amdgcn_readfirstlane((int) frame);
            const uint32_t point = vf / g.fc;
            const int32_t *const row = g.tab + (size_t) point * 8;
            qg.inv_step = __builtin_bit_cast(float, qsload(row, 0));
            qg.cmax = qsload(row, 1), qg.rmax = qsload(row, 2), qg.pmax = qsload(row, 3);
            qg.scale_num = qsload(row, 4), qg.scale_shift = qsload(row, 5), qg.rnd = qsload(row, 6), qg.offset = qsload(row, 7);
            qg.c_in = nullptr, qg.post_out = nullptr;
            sym_frame = (size_t) (vf - point * g.fc);
        }
        const QuantArgs &qa = [&]() -> const QuantArgs & {
            if constexpr (GRID) return qg;
            else return qa_arg;
        }();
        // ---- start of a frame: P = quantised channel LLR, R = 0 -------------------------------------------------------------------
        if constexpr (IO) {
            // (rows are n values apart: 2-byte aligned only, so one value per load)
            const int16_t *const c = qa.c_in + (size_t) frame * t.n;
            for (int v = l; v < t.n; v += L) P[v] = (short) min(max((int) c[v], -qa.cmax), qa.cmax);
        } else {
            for (int v = l; v < t.n; v += L) P[v] = (short) quantize_symbol(a, qa, sym_frame * t.n + v);
        }
        for (int w = t.n + l; w < 2 * t.p_words; w += L) P[w] = 0;   // neutral cell: decides 0
        {
            uint32_t *Rw = reinterpret_cast<uint32_t *>(R);
            for (int w = l; w < t.r_words; w += L) Rw[w] = 0u;
        }
        int posn[Q_CHUNK];
        fetch(0, 0, posn);
        int it = 0;             // iterations (rounds over all sets) this frame has been through
        bool latched = false;
        uint32_t noisy_acc = 0; // some step of the current round was not quiet for this thread's checks
        for (;;) {
            // ---- round boundary (and the barrier behind the frame's start / the last set) -----------------------------------
            const bool loud = __syncthreads_or(noisy_acc != 0u ? 1 : 0) != 0;
            noisy_acc = 0;
            const bool conv = it > 0 && !loud;
            const bool out_of_sweeps = it >= a.max_iter;
            bool conv2 = conv;
            if (out_of_sweeps && !conv && !latched) {   // (workgroup-uniform)
                const bool bad = syndrome_bad();
                if (!bad && a.max_iter > 0) conv2 = true;
            }
            const bool out_now = conv2 && !latched;
            const bool finish = (a.early_exit && conv2) || out_of_sweeps;
            const bool fail_now = finish && !conv2 && !latched;
            if (out_now || fail_now) {
                if (out_now) {
                    // the word, 64 hard decisions per wavefront and trip: the wavefronts' chunks are 64-aligned, so they fill
                    // whole output words and no two wavefronts write the same one
                    for (int v0 = l & ~63; v0 < t.n; v0 += L) {
                        const int v = v0 + (l & 63);
                        const unsigned long long b = __ballot(v < t.n && P[v < t.n ? v : t.n] < 0);
                        if ((l & 63) == 0) {
                            OB[v0 >> 5] = (uint32_t) b;
                            if ((v0 >> 5) + 1 < t.nwords) OB[(v0 >> 5) + 1] = (uint32_t) (b >> 32);
                        }
                    }
                } else {
                    for (int w = l; w < t.nwords; w += L) OB[w] = 0u;
                }
                if constexpr (IO) {
                    // the posteriors of this round boundary: nobody has written P since the barrier of the round's OR, and the
                    // barrier below stands between these reads and the next set
                    if (qa.post_out) {
                        int16_t *const po = qa.post_out + (size_t) frame * t.n;
#pragma nounroll
                        for (int v = l; v < t.n; v += L) po[v] = P[v];
                    }
                }
                __syncthreads();   // (also: every posterior of the word is read before the next set rewrites it)
                if (a.out_bits)
                    for (int w = l; w < t.nwords; w += L) a.out_bits[(size_t) frame * t.nwords + w] = OB[w];
                if (l == 0) {
                    if (a.out_ok) a.out_ok[frame] = out_now ? 1 : 0;
                    if (a.out_iters) a.out_iters[frame] = it < a.max_iter ? it : a.max_iter;
                }
                latched = true;
            }
            if (finish) break;
            // ---- one iteration: every set in turn, posteriors updated in place ----------------------------------------------
            for (int k = 0; k < NS; ++k) {
                const int deg = qsload(t.step, 8 * k), barrier = qsload(t.step, 8 * k + 1), toff = qsload(t.step, 8 * k + 3), cnt = qsload(t.step, 8 * k + 4),
                          stride = qsload(t.step, 8 * k + 5);
                const int kn = k + 1 < NS ? k + 1 : 0;
                noisy_acc |= q_layer_step(Pb, R + toff + l, stride, deg, l < cnt, posn, fetch, k, kn, qa);
                if (barrier) __syncthreads();
            }
            it += 1;
        }
    }
}

template <bool IO>
static const void *q_kernel_ptr_l(int L) {
    switch (L) {
        case 64: return (const void *) bp_layered_q_kernel<64, IO>;
        case 128: return (const void *) bp_layered_q_kernel<128, IO>;
        case 256: return (const void *) bp_layered_q_kernel<256, IO>;
        case 512: return (const void *) bp_layered_q_kernel<512, IO>;
        case 1024: return (const void *) bp_layered_q_kernel<1024, IO>;
        default: return nullptr;
    }
}

// io: the instance of the integer entrance (channel values in, posteriors out)
const void *bp_layered_q_kernel_ptr(int L, bool io) { return io ? q_kernel_ptr_l<true>(L) : q_kernel_ptr_l<false>(L); }

// the grid form (acg_ldpc_mc_run_quants): a quantiser per virtual frame from QuantGridArgs::tab
const void *bp_layered_q_grid_kernel_ptr(int L) {
    switch (L) {
        case 64: return (const void *) bp_layered_q_kernel<64, false, QuantGridArgs>;
        case 128: return (const void *) bp_layered_q_kernel<128, false, QuantGridArgs>;
        case 256: return (const void *) bp_layered_q_kernel<256, false, QuantGridArgs>;
        case 512: return (const void *) bp_layered_q_kernel<512, false, QuantGridArgs>;
        case 1024: return (const void *) bp_layered_q_kernel<1024, false, QuantGridArgs>;
        default: return nullptr;
    }
}

// acg_ldpc_debug_quantize: the device function the decode kernel calls, on a plain array of symbols
__global__ void __launch_bounds__(256) quantize_debug_kernel(const DecodeArgs a, const QuantArgs qa, const int64_t count, int16_t *__restrict__ out) {
    for (int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t) gridDim.x * 256) out[i] = (int16_t) quantize_symbol(a, qa, (size_t) i);
}

hipError_t quantize_debug_launch(const DecodeArgs &a, const QuantArgs &q, int64_t count, int16_t *out, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const int grid = (int) std::min<int64_t>((count + 255) / 256, 1024);
    hipLaunchKernelGGL(quantize_debug_kernel, dim3(grid), dim3(256), 0, s, a, q, count, out);
    return hipGetLastError();
}

}  // namespace acg
