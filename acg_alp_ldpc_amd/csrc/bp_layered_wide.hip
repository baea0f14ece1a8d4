// Workgroup-per-frame layered BP for WIDE checks — bp_layered_block.hip with check degree 1 ... 32 instead of 1 ... 8: the
// layered engine for high-rate codes (802.11n rate 5/6: degree 20-22, the 10GBASE-T (6,32)-regular code, 5G NR base graph 1).
// Everything but the per-check step is that kernel: one workgroup of L = 256, 512 or 1024 threads owns a frame, LDS holds P[n]
// (fp32) + the neutral cell | one message cell per edge, the checks in set / slot order | the packed output word; the steps are
// the (set, pass) pairs of LayerBlockTables; one barrier separates sets; the quiet-round rule, latching, the final syndrome
// pass and max_iter = 0 are the same lines.  tests/layered_ref.py (_run_layered) restates it as it restates that kernel.
//
// The step of a check of degree D <= 8 is block_layer_step of bp_layered_block.hip (layer_front / layer_back / layer_back_spa
// of bp_layer_math.inc, fully unrolled).  A check of degree 9 ... 32 cannot be unrolled like that: at L = 1024 a wavefront has
// 128 VGPRs, and pos, p, q, r, mag and pre of 32 edges are 192.  It is worked off in CHUNKS of 8 edges (D is a run-time value,
// uniform over the workgroup: nc = ceil(D / 8) = 2, 3 or 4 chunks behind scalar branches, every register array indexed by
// constants) in two passes over the thread's own cells — the checks of a set share no variable, so between the passes nobody
// else touches them:
//   pass 1, chunks ascending: p_j through the positions, r_j from the message cells, q_j = p_j - r_j; the reductions over the
//           whole check — min-sum: m1, m2, the XOR of the signs; sum-product: mag_j = phi(|q_j|), kept for all 32 edges, and
//           the running prefix sum at the start of every chunk.  Nothing is written.
//   pass 2, chunks descending: p_j and r_j read AGAIN (the same bits: nothing of the check has been written before all of it
//           was read, and what pass 2 writes belongs to chunks it has finished), q_j recomputed, the new message, p'_j = q_j +
//           r'_j, stores.  Sum-product: pre_j restarts from the chunk's saved prefix and adds the same mag in the same order
//           as pass 1 did, so it has the bits of ONE ascending sum over all D edges; suf runs on from chunk to chunk in
//           descending edge order.  Two phi per edge, as for D <= 8.
// An edge beyond D in the last chunk reads the neutral cell (+inf, sign +: never a minimum) and no message, contributes
// mag = 0 (x + 0 = x) and stores nothing.
//
// Positions.  32-bit byte offsets in device memory as in bp_layered_block.hip, but a thread holds ONE chunk of them and the
// next: the 8 entries of the chunk that follows — of the same pass, of pass 2, or chunk 0 of the next step — are fetched
// before the arithmetic of the current chunk, so across a barrier it is still "the next step's positions are under way
// while this one computes".  Pass 2 reads the table a second time (L2 / vector cache hits).
//
// Message cells of a wide check: R[check][edge] as everywhere, but for EVEN D the row of the check in thread l is rotated by
// l mod 32 (mod D) cells: edge j lives in cell (j + rot) mod D of its row.  Unrotated, a wavefront's accesses to edge j have a
// stride of D cells; D = 32 with fp32 messages is a stride of 32 words, all 32 lanes of a half-wavefront on ONE bank
// (ds_read_b32 / ds_write_b32: bank = word mod 32, conflicts within 32-lane halves) — 32 LDS cycles instead of 1 for every
// message read and write.  Rotated, lane l is at word 32 l + (j + l) mod 32: 32 banks.  fp16, D = 32: word 16 l + ((j + l) mod
// 32) / 2, even lanes on banks 0-15, odd lanes on 16-31, no two alike.  An odd D has an odd stride (fp32) and is left alone.
// The rotation is private to this kernel: R starts at zero and never leaves LDS.
#include <hip/hip_runtime.h>

#include "launchers.hpp"

namespace acg {
#include "bp_core.inc"   // Dom<float>::phi for the sum-product instances
#include "bp_layer_math.inc"

constexpr int WIDE_MAXD = 32;
constexpr int WIDE_CHUNKS = WIDE_MAXD / LMAXD;

// one step of a frame for a check of degree <= 8 (block_layer_step of bp_layered_block.hip)
template <int D, typename RT, int ALGO>
__device__ __forceinline__ uint32_t wide_narrow_step(unsigned char *__restrict__ Pb, RT *__restrict__ Rl, const int (&pos)[LMAXD], const float scale) {
    float r[LMAXD];
#pragma unroll
    for (int j = 0; j < D; ++j) r[j] = (float) Rl[j];
    float *addr[LMAXD];
    float p[LMAXD], q[LMAXD];
    layer_front<D>(Pb, pos, r, addr, p, q);
    if constexpr (ALGO == 0) return layer_back_spa<D, 1, RT>(Rl, addr, p, q, true);
    else return layer_back<D, 1, RT>(Rl, addr, p, q, true, scale);
}

// message cell of edge e in the (rotated) row of a wide check
__device__ __forceinline__ int wide_cell(const int e, const int rot, const int D) {
    const int i = e + rot;
    return i >= D ? i - D : i;
}

// q = p - r of the 8 edges from e0 on (edges beyond D: the neutral cell, no message); of p only the signs are needed afterwards:
// bit j of psign is the hard decision of edge e0 + j (8 registers less than keeping p next to q)
template <typename RT>
__device__ __forceinline__ void wide_load(unsigned char *__restrict__ Pb, const RT *__restrict__ Rl, const int (&pos)[LMAXD], const int e0, const int rot,
                                          const int D, uint32_t &psign, float (&q)[LMAXD]) {
    float p[LMAXD];
#pragma unroll
    for (int j = 0; j < LMAXD; ++j) p[j] = *reinterpret_cast<const float *>(Pb + pos[j]);
    psign = 0;
#pragma unroll
    for (int j = 0; j < LMAXD; ++j) {
        float r = 0.0f;
        if (e0 + j < D) r = (float) Rl[wide_cell(e0 + j, rot, D)];
        q[j] = p[j] - r;
        psign |= (__float_as_uint(p[j]) >> 31) << j;
    }
}

// One step of a frame for a check of degree D = 9 ... 32 (see the head of the file).  posn: the positions of chunk 0 on entry,
// those of chunk 0 of the next step kn on return; fetch(k, c, posn) is the kernel's position fetch.
// `active`: this thread has a check in the step (the others only keep the position pipeline going).
// -> sign bit set <=> the step was not quiet for this thread
template <typename RT, int ALGO, typename Fetch>
__device__ __forceinline__ uint32_t wide_layer_step(unsigned char *__restrict__ Pb, RT *__restrict__ Rl, const int D, const int rot, const bool active,
                                                    int (&posn)[LMAXD], const Fetch fetch, const int k, const int kn, const float scale) {
    const int nc = (D + LMAXD - 1) / LMAXD;
    uint32_t S = 0, parity = 0, flipped = 0;
    float m1 = INFINITY, m2 = INFINITY;     // min-sum
    float mag[WIDE_MAXD], base[WIDE_CHUNKS];  // sum-product
    float s = 0.0f;
    // ---- pass 1: the reductions over the whole check ------------------------------------------------------------------------
#pragma unroll
    for (int c = 0; c < WIDE_CHUNKS; ++c) {
        if (c < nc) {
            int pos[LMAXD];
#pragma unroll
            for (int j = 0; j < LMAXD; ++j) pos[j] = posn[j];
            if (c + 1 < nc) fetch(k, c + 1, posn);   // (the last chunk of pass 1 is the first of pass 2: its positions stay)
            if (active) {
                float q[LMAXD];
                uint32_t psign;
                wide_load<RT>(Pb, Rl, pos, c * LMAXD, rot, D, psign, q);
                parity ^= psign;                                        // parity of the hard decisions this check sees
                if constexpr (ALGO == 0) base[c] = s;
#pragma unroll
                for (int j = 0; j < LMAXD; ++j) {
                    S ^= __float_as_uint(q[j]);
                    const float a = __uint_as_float(__float_as_uint(q[j]) & 0x7FFFFFFFu);
                    if constexpr (ALGO == 0) {
                        float m = 0.0f;
                        if (c * LMAXD + j < D) m = Dom<float>::phi(a);
                        mag[c * LMAXD + j] = m;
                        s += m;
                    } else {
                        m2 = __builtin_amdgcn_fmed3f(a, m1, m2);
                        m1 = __builtin_fminf(m1, a);
                    }
                }
            }
        }
    }
    // the two minima are scaled once per check and rounded once to the storage type (layer_back)
    uint32_t m1s = 0, m2s = 0;
    if constexpr (ALGO == 1) {
        m1s = __float_as_uint((float) (RT) (scale * m1)) & 0x7FFFFFFFu;
        m2s = __float_as_uint((float) (RT) (scale * m2)) & 0x7FFFFFFFu;
        asm volatile("" : "+v"(m1s), "+v"(m2s));
    }
    // ---- pass 2: new messages and posteriors, chunk by chunk from the last ------------------------------------------------------
    float suf = 0.0f;
#pragma unroll
    for (int c = WIDE_CHUNKS - 1; c >= 0; --c) {
        if (c < nc) {
            int pos[LMAXD];
#pragma unroll
            for (int j = 0; j < LMAXD; ++j) pos[j] = posn[j];
            if (c > 0) fetch(k, c - 1, posn);
            else fetch(kn, 0, posn);
            if (active) {
                // (the rotation through opaque copies: the compiler would otherwise keep the 32 cell addresses of pass 1 alive for
                // pass 2 and the stores — 32 registers for three instructions per access)
                int rot_l = rot, rot_s = rot;
                asm volatile("" : "+v"(rot_l), "+v"(rot_s));
                float q[LMAXD];
                uint32_t psign;
                wide_load<RT>(Pb, Rl, pos, c * LMAXD, rot_l, D, psign, q);
                float pre[LMAXD];
                if constexpr (ALGO == 0) {
                    float t = base[c];
#pragma unroll
                    for (int j = 0; j < LMAXD; ++j) {
                        pre[j] = t;
                        t += mag[c * LMAXD + j];
                    }
                }
#pragma unroll
                for (int j = LMAXD - 1; j >= 0; --j) {
                    if (c * LMAXD + j < D) {
                        uint32_t mg;
                        if constexpr (ALGO == 0) {
                            float out = __builtin_fminf(Dom<float>::phi(pre[j] + suf), LAYERED_SPA_SATURATION);
                            suf += mag[c * LMAXD + j];
                            out = (float) (RT) out;                      // (fp16 storage: P' adds exactly what the next iteration subtracts)
                            mg = __float_as_uint(out) & 0x7FFFFFFFu;
                        } else {
                            const float a = __uint_as_float(__float_as_uint(q[j]) & 0x7FFFFFFFu);
                            mg = (a == m1) ? m2s : m1s;                  // a tie makes m2 == m1: either answer is the same
                        }
                        const float rn = __uint_as_float(mg | ((S ^ __float_as_uint(q[j])) & 0x80000000u));
                        const float pn = q[j] + rn;
                        flipped |= (__float_as_uint(pn) >> 31) ^ (psign >> j);  // (bit 0) a hard decision flipped
                        *reinterpret_cast<float *>(Pb + pos[j]) = pn;
                        Rl[wide_cell(c * LMAXD + j, rot_s, D)] = (RT) rn;         // (exact: the magnitude is already a value of RT)
                    }
                }
            }
        }
    }
    return ((__builtin_popcount(parity) | flipped) & 1u) << 31;
}

// RT: storage type of the messages (float, or _Float16 with ACG_LDPC_PREC_F16); ALGO: 1 = normalised min-sum, 0 = sum-product
template <int L, typename RT, int ALGO>
__global__ void __launch_bounds__(L) bp_layered_wide_kernel(const LayerBlockTables t, const DecodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned long long fr_lds;
    const int l = threadIdx.x;
    unsigned char *Pb = smem;
    float *P = reinterpret_cast<float *>(smem);              // P[n] + neutral cell (+ padding to a multiple of 4 words)
    RT *R = reinterpret_cast<RT *>(P + t.p_words);
    uint32_t *OB = reinterpret_cast<uint32_t *>(P + t.p_words + t.r_words);
    const float scale = a.ms_scale;
    const int NS = t.n_steps;
    const int neutral = 4 * t.n;

    // positions of chunk c (edges 8 c ... 8 c + 7) of step k for this thread (the neutral cell where it has no such edge)
    auto fetch = [tstep = t.step, tpos = t.pos, l, neutral](const int k, const int c, int (&pos)[LMAXD]) {
        const int deg = lsload(tstep, 8 * k), toff = lsload(tstep, 8 * k + 3), cnt = lsload(tstep, 8 * k + 4), stride = lsload(tstep, 8 * k + 5);
        const int32_t *T = tpos + toff + (size_t) (c * LMAXD) * stride;   // (scalar: the lane is the vector offset of every load)
#pragma unroll
        for (int j = 0; j < LMAXD; ++j) pos[j] = (c * LMAXD + j < deg && l < cnt) ? (T + (size_t) j * stride)[l] : neutral;
    };
    // explicit syndrome of the posteriors' signs (frames that ran out of iterations without a quiet round)
    auto syndrome_bad = [&]() -> bool {
        uint32_t acc = 0;
        for (int k = 0; k < NS; ++k) {
            const int deg = lsload(t.step, 8 * k), toff = lsload(t.step, 8 * k + 3), cnt = lsload(t.step, 8 * k + 4), stride = lsload(t.step, 8 * k + 5);
            if (l < cnt) {
                const int32_t *T = t.pos + toff + l;
                uint32_t S = 0;
                for (int j = 0; j < deg; ++j) S ^= __float_as_uint(*reinterpret_cast<const float *>(Pb + T[(size_t) j * stride]));
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
        // ---- start of a frame: P = channel LLR (channel.h:14-16), R = 0 ------------------------------------------------------
        for (int v = l; v < t.n; v += L) {
            float llr;
            if (a.y_is_f64) llr = (float) (2 * reinterpret_cast<const double *>(a.y)[(size_t) frame * t.n + v] / a.var);
            else llr = (float) ((double) reinterpret_cast<const float *>(a.y)[(size_t) frame * t.n + v] * a.inv_var2);
            P[v] = (ALGO == 0) ? llr * (float) Dom<float>::scale : llr;
        }
        for (int w = t.n + l; w < t.p_words; w += L) P[w] = INFINITY;   // neutral cell: never the minimum, sign +
        for (int w = l; w < t.e; w += L) R[w] = (RT) 0.0f;
        int posn[LMAXD];
        fetch(0, 0, posn);
        int it = 0;             // iterations (rounds over all sets) this frame has been through
        bool latched = false;
        uint32_t noisy_acc = 0; // sign bit: some step of the current round was not quiet for this thread's checks
        for (;;) {
            // ---- round boundary (and the barrier behind the frame's start / the last set) -----------------------------------
            const bool loud = __syncthreads_or((noisy_acc >> 31) != 0u ? 1 : 0) != 0;
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
                        const unsigned long long b = __ballot(v < t.n && (__float_as_uint(P[v < t.n ? v : t.n]) >> 31) != 0u);
                        if ((l & 63) == 0) {
                            OB[v0 >> 5] = (uint32_t) b;
                            if ((v0 >> 5) + 1 < t.nwords) OB[(v0 >> 5) + 1] = (uint32_t) (b >> 32);
                        }
                    }
                } else {
                    for (int w = l; w < t.nwords; w += L) OB[w] = 0u;
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
                const int deg = lsload(t.step, 8 * k), barrier = lsload(t.step, 8 * k + 1), roff = lsload(t.step, 8 * k + 2), cnt = lsload(t.step, 8 * k + 4);
                const int kn = k + 1 < NS ? k + 1 : 0;
                RT *Rl = R + roff + (size_t) l * deg;
                if (deg <= LMAXD) {
                    int pos[LMAXD];
#pragma unroll
                    for (int j = 0; j < LMAXD; ++j) pos[j] = posn[j];
                    fetch(kn, 0, posn);
                    if (l < cnt) {
                        uint32_t noisy = 0;
#define ACG_CALL(D) noisy = wide_narrow_step<D, RT, ALGO>(Pb, Rl, pos, scale)
                        ACG_LAYER_SWITCH(deg, ACG_CALL)
#undef ACG_CALL
                        noisy_acc |= noisy;
                    }
                } else {
                    // even degrees: the check's row of message cells is rotated by the lane (LDS banks; see the head of the file)
                    int rot = 0;
                    if ((deg & 1) == 0) {
                        rot = l & 31;
#pragma unroll
                        for (int i = 0; i < 3; ++i) rot -= rot >= deg ? deg : 0;   // (31 < 4 * 9)
                    }
                    noisy_acc |= wide_layer_step<RT, ALGO>(Pb, Rl, deg, rot, l < cnt, posn, fetch, k, kn, scale);
                }
                if (barrier) __syncthreads();
            }
            it += 1;
        }
    }
}

template <typename RT, int ALGO>
static const void *layered_wide_ptr_l(int L) {
    switch (L) {
        case 256: return (const void *) bp_layered_wide_kernel<256, RT, ALGO>;
        case 512: return (const void *) bp_layered_wide_kernel<512, RT, ALGO>;
        case 1024: return (const void *) bp_layered_wide_kernel<1024, RT, ALGO>;
        default: return nullptr;
    }
}

// algo: 0 sum-product, 1 min-sum; f16: messages stored in half precision.  Decode only, as bp_layered_block_kernel.
const void *bp_layered_wide_kernel_ptr(int L, bool f16, int algo) {
    if (algo == 0) return f16 ? layered_wide_ptr_l<_Float16, 0>(L) : layered_wide_ptr_l<float, 0>(L);
    return f16 ? layered_wide_ptr_l<_Float16, 1>(L) : layered_wide_ptr_l<float, 1>(L);
}

}  // namespace acg
