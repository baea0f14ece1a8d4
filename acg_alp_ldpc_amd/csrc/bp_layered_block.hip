// Workgroup-per-frame layered BP — the layered schedule of bp_layered.hip (conflict-free same-degree sets of checks, posteriors
// updated in place after every set) for codes whose frame is too large for a wavefront group: one workgroup of L = 256, 512 or
// 1024 threads owns a frame, all of the frame's state lives in LDS for the whole decode, and the graph description stays in
// device memory.  What bp_block.hip is to the flooding kernels.  The per-check arithmetic is bp_layer_math.inc, the same
// functions bp_layered_kernel calls; the stopping rule is the same too (a round in which every step was quiet), so a code both
// engines accept with the same sets decodes to the same words, flags and iteration counts.
//
// Sets.  A set may hold more checks than the workgroup has threads (LayeredBlockLayout: first-fit colouring without a cap, or
// the block rows of a quasi-cyclic H): it is worked off in ceil(cnt / L) passes, thread l taking check l + pass * L.  The checks
// of a set share no variable, so its passes need no barrier between them; one __syncthreads() separates consecutive sets, and
// the workgroup-wide OR that ends an iteration is the barrier behind the last one.  The host flattens (set, pass) into STEPS
// (LayerBlockTables::step): the kernel walks one list.
//
// LDS of the workgroup: P[n] posteriors (fp32) + the neutral cell | R: one message cell per edge, fp32 or _Float16 | the packed
// output word.  Nothing else: for the (3,6)-regular 5000 x 10000 code that is 10 004 + 30 000 + 313 words = 161 268 of the
// 163 840 bytes of a CU, which leaves no room for padding of any kind.  Hence the message layout: R[check][edge], the checks in
// set / slot order — edge j of a check sits j cells behind its edge 0 (G = 1 in bp_layer_math.inc), whatever the size of the
// set.  A wavefront's D accesses of a step cover 64 D consecutive cells between them; taken one instruction at a time they have
// stride D cells (fp32, D = 6: two lanes per bank and 32-lane group; fp16, D = 6: 12 bytes, conflict-free).  Rows of 64 lanes
// would be conflict-free for every D but pad every set to a multiple of 64 checks: 168 756 bytes for that code.
//
// Positions.  Which posterior cell edge j of the check in (set, slot) reads is a 32-bit byte offset in device memory at
// pos[set offset + j * cnt + slot]: consecutive lanes read consecutive entries, every workgroup reads the same table (it stays
// in L2), and nothing limits n but the LDS.  The entries of the NEXT step are fetched before the arithmetic of the current one
// (they depend on the table alone), so their latency hides behind the step and its barrier.
#include <hip/hip_runtime.h>

#include "launchers.hpp"

namespace acg {
#include "bp_core.inc"   // Dom<float>::phi for the sum-product instances
#include "bp_layer_math.inc"

// one step of a frame: old messages of this thread's check, posteriors through the prefetched positions, arithmetic, stores
template <int D, typename RT, int ALGO>
__device__ __forceinline__ uint32_t block_layer_step(unsigned char *__restrict__ Pb, RT *__restrict__ Rl, const int (&pos)[LMAXD], const float scale) {
    float r[LMAXD];
#pragma unroll
    for (int j = 0; j < D; ++j) r[j] = (float) Rl[j];
    float *addr[LMAXD];
    float p[LMAXD], q[LMAXD];
    layer_front<D>(Pb, pos, r, addr, p, q);
    if constexpr (ALGO == 0) return layer_back_spa<D, 1, RT>(Rl, addr, p, q, true);
    else return layer_back<D, 1, RT>(Rl, addr, p, q, true, scale);
}

// RT: storage type of the messages (float, or _Float16 with ACG_LDPC_PREC_F16); ALGO: 1 = normalised min-sum, 0 = sum-product
template <int L, typename RT, int ALGO>
__global__ void __launch_bounds__(L) bp_layered_block_kernel(const LayerBlockTables t, const DecodeArgs a) {
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

    // positions of step k for this thread (the neutral cell where it has no check in that step)
    auto fetch = [&](const int k, int (&pos)[LMAXD]) {
        const int deg = lsload(t.step, 8 * k), toff = lsload(t.step, 8 * k + 3), cnt = lsload(t.step, 8 * k + 4), stride = lsload(t.step, 8 * k + 5);
        const int32_t *T = t.pos + toff + l;
#pragma unroll
        for (int j = 0; j < LMAXD; ++j) pos[j] = (j < deg && l < cnt) ? T[(size_t) j * stride] : neutral;
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
        fetch(0, posn);
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
                int pos[LMAXD];
#pragma unroll
                for (int j = 0; j < LMAXD; ++j) pos[j] = posn[j];
                fetch(k + 1 < NS ? k + 1 : 0, posn);
                if (l < cnt) {
                    uint32_t noisy = 0;
#define ACG_CALL(D) noisy = block_layer_step<D, RT, ALGO>(Pb, R + roff + (size_t) l * D, pos, scale)
                    ACG_LAYER_SWITCH(deg, ACG_CALL)
#undef ACG_CALL
                    noisy_acc |= noisy;
                }
                if (barrier) __syncthreads();
            }
            it += 1;
        }
    }
}

template <typename RT, int ALGO>
static const void *layered_block_ptr_l(int L) {
    switch (L) {
        case 256: return (const void *) bp_layered_block_kernel<256, RT, ALGO>;
        case 512: return (const void *) bp_layered_block_kernel<512, RT, ALGO>;
        case 1024: return (const void *) bp_layered_block_kernel<1024, RT, ALGO>;
        default: return nullptr;
    }
}

// algo: 0 sum-product, 1 min-sum; f16: messages stored in half precision.  Decode only: a Monte-Carlo run on such a handle goes
// AWGN kernel -> this kernel -> classification kernel.
const void *bp_layered_block_kernel_ptr(int L, bool f16, int algo) {
    if (algo == 0) return f16 ? layered_block_ptr_l<_Float16, 0>(L) : layered_block_ptr_l<float, 0>(L);
    return f16 ? layered_block_ptr_l<_Float16, 1>(L) : layered_block_ptr_l<float, 1>(L);
}

// The launch of the three workgroup-per-frame layered kernels (this file's, bp_layered_wide.hip's and bp_layered_q.hip's); q: the
// third argument of bp_layered_q_kernel, null for the float kernels; g: the fourth of bp_layered_q_grid_kernel
hipError_t bp_layered_wg_launch(const void *kernel, const LayerBlockTables &t, const DecodeArgs &a, const QuantArgs *q, int grid, int block, size_t lds,
                                hipStream_t s, const QuantGridArgs *g) {
    LayerBlockTables tt = t;
    DecodeArgs aa = a;
    QuantArgs qq = q ? *q : QuantArgs{};
    QuantGridArgs gg = g ? *g : QuantGridArgs{};
    void *args[4] = {&tt, &aa, &qq, &gg};   // (hipLaunchKernel reads as many as the kernel has parameters)
    return hipLaunchKernel(kernel, dim3(grid), dim3(block), args, lds, s);
}

}  // namespace acg
