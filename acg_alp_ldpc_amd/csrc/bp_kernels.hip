// Fused belief-propagation kernels for gfx950 (MI355X).
//
// Replaces, for a whole batch of frames per launch, the reference's per-frame
//   BeliefPropagation::decode            algo/bp.h:183-199
//   c_receive_messages / VNode::message  algo/bp.h:160-169, 77-83   (variable -> check)
//   v_receive_messages / CNode::message  algo/bp.h:171-181, 49-57   (check -> variable)
//   VNode::estimate + IsCodeword         algo/bp.h:85-90, 191-196 ; utils/codeword.h:90-95
// and, in Monte-Carlo mode, transmit (utils/channel.h:18-26) and the per-frame classification
// of exp() (experiment.h:109-120).
//
// Mapping: L lanes of a 64-wide wavefront (L = 64, 32 or 16) cooperate on ONE
// frame; the frame's E messages live in LDS for all iterations, updated in place, so HBM sees
// only the channel symbols in and the packed hard decisions out.  The Tanner graph is shared by
// every frame of the launch, so all graph indices are either implicit in the layout (check side:
// unit-stride, bank-conflict-free) or small read-only tables (variable side).  No cross-lane
// traffic is needed inside a phase: each lane owns whole nodes and forms the exclude-self sums
// (bp.h:50-55, 78-81) with a prefix/suffix scan in registers.  The per-check parity of the hard
// decisions rides in the LSB of each v->c magnitude, so the syndrome test costs one XOR per edge
// and a wave ballot.
//
// Source layout: bp_core.inc holds the kernel; bp_inst_{spa,ms}_{f32,f64}.hip instantiate it (parallel
// compilation); this file holds the dispatcher, the launcher and the phi debug kernels.  The stand-alone Monte-Carlo kernels
// (AWGN generator, classification) are in mc_kernels.hip.
//
// A wavefront is a persistent worker: each L-lane group walks frames g, g+G, g+2G, ... and
// restarts on a new frame the moment its current one reaches a zero syndrome (the reference's
// early exit, bp.h:195-196), independently of the other groups in the wave.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "launchers.hpp"

namespace acg {
#include "bp_core.inc"

const void *bp_kernel_ptr_dbg(int f64, int L, int sat) {
    if (sat != 0 && f64) return nullptr;
#ifdef ACG_FAST_BUILD
    return f64 ? nullptr : bp_kernel_ptr_spa_f32_dbg(L, sat);
#else
    return f64 ? bp_kernel_ptr_spa_f64_dbg(L) : bp_kernel_ptr_spa_f32_dbg(L, sat);
#endif
}

// algo: 0 sum-product, 1 min-sum; f64: 0/1; sat: the phi fast path where an instance has it (fp32 sum-product); split: of
// those, the instance with the one-series phi
const void *bp_kernel_ptr(int algo, int f64, int maxd, int L, bool mc, int variant, bool sat, bool split) {
#ifdef ACG_FAST_BUILD
    if (f64 || algo) return nullptr;
    return bp_kernel_ptr_spa_f32(maxd, L, mc, variant, sat, split);
#else
    if (algo == 0) return f64 ? bp_kernel_ptr_spa_f64(maxd, L, mc, variant) : bp_kernel_ptr_spa_f32(maxd, L, mc, variant, sat, split);
    return f64 ? bp_kernel_ptr_ms_f64(maxd, L, mc, variant) : bp_kernel_ptr_ms_f32(maxd, L, mc, variant);
#endif
}

hipError_t bp_launch(const void *kernel, const BpTables &t, const DecodeArgs &a, int grid, int block, size_t lds,
                     hipStream_t s) {
    BpTables tt = t;
    DecodeArgs aa = a;
    void *args[2] = {&tt, &aa};
    return hipLaunchKernel(kernel, dim3(grid), dim3(block), args, lds, s);
}

// ------------------------------------------------------------------------------------------
// debug / test kernels
__global__ void phi_debug_kernel(const float *x, float *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    // the fp32 kernels evaluate phi in the log2(e)-scaled domain: report it back in natural units
    if (i < n) out[i] = (float) ((double) Dom<float>::phi((float) ((double) x[i] * Dom<float>::scale)) / Dom<float>::scale);
}
__global__ void phi_debug_kernel_f64(const double *x, double *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = phi_f(x[i]);
}

// the phi fast path of the fp32 sum-product sweeps against the full evaluation, raw bits in the scaled domain:
// out[3i] = Dom<float>::phi(x), out[3i+1] = BpPass::phi_c(x) (check side), out[3i+2] = BpPass::phi_v(|x|) (variable side)
__global__ void phi_sat_debug_kernel(const float *x, uint32_t *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    using P = BpPass<float, 1, 64, 0, true>;
    if (i < n) {
        out[3 * i] = __float_as_uint(Dom<float>::phi(x[i]));
        out[3 * i + 1] = __float_as_uint(P::phi_c(x[i]));
        out[3 * i + 2] = __float_as_uint(P::phi_v(__builtin_fabsf(x[i])));
    }
}

hipError_t phi_sat_debug_launch(const float *x, uint32_t *out, int n, hipStream_t s) {
    hipLaunchKernelGGL(phi_sat_debug_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x, out, n);
    return hipGetLastError();
}

// The one-series phi of the split sweeps against the full evaluation, over every non-negative fp32 bit pattern (NaNs included).
// out (PHI_SPLIT_NOUT words, set up by the launcher): [0] patterns whose one series does not give phi's bits — phi_large on
// 2 <= x < 66, phi_small on 0 < x <= 1 — [1] the smallest such pattern, [2] the largest finite x > 0 with ps >= pl, [3] the
// smallest x > 0 with pl >= ps (between them either series is right: the distance to the thresholds is the margin), [4]
// patterns where max(ps, pl) behind phi's saturation select, the full path of a split row, does not give phi's bits, [5] the
// smallest such pattern.  Grid-stride; one atomic per counter and thread.
__global__ void phi_split_debug_kernel(uint32_t *out) {
    uint32_t bad = 0, first = 0xFFFFFFFFu, top_small = 0u, low_large = 0xFFFFFFFFu, bad_full = 0, first_full = 0xFFFFFFFFu;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < 0x80000000ull; i += stride) {
        const uint32_t b = (uint32_t) i;
        const float x = __uint_as_float(b);
        const uint32_t full = __float_as_uint(Dom<float>::phi(x));
        const float ps = Dom<float>::phi_small(x), pl = Dom<float>::phi_large(x);
        if (x >= ACG_PHI_SPLIT_HI && x < 66.0f && __float_as_uint(pl) != full) bad += 1, first = b < first ? b : first;
        if (x > 0.0f && x <= ACG_PHI_SPLIT_LO && __float_as_uint(ps) != full) bad += 1, first = b < first ? b : first;
        if (x > 0.0f && x < 66.0f) {
            if (ps >= pl) top_small = b > top_small ? b : top_small;
            if (pl >= ps) low_large = b < low_large ? b : low_large;
        }
        float o = __builtin_fmaxf(ps, pl);
        o = (x >= 66.0f) ? 0.0f : o;
        if (__float_as_uint(o) != full) bad_full += 1, first_full = b < first_full ? b : first_full;
    }
    if (bad) atomicAdd(&out[0], bad);
    atomicMin(&out[1], first);
    atomicMax(&out[2], top_small);
    atomicMin(&out[3], low_large);
    if (bad_full) atomicAdd(&out[4], bad_full);
    atomicMin(&out[5], first_full);
}

hipError_t phi_split_debug_launch(uint32_t *out, hipStream_t s) {
    const uint32_t init[PHI_SPLIT_NOUT] = {0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu};
    if (hipError_t e = hipMemcpyAsync(out, init, sizeof(init), hipMemcpyHostToDevice, s)) return e;
    hipLaunchKernelGGL(phi_split_debug_kernel, dim3(4096), dim3(256), 0, s, out);
    return hipGetLastError();
}

hipError_t phi_debug_launch(const void *x, void *out, int n, int f64, hipStream_t s) {
    if (f64)
        hipLaunchKernelGGL(phi_debug_kernel_f64, dim3((n + 255) / 256), dim3(256), 0, s, (const double *) x, (double *) out, n);
    else
        hipLaunchKernelGGL(phi_debug_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const float *) x, (float *) out, n);
    return hipGetLastError();
}

}  // namespace acg
