// Instantiations of the fused BP kernel for T = float, ALGO = 0 (sum-product, fp32).
#include <hip/hip_runtime.h>

#include "launchers.hpp"

namespace acg {
#include "bp_core.inc"

constexpr int BP_NVP = 12;  // register-resident LLRs for codes with <= 12 variable passes (n <= 12 * L)

// variant: 0 = index table read from global, LLR in LDS; 1 = index table in LDS, LLR in LDS;
//          2 = index table in LDS, LLR in registers (degree <= 8 kernels only)
// sat: the phi fast path (BpCore::SATSKIP), instantiated for variant 2
// split: those instances with the one-series phi (split::; degree <= 8, the ones with the freeze path)
template <int MAXD, int L>
static const void *kptr(bool mc, int variant, bool sat, bool split) {
    if constexpr (MAXD <= 8) {
        // (not L = 64 and not the Monte-Carlo instances: there the split sweeps cost scratch that the instances without them do
        // not need, profiles/r17_phisplit_summary.md)
        if constexpr (L <= 32) {
            if (variant == 2 && sat && split && !mc) return (const void *) split::bp_fused_kernel<float, MAXD, L, 0, false, true, BP_NVP>;
        }
    }
    if (MAXD <= 8 && variant == 2 && sat)
        return mc ? (const void *) sat::bp_fused_kernel<float, MAXD, L, 0, true, true, (MAXD <= 8 ? BP_NVP : 0)>
                  : (const void *) sat::bp_fused_kernel<float, MAXD, L, 0, false, true, (MAXD <= 8 ? BP_NVP : 0)>;
    if (MAXD <= 8 && variant == 2)
        return mc ? (const void *) bp_fused_kernel<float, MAXD, L, 0, true, true, (MAXD <= 8 ? BP_NVP : 0)>
                  : (const void *) bp_fused_kernel<float, MAXD, L, 0, false, true, (MAXD <= 8 ? BP_NVP : 0)>;
    if (variant >= 1)
        return mc ? (const void *) bp_fused_kernel<float, MAXD, L, 0, true, true, 0>
                  : (const void *) bp_fused_kernel<float, MAXD, L, 0, false, true, 0>;
    return mc ? (const void *) bp_fused_kernel<float, MAXD, L, 0, true, false, 0>
              : (const void *) bp_fused_kernel<float, MAXD, L, 0, false, false, 0>;
}

template <int MAXD>
static const void *kptr_l(int L, bool mc, int variant, bool sat, bool split) {
    switch (L) {
        case 64: return kptr<MAXD, 64>(mc, variant, sat, split);
        case 32: return kptr<MAXD, 32>(mc, variant, sat, split);
        case 16: return kptr<MAXD, 16>(mc, variant, sat, split);
        default: return nullptr;
    }
}

const void *bp_kernel_ptr_spa_f32(int maxd, int L, bool mc, int variant, bool sat, bool split) {
    if (maxd <= 8) return kptr_l<8>(L, mc, variant, sat, split);
#ifndef ACG_FAST_BUILD
    if (maxd <= 16) return kptr_l<16>(L, mc, variant, sat, false);
    if (maxd <= 32) return kptr_l<32>(L, mc, variant, sat, false);
#endif
    return nullptr;
}

// tests only (acg_ldpc_debug_bp_trace): the headline instance (degree <= 8, index table in LDS, LLRs in registers) with
// the message dump compiled in
// sat: 1 = the fixed-work instance with the phi fast path, 2 = that with the one-series phi as well (L = 32), each with the dump
const void *bp_kernel_ptr_spa_f32_dbg(int L, int sat) {
    if (sat == 1 && L == 32) return (const void *) sat::bp_fused_kernel<float, 8, 32, 0, false, true, BP_NVP, true>;
    if (sat == 2 && L == 32) return (const void *) split::bp_fused_kernel<float, 8, 32, 0, false, true, BP_NVP, true>;
    if (sat != 0) return nullptr;
    if (L == 64) return (const void *) bp_fused_kernel<float, 8, 64, 0, false, true, BP_NVP, true>;
    if (L == 32) return (const void *) bp_fused_kernel<float, 8, 32, 0, false, true, BP_NVP, true>;
    return nullptr;
}

}  // namespace acg
