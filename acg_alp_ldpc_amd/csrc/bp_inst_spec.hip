// Instances of the fused BP kernel with a code's pass structure constant (bp_core.inc, static pass policy), one pair
// (MC off / on) per code of SPEC_CODES: the fixed-work fp32 sum-product kernel with the phi fast path, degree <= 8, index table
// in LDS, LLRs in registers.  The include with the policies, the kernels and the registry lines is written by
// tools/bp_spec_gen.cpp when the library is built (_obj/bp_spec_gen.inc, see the Makefile).  Each pair lives in a namespace of
// its own, spec_<name>, under the kernel name and template arguments of the instance it stands in for (as sat:: does).
#include <hip/hip_runtime.h>

#include "bp_spec.hpp"
#include "launchers.hpp"

namespace acg {
#include "bp_core.inc"

constexpr int BP_NVP = 12;  // as bp_inst_spa_f32.hip: the instances these stand in for

namespace {
struct BpSpecEntry {
    BpSpecSig sig;
    const void *kernel[3];  // MC off / on; then MC off with the one-series phi (split::)
};
}  // namespace

#include "bp_spec_gen.inc"

static const BpSpecEntry spec_entries[] = {ACG_BP_SPEC_ENTRIES {{nullptr, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}}};

// the instance whose signature equals the layout's (bp_spec_matches), or null; *name, *sat_rows: the entry's; split: the instance
// with the one-series phi (there is none with the Monte-Carlo generator)
const void *bp_spec_kernel_ptr(const BpLayout &lay, bool mc, const char **name, const char **sat_rows, bool split, const char **split_rows) {
    for (const BpSpecEntry *e = spec_entries; e->sig.name; ++e) {
        if (bp_spec_matches(e->sig, lay)) {
            if (name) *name = e->sig.name;
            if (sat_rows) *sat_rows = e->sig.sat_rows;
            if (split_rows) *split_rows = e->sig.split_rows;
            return e->kernel[mc ? 1 : (split ? 2 : 0)];
        }
    }
    return nullptr;
}

}  // namespace acg
