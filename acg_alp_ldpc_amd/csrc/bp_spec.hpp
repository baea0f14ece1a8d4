// Build-time instances of the fused BP kernel with a code's pass structure constant (bp_core.inc, static pass policy): the
// signature of such an instance and the test a decoder handle's layout has to pass to run it.  Host only, no HIP: shared by
// the generator (tools/bp_spec_gen.cpp), the registry (bp_inst_spec.hip), the handle set-up (api.hip) and the host tests.
// Not part of the ABI.
#pragma once

#include <cstdint>
#include <vector>

#include "ldpc_internal.hpp"

namespace acg {

// entries of c_cnt_ge / v_cnt_ge a degree <= 8 kernel reads (BpCore::ccnt, vcnt: MAXD + 2), zero padded
constexpr int BP_SPEC_NCNT = 10;

// Every value the static policy folds into the kernel text.  Two layouts with equal signatures run the same instance, whatever
// matrix they come from: the index tables (v_apos, v_var, a_var) and all sizes stay run-time data.
struct BpSpecSig {
    const char *name;
    int L, n_cpass, n_apass, n_vpass;
    const int32_t *c_pass;    // [n_cpass][2] = {largest degree, A offset}, as BpTables::c_pass
    const int32_t *v_pass;    // [n_vpass][2] = {largest degree, index-table offset}
    const int32_t *c_cnt_ge;  // [BP_SPEC_NCNT]
    const int32_t *v_cnt_ge;  // [BP_SPEC_NCNT]
    // Not part of the match: the rows of the instance that keep their phi fast-path test (the policy's c_sat_rows / v_sat_rows,
    // hexadecimal, one mask per pass: "c:7f,3f,30,1f,f/v:3f,...") with the census SNR and threshold they come from; results do
    // not depend on them
    const char *sat_rows = nullptr;
    // likewise not part of the match: the rows that take the one-series phi where the wavefront allows (c_split_rows /
    // v_split_rows, same form without the census part; all rows unless the generator was given -r)
    const char *split_rows = nullptr;
};

// the signature's tables of a layout, owned
struct BpSpecTables {
    int L = 0, n_cpass = 0, n_apass = 0, n_vpass = 0;
    std::vector<int32_t> c_pass, v_pass, c_cnt_ge, v_cnt_ge;
    BpSpecSig sig(const char *name) const {
        return BpSpecSig{name, L, n_cpass, n_apass, n_vpass, c_pass.data(), v_pass.data(), c_cnt_ge.data(), v_cnt_ge.data()};
    }
};

inline BpSpecTables bp_spec_tables(const BpLayout &lay) {
    BpSpecTables s;
    s.L = lay.L;
    s.n_cpass = lay.n_cpass;
    s.n_apass = lay.n_apass;
    s.n_vpass = lay.n_vpass;
    for (int p = 0; p < lay.n_cpass; p++) {
        s.c_pass.push_back(lay.c_maxdeg[p]);
        s.c_pass.push_back(lay.c_off[p]);
    }
    for (int p = 0; p < lay.n_vpass; p++) {
        s.v_pass.push_back(lay.v_maxdeg[p]);
        s.v_pass.push_back(lay.v_idx_off[p]);
    }
    s.c_cnt_ge.assign(BP_SPEC_NCNT, 0);
    s.v_cnt_ge.assign(BP_SPEC_NCNT, 0);
    for (size_t i = 0; i < lay.c_cnt_ge.size() && i < (size_t) BP_SPEC_NCNT; i++) s.c_cnt_ge[i] = lay.c_cnt_ge[i];
    for (size_t i = 0; i < lay.v_cnt_ge.size() && i < (size_t) BP_SPEC_NCNT; i++) s.v_cnt_ge[i] = lay.v_cnt_ge[i];
    return s;
}

// the layout of a handle against the signature of an instance: every folded constant takes part
inline bool bp_spec_matches(const BpSpecSig &s, const BpLayout &lay) {
    if (lay.max_cdeg > 8 || lay.max_vdeg > 8) return false;  // (BP_SPEC_NCNT entries would not hold the histograms)
    if (s.L != lay.L || s.n_cpass != lay.n_cpass || s.n_apass != lay.n_apass || s.n_vpass != lay.n_vpass) return false;
    const BpSpecTables t = bp_spec_tables(lay);
    for (int i = 0; i < 2 * s.n_cpass; i++)
        if (s.c_pass[i] != t.c_pass[i]) return false;
    for (int i = 0; i < 2 * s.n_vpass; i++)
        if (s.v_pass[i] != t.v_pass[i]) return false;
    for (int i = 0; i < BP_SPEC_NCNT; i++)
        if (s.c_cnt_ge[i] != t.c_cnt_ge[i] || s.v_cnt_ge[i] != t.v_cnt_ge[i]) return false;
    return true;
}

}  // namespace acg
