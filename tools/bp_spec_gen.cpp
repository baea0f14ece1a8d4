// Build tool: the generated include of acg_alp_ldpc_amd/csrc/bp_inst_spec.hip — for every code of SPEC_CODES one instance pair of
// the fused fixed-work sum-product kernel with the code's pass structure as compile-time constants (bp_core.inc, static pass
// policy).  Host only; csrc/Makefile builds and runs it:
//   g++ -O2 -std=c++17 -Iinclude tools/bp_spec_gen.cpp acg_alp_ldpc_amd/csrc/code.cpp -o bp_spec_gen
//   bp_spec_gen [-o out.inc] [--print] [-s <dB>] [-t <per cent>] [-r c|v:<pass>:<row>]... <matrix.txt>[:L] ...
//                                                                     (L = 16, 32 or 64; 0 or none: the library's own choice)
// Per pair it calls bp_layout_build the way the handle set-up does (absorbed degree-1 variables included) and writes
//   namespace spec_<name> { struct Pass (the constexpr tables); the kernel bp_fused_kernel<...>; the signature arrays }
// and one line of the registry macro ACG_BP_SPEC_ENTRIES: name, L, signature, kernel pointers (MC off / on, then MC off of the instance with the one-series phi).  <name> is the
// file's base name and the group width, e.g. H05_L32.  A pair whose layout does not take the fp32 sum-product, degree <= 8,
// register-LLR fixed-work path is skipped with a message.  --print: the structure of every accepted pair as plain lines on
// stdout (name / c_pass / v_pass / c_cnt_ge / v_cnt_ge / n_apass), the histograms as the layout holds them.
// The policy also says which edge rows keep their phi fast-path test (c_sat_rows / v_sat_rows, bp_core.inc): the tool runs the census
// of csrc/bp_sat_census.hpp on the layout (300 frames of at most 50 sweeps, stopped at their first state repeat, at -s dB; default
// -2) and clears the bit of every row whose share of fully skipped units is below -t per cent (default: SAT_ROWS_T below).  -t 0
// keeps every test without running the census, -t 101 clears all.  The masks, the SNR and the threshold stand in the include as a
// comment, as the two look-ups and as the registry's sat_rows string.
// A second pair of look-ups, c_split_rows / v_split_rows, says which rows take the one-series phi where the wavefront allows
// (BpPass::word_c / word_v, SPLIT): every row, unless -r c:<pass>:<row> or -r v:<pass>:<row> (repeatable) clears one for a
// measured build.  Pass and row numbers are a code's own, so -r is meant for a run with one code; it is applied to every listed
// code and refused where a code has no such row.  The masks stand in the registry as split_rows.  Results do not depend on
// either pair.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../acg_alp_ldpc_amd/csrc/bp_sat_census.hpp"
#include "../acg_alp_ldpc_amd/csrc/bp_spec.hpp"

namespace acg {
void set_error(const std::string &msg) { fprintf(stderr, "bp_spec_gen: %s\n", msg.c_str()); }
}
using namespace acg;

// default of -t: every row keeps its test.  On H05 every threshold that clears a row measured slower than none at -3, -2 and
// +2 dB (profiles/r15_satrows_summary.md), so clearing rows is an option for a code it is measured to pay on
static const double SAT_ROWS_T = 0.0;
static const int CENSUS_FRAMES = 300, CENSUS_SWEEPS = 50;

static std::string hexlist(const std::vector<uint32_t> &v, const std::vector<int32_t> &pass) {
    std::string s;
    char b[16];
    for (size_t p = 0; p < v.size(); p++) {
        const int D = pass[2 * p];  // the rows the pass has
        snprintf(b, sizeof b, "%s%x", p ? "," : "", (unsigned) (v[p] & (D >= 32 ? ~0u : ((1u << D) - 1u))));
        s += b;
    }
    return s;
}

static std::string list(const std::vector<int32_t> &v) {
    std::string s;
    for (size_t i = 0; i < v.size(); i++) s += (i ? "," : "") + std::to_string(v[i]);
    return s;
}

// The layout a default fixed-work fp32 sum-product decoder of this code runs at L lanes per frame, by the handle set-up's own
// decisions (bp_layout_absorb, bp_wave_plan): the fused kernel with the index table in LDS and the LLRs in registers (variant
// 2) is the one the instances stand in for; false + why: another path
static bool spec_layout(const Code &c, int L, BpLayout &lay, std::string &why) {
    if (std::max(c.max_cdeg, c.max_vdeg) > 8) return why = "node degree > 8", false;
    if (L != 16 && L != 32 && L != 64) return why = "not a wavefront-group width (16, 32, 64): " + std::to_string(L), false;
    if (!bp_layout_build(c, L, lay) || !bp_layout_absorb(c, L, lay)) return why = "no layout", false;
    const BpWavePlan w = bp_wave_plan(c, lay, false);
    if (w.waves == 0) return why = "a wavefront's frames do not fit in LDS", false;
    if (w.variant != 2)
        return why = !w.a_fits16 ? "message array of 64 KiB or more" : !w.llr_regs ? "more than 12 variable passes: LLRs in LDS" : "index table not in LDS", false;
    return true;
}

int main(int argc, char **argv) {
    const char *out_path = nullptr;
    bool print = false;
    double snr = -2.0, thr = SAT_ROWS_T;
    std::vector<std::string> pairs;
    struct Clear { char side; int pass, row; };
    std::vector<Clear> clears;
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-o") && i + 1 < argc) out_path = argv[++i];
        else if (!strcmp(argv[i], "--print")) print = true;
        else if (!strcmp(argv[i], "-s") && i + 1 < argc) snr = atof(argv[++i]);
        else if (!strcmp(argv[i], "-t") && i + 1 < argc) thr = atof(argv[++i]);
        else if (!strcmp(argv[i], "-r") && i + 1 < argc) {
            Clear c{};
            if (sscanf(argv[++i], "%c:%d:%d", &c.side, &c.pass, &c.row) != 3 || (c.side != 'c' && c.side != 'v') || c.pass < 0 || c.row < 0 || c.row > 31) {
                fprintf(stderr, "bp_spec_gen: -r takes c:<pass>:<row> or v:<pass>:<row>, not %s\n", argv[i]);
                return 2;
            }
            clears.push_back(c);
        }
        else pairs.push_back(argv[i]);
    }
    if (pairs.empty() && !out_path) {
        fprintf(stderr, "usage: bp_spec_gen [-o out.inc] [--print] [-s <dB>] [-t <per cent>] [-r c|v:<pass>:<row>]... <matrix.txt>[:L] ...\n");
        return 2;
    }
    std::string text = "// generated by tools/bp_spec_gen.cpp from SPEC_CODES (csrc/Makefile): do not edit, do not commit\n";
    std::string entries;
    std::set<std::string> names;
    for (const std::string &pr : pairs) {
        std::string path = pr;
        int L = 0;
        const size_t colon = pr.rfind(':');
        if (colon != std::string::npos && colon + 1 < pr.size() && pr.find_first_not_of("0123456789", colon + 1) == std::string::npos) {
            path = pr.substr(0, colon);
            L = atoi(pr.c_str() + colon + 1);
        }
        std::vector<uint8_t> H;
        int m = 0, n = 0;
        Code c;
        if (!code_read_txt(path.c_str(), H, m, n) || !code_build(c, H.data(), m, n)) {
            fprintf(stderr, "bp_spec_gen: cannot read %s\n", path.c_str());
            return 1;
        }
        if (L == 0) L = bp_default_lanes(c, false);
        BpLayout lay;
        std::string why;
        if (!spec_layout(c, L, lay, why)) {
            fprintf(stderr, "bp_spec_gen: %s skipped: %s\n", pr.c_str(), why.c_str());
            continue;
        }
        size_t b = path.find_last_of('/');
        std::string name = path.substr(b == std::string::npos ? 0 : b + 1);
        name = name.substr(0, name.find('.'));
        for (char &ch : name)
            if (!((ch >= '0' && ch <= '9') || (ch >= 'a' && ch <= 'z') || (ch >= 'A' && ch <= 'Z'))) ch = '_';
        name += "_L" + std::to_string(L);
        if (!names.insert(name).second) {
            fprintf(stderr, "bp_spec_gen: %s skipped: the name %s is taken\n", pr.c_str(), name.c_str());
            continue;
        }
        const BpSpecTables s = bp_spec_tables(lay);
        // the rows that keep their fast-path test
        SatRows rows;
        if (thr > 0) rows = bp_sat_rows(bp_sat_census(c, lay, CENSUS_FRAMES, CENSUS_SWEEPS, snr, true), thr);
        else rows = bp_sat_rows(bp_sat_census_empty(lay), 0);
        char snr_s[24], thr_s[24];
        snprintf(snr_s, sizeof snr_s, "%g", snr);
        snprintf(thr_s, sizeof thr_s, "%g", thr);
        const std::string rows_str = "c:" + hexlist(rows.c, s.c_pass) + "/v:" + hexlist(rows.v, s.v_pass) + "@" + snr_s + "dB,t" + thr_s;
        if (print) {
            printf("name = %s\nL = %d\nc_pass = %s\nv_pass = %s\nc_cnt_ge = %s\nv_cnt_ge = %s\nn_apass = %d\n", name.c_str(), L, list(s.c_pass).c_str(),
                   list(s.v_pass).c_str(), list(lay.c_cnt_ge).c_str(), list(lay.v_cnt_ge).c_str(), lay.n_apass);
            fprintf(stderr, "bp_spec_gen: %s sat_rows %s\n", name.c_str(), rows_str.c_str());
        }
        const std::string ns = "spec_" + name;
        auto lookup = [&](const char *fn, const std::vector<int32_t> &v) {
            return "    static constexpr int " + std::string(fn) + "(int i) {\n        constexpr int32_t v[] = {" + list(v) + "};\n        return v[i];\n    }\n";
        };
        auto host = [&](const char *nm, const std::vector<int32_t> &v) { return "static const int32_t " + std::string(nm) + "[] = {" + list(v) + "};\n"; };
        text += "\n// " + path.substr(b == std::string::npos ? 0 : b + 1) + ", " + std::to_string(L) + " lanes per frame\nnamespace " + ns + " {\n";
        text += "struct Pass {\n    static constexpr bool STATIC = true;\n";
        text += "    static constexpr int n_cpass = " + std::to_string(s.n_cpass) + ", n_apass = " + std::to_string(s.n_apass) +
                ", n_vpass = " + std::to_string(s.n_vpass) + ";\n";
        text += lookup("c_pass", s.c_pass) + lookup("v_pass", s.v_pass) + lookup("c_cnt_ge", s.c_cnt_ge) + lookup("v_cnt_ge", s.v_cnt_ge);
        auto ulookup = [&](const char *fn, const std::vector<uint32_t> &v) {
            std::string l;
            for (size_t i = 0; i < v.size(); i++) l += (i ? "," : "") + std::to_string(v[i]) + "u";
            return "    static constexpr unsigned " + std::string(fn) + "(int p) {\n        constexpr unsigned v[] = {" + l + "};\n        return v[p];\n    }\n";
        };
        text += "    // rows that keep their phi fast-path test (bit j = edge row j of the pass): census at " + std::string(snr_s) + "dB, threshold " + thr_s +
                " per cent of fully skipped units\n    // " + rows_str + "\n";
        text += ulookup("c_sat_rows", rows.c) + ulookup("v_sat_rows", rows.v);
        // rows that take the one-series phi where their unit allows
        std::vector<uint32_t> split_c((size_t) s.n_cpass, ~0u), split_v((size_t) s.n_vpass, ~0u);
        for (const Clear &cl : clears) {
            std::vector<uint32_t> &m = cl.side == 'c' ? split_c : split_v;
            const std::vector<int32_t> &pt = cl.side == 'c' ? s.c_pass : s.v_pass;
            if ((size_t) cl.pass >= m.size() || cl.row >= pt[2 * (size_t) cl.pass]) {
                fprintf(stderr, "bp_spec_gen: -r %c:%d:%d: %s has no such row\n", cl.side, cl.pass, cl.row, name.c_str());
                return 2;
            }
            m[(size_t) cl.pass] &= ~(1u << cl.row);
        }
        const std::string split_str = "c:" + hexlist(split_c, s.c_pass) + "/v:" + hexlist(split_v, s.v_pass);
        text += "    // rows that take the one-series phi where the wavefront allows (bit j = edge row j of the pass)\n    // " + split_str + "\n";
        text += ulookup("c_split_rows", split_c) + ulookup("v_split_rows", split_v);
        text += "};\n";
        text += "template <typename T, int MAXD, int L, int ALGO, bool MC, bool IDXLDS, int NVP, bool DBG = false>\n"
                "__global__ void __launch_bounds__(256, (bp_min_waves<T, MAXD, L, NVP>())) bp_fused_kernel(const BpTables t, const DecodeArgs a) {\n"
                "    bp_fused_body<T, MAXD, L, ALGO, MC, IDXLDS, NVP, DBG, true, Pass>(t, a);\n}\n";
        text += "namespace split {\n"
                "template <typename T, int MAXD, int L, int ALGO, bool MC, bool IDXLDS, int NVP, bool DBG = false>\n"
                "__global__ void __launch_bounds__(256, (bp_min_waves<T, MAXD, L, NVP>())) bp_fused_kernel(const BpTables t, const DecodeArgs a) {\n"
                "    bp_fused_body<T, MAXD, L, ALGO, MC, IDXLDS, NVP, DBG, true, Pass, true>(t, a);\n}\n}  // namespace split (the one-series phi; ACG_BP_NO_PHISPLIT=1: the kernel above)\n";
        text += host("sig_c_pass", s.c_pass) + host("sig_v_pass", s.v_pass) + host("sig_c_cnt_ge", s.c_cnt_ge) + host("sig_v_cnt_ge", s.v_cnt_ge);
        text += "}  // namespace " + ns + "\n";
        const std::string k = "(const void *) " + ns + "::bp_fused_kernel<float, 8, " + std::to_string(L) + ", 0, ";
        const std::string ks = "(const void *) " + ns + "::split::bp_fused_kernel<float, 8, " + std::to_string(L) + ", 0, ";
        entries += " \\\n    {{\"" + name + "\", " + std::to_string(L) + ", " + std::to_string(s.n_cpass) + ", " + std::to_string(s.n_apass) + ", " +
                   std::to_string(s.n_vpass) + ", " + ns + "::sig_c_pass, " + ns + "::sig_v_pass, " + ns + "::sig_c_cnt_ge, " + ns + "::sig_v_cnt_ge, \"" + rows_str + "\", \"" + split_str + "\"}, {" + k +
                   "false, true, BP_NVP>, " + k + "true, true, BP_NVP>, " + ks + "false, true, BP_NVP>}},";
    }
    text += "\n#define ACG_BP_SPEC_ENTRIES" + entries + "\n";
    if (out_path) {
        FILE *f = fopen(out_path, "w");
        if (!f || fwrite(text.data(), 1, text.size(), f) != text.size() || fclose(f) != 0) {
            fprintf(stderr, "bp_spec_gen: cannot write %s\n", out_path);
            return 1;
        }
    }
    return 0;
}
