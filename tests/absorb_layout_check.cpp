// Host-only check of the absorbed degree-1 variables of acg::bp_layout_build (csrc/code.cpp, BpLayout::n_apass):
//   absorb_layout_check <matrix.txt> <L>
// builds the layout with and without absorption, checks that the absorbed variables and the variable passes partition
// the code, that every absorbed variable is the last edge of the check in its lane and has degree 1, that every other
// edge keeps its position j inside its check, and prints "<absorbed variables> <variable passes> <variable passes without>".
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../acg_alp_ldpc_amd/csrc/ldpc_internal.hpp"

namespace acg {
void set_error(const std::string &) {}  // code.cpp reports through the library's error slot (api.hip)
}

#define FAIL(...) return printf(__VA_ARGS__), printf("\n"), 1

int main(int argc, char **argv) {
    if (argc < 3) FAIL("usage: absorb_layout_check <matrix.txt> <L>");
    std::vector<uint8_t> Hd;
    int m = 0, n = 0;
    if (!acg::code_read_txt(argv[1], Hd, m, n)) FAIL("CANNOT READ");
    acg::Code c;
    if (!acg::code_build(c, Hd.data(), m, n)) FAIL("CANNOT BUILD");
    const int L = atoi(argv[2]);
    acg::BpLayout o, a;
    if (!acg::bp_layout_build(c, L, o) || !acg::bp_layout_build(c, L, a, acg::BP_MAX_APASS)) FAIL("LAYOUT FAILED");
    if (o.n_apass != 0 || o.n_absorbed != 0) FAIL("ABSORPTION WITHOUT BEING ASKED");
    if (a.n_apass > acg::BP_MAX_APASS || a.n_cpass != o.n_cpass) FAIL("BAD PASS COUNTS");
    auto cdeg = [&](int i) { return c.row_ptr[i + 1] - c.row_ptr[i]; };
    auto vdeg = [&](int j) { return c.col_ptr[j + 1] - c.col_ptr[j]; };
    // every variable exactly once: in a variable pass or absorbed
    std::vector<int> seen(n, 0);
    for (int s = 0; s < a.n_vpass * L; s++)
        if (a.v_var[s] >= 0) seen[a.v_var[s]]++;
    int absorbed = 0;
    const int p0 = a.n_cpass - a.n_apass;
    for (int s = 0; s < a.n_apass * L; s++) {
        const int v = a.a_var[s];
        const int chk = (p0 * L + s < m) ? a.c_chk[(size_t) p0 * L + s] : -1;
        if ((v >= 0) != (chk >= 0)) FAIL("ABSORBED PASS SLOT %d: variable %d, check %d", s, v, chk);
        if (v < 0) continue;
        seen[v]++;
        absorbed++;
        if (vdeg(v) != 1) FAIL("ABSORBED VARIABLE %d HAS DEGREE %d", v, vdeg(v));
        if (c.edge_var[c.row_ptr[chk + 1] - 1] != v) FAIL("ABSORBED VARIABLE %d IS NOT THE LAST EDGE OF CHECK %d", v, chk);
    }
    for (int v = 0; v < n; v++)
        if (seen[v] != 1) FAIL("VARIABLE %d SEEN %d TIMES", v, seen[v]);
    if (absorbed != a.n_absorbed || a.n_vpass != (n - absorbed + L - 1) / L) FAIL("COUNTS");
    // checks: same degree sequence per slot (pass degrees unchanged), degrees descending
    for (int s = 0; s < o.n_cpass * L; s++) {
        const int d0 = o.c_chk[s] >= 0 ? cdeg(o.c_chk[s]) : -1, d1 = a.c_chk[s] >= 0 ? cdeg(a.c_chk[s]) : -1;
        if (d0 != d1) FAIL("CHECK SLOT %d: DEGREE %d -> %d", s, d0, d1);
    }
    for (int p = 0; p < a.n_cpass; p++)
        if (a.c_maxdeg[p] != o.c_maxdeg[p]) FAIL("PASS %d DEGREE", p);
    // edge positions: the variable sweep's index table names, for edge k of every remaining variable, the word of edge j
    // of its check, where j is the edge's rank in the check (variables ascending), exactly as without absorption
    std::vector<int> word_owner((size_t) a.a_words, -1);
    for (int s = 0; s < a.n_cpass * L; s++) {
        const int chk = a.c_chk[s];
        if (chk < 0) continue;
        const int p = s / L, l = s % L;
        const int real = cdeg(chk) - (p >= p0 ? 1 : 0);
        for (int j = 0; j < real; j++) word_owner[(size_t) a.c_off[p] + (size_t) j * L + l] = c.row_ptr[chk] + j;
        if (p >= p0 && a.c_off[p] + (a.c_maxdeg[p] - 1) * L > a.zero_pos) FAIL("PASS %d OVERRUNS", p);
    }
    for (int s = 0; s < a.n_vpass * L; s++) {
        const int v = a.v_var[s];
        if (v < 0) continue;
        const int p = s / L, l = s % L;
        for (int k = 0; k < vdeg(v); k++) {
            const int e = c.col_edge[c.col_ptr[v] + k];
            const int w = a.v_apos[(size_t) a.v_idx_off[p] + (size_t) k * L + l];
            if (w < 0 || w >= a.a_words || word_owner[w] != e) FAIL("VARIABLE %d EDGE %d: WORD %d", v, k, w);
        }
    }
    // v_cnt_ge: slot < v_cnt_ge[d] <=> variable in the slot has degree >= d
    for (int s = 0; s < a.n_vpass * L; s++) {
        const int d = a.v_var[s] >= 0 ? vdeg(a.v_var[s]) : 0;
        for (int dd = 1; dd <= c.max_vdeg; dd++)
            if ((s < a.v_cnt_ge[dd]) != (d >= dd)) FAIL("V_CNT_GE SLOT %d DEGREE %d", s, dd);
    }
    if (o.zero_pos - a.zero_pos != L * a.n_apass) FAIL("MESSAGE ARRAY %d -> %d", o.zero_pos, a.zero_pos);
    printf("%d %d %d\n", a.n_absorbed, a.n_vpass, o.n_vpass);
    return 0;
}
