// Host check of the signature match that picks a build-time instance of the fused BP kernel (csrc/bp_spec.hpp); built and run
// by tests/test_bp_spec.py, once plainly and once under -fsanitize=address,undefined.
//   bp_spec_check <data/H05.txt>
// The signature is that of H05 at 32 lanes per frame with its degree-1 variables absorbed: the layout the handle set-up builds.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../acg_alp_ldpc_amd/csrc/bp_spec.hpp"

namespace acg {
void set_error(const std::string &msg) { fprintf(stderr, "%s\n", msg.c_str()); }
}
using namespace acg;

static int fails = 0;
static void expect(bool cond, const char *what) {
    if (!cond) {
        fprintf(stderr, "FAILED: %s\n", what);
        fails++;
    }
}

static BpLayout layout(const Code &c, int L, bool absorb) {
    BpLayout lay;
    if (!bp_layout_build(c, L, lay) || (absorb && !bp_layout_absorb(c, L, lay))) {
        fprintf(stderr, "no layout\n");
        exit(2);
    }
    return lay;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::vector<uint8_t> H;
    int m = 0, n = 0;
    Code c;
    if (!code_read_txt(argv[1], H, m, n) || !code_build(c, H.data(), m, n)) return 2;
    const BpLayout lay32 = layout(c, 32, true);
    const BpSpecTables tab = bp_spec_tables(lay32);
    const BpSpecSig sig = tab.sig("H05_L32");
    expect(lay32.n_apass == 2 && lay32.n_cpass == 5 && lay32.n_vpass == 7, "H05 at L = 32: 5 check passes, 2 of them absorbed, 7 variable passes");
    expect((int) tab.c_cnt_ge.size() == BP_SPEC_NCNT && (int) tab.v_cnt_ge.size() == BP_SPEC_NCNT, "histograms padded to BP_SPEC_NCNT");

    expect(bp_spec_matches(sig, layout(c, 32, true)), "accepts H05 at L = 32");
    expect(!bp_spec_matches(sig, layout(c, 64, true)), "rejects H05 at L = 64");
    expect(!bp_spec_matches(sig, layout(c, 32, false)), "rejects H05 built without absorption");
    expect(!bp_spec_matches(sig, layout(c, 16, true)), "rejects H05 at L = 16");

    // every table of the signature with one entry off by one, and every count: the unchanged layout must be rejected
    int variants = 0;
    for (int which = 0; which < 4; which++) {
        const size_t len = which == 0 ? tab.c_pass.size() : which == 1 ? tab.v_pass.size() : (size_t) BP_SPEC_NCNT;
        for (size_t i = 0; i < len; i++) {
            BpSpecTables t2 = tab;
            std::vector<int32_t> &v = which == 0 ? t2.c_pass : which == 1 ? t2.v_pass : which == 2 ? t2.c_cnt_ge : t2.v_cnt_ge;
            v[i] += 1;
            expect(!bp_spec_matches(t2.sig("x"), lay32), "rejects a signature whose tables differ in one entry");
            variants++;
        }
    }
    for (int which = 0; which < 4; which++) {
        BpSpecTables t2 = tab;
        // (a larger count would make the match read past the tables: the counts are compared first, which this holds it to)
        (which == 0 ? t2.L : which == 1 ? t2.n_cpass : which == 2 ? t2.n_apass : t2.n_vpass) -= 1;
        expect(!bp_spec_matches(t2.sig("x"), lay32), "rejects a signature whose count differs");
    }

    // a matrix whose tables differ in one entry: one edge of H05 removed (a check of degree 7 becomes one of degree 6)
    {
        std::vector<uint8_t> H2 = H;
        int row = -1;
        for (int i = 0; i < m && row < 0; i++)
            if (c.row_ptr[i + 1] - c.row_ptr[i] == c.max_cdeg) row = i;
        // take the edge to a variable of degree >= 2, so that no variable is left without a check
        for (int e = c.row_ptr[row]; e < c.row_ptr[row + 1]; e++) {
            const int v = c.edge_var[e];
            if (c.col_ptr[v + 1] - c.col_ptr[v] >= 2) {
                H2[(size_t) row * n + v] = 0;
                break;
            }
        }
        Code c2;
        if (!code_build(c2, H2.data(), m, n)) return 2;
        expect(c2.E == c.E - 1, "the changed matrix has one edge less");
        expect(!bp_spec_matches(sig, layout(c2, 32, true)), "rejects a matrix whose tables differ in one entry");
    }
    // another matrix with the same signature is a match: two columns of H05 of equal degree exchanged
    {
        int a = -1, b = -1;
        for (int v = 0; v + 1 < n && a < 0; v++) {
            bool differ = false;
            for (int i = 0; i < m; i++) differ |= H[(size_t) i * n + v] != H[(size_t) i * n + v + 1];
            if (differ && c.col_ptr[v + 1] - c.col_ptr[v] == c.col_ptr[v + 2] - c.col_ptr[v + 1]) a = v, b = v + 1;
        }
        expect(a >= 0, "H05 has two neighbouring columns of equal degree that differ");
        if (a >= 0) {
            std::vector<uint8_t> H3 = H;
            for (int i = 0; i < m; i++) std::swap(H3[(size_t) i * n + a], H3[(size_t) i * n + b]);
            Code c3;
            if (!code_build(c3, H3.data(), m, n)) return 2;
            const BpLayout l3 = layout(c3, 32, true);
            expect(l3.v_apos != lay32.v_apos || l3.v_var != lay32.v_var, "the exchanged columns change the index tables");
            expect(bp_spec_matches(sig, l3), "accepts another matrix with the same signature");
        }
    }
    if (fails) return 1;
    printf("ok %d one-entry variants\n", variants);
    return 0;
}
