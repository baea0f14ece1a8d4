// Host-only dump of the streamed QP-ADMM engine's tables (acg::admm_stream_tables_build, csrc/code.cpp), expanded row by
// row with the same rules the kernel uses (admm_group_rows / admm_row_plus / admm_row_b, csrc/kernels.hpp):
//   admm_stream_tables_check <matrix.txt>
// prints "<n_var> <n_con>", then per variable i one line "A i j0 c0 j1 c1 ..." (its list in sweep order), per row j
// "R j b v0 c0 v1 c1 ..." (the row's terms in the order the row update subtracts them).  tests/test_admm_stream_tables.py
// compares both with a restatement of ConstructADMMProblem (qp_admm.h:13-102).
#include <cstdio>
#include <string>
#include <vector>

#include "../acg_alp_ldpc_amd/csrc/ldpc_internal.hpp"

namespace acg {
void set_error(const std::string &msg) { fprintf(stderr, "%s\n", msg.c_str()); }
}

int main(int argc, char **argv) {
    if (argc < 2) return printf("usage: admm_stream_tables_check <matrix.txt>\n"), 1;
    std::vector<uint8_t> Hd;
    int m = 0, n = 0;
    acg::Code c;
    if (!acg::code_read_txt(argv[1], Hd, m, n) || !acg::code_build(c, Hd.data(), m, n)) return printf("CANNOT READ\n"), 1;
    acg::AdmmStreamTables t;
    if (!acg::admm_stream_tables_build(c, t)) return printf("BUILD FAILED\n"), 1;
    if ((int) t.var_ptr.size() != t.n_var + 1 || (int) t.grp.size() != 4 * t.n_grp) return printf("BAD SIZES\n"), 1;
    printf("%d %d\n", t.n_var, t.n_con);
    for (int i = 0; i < t.n_var; i++) {
        printf("A %d", i);
        for (int k = t.var_ptr[i]; k < t.var_ptr[i + 1]; k++) {
            const uint32_t e = t.var_ent[k];
            const int j0 = (int) (e & 0x0FFFFFFFu), wp = (int) ((e >> 28) & 3u), ty = (int) (e >> 30);
            for (int r = 0; r < acg::admm_group_rows(ty); r++) printf(" %d %d", j0 + r, acg::admm_row_plus(ty, r, wp) ? 1 : -1);
        }
        printf("\n");
    }
    int next_row = 0;
    for (int g = 0; g < t.n_grp; g++) {
        const uint32_t h = t.grp[(size_t) g * 4];
        const int j0 = (int) (h & 0x0FFFFFFFu), ty = (int) (h >> 30);
        if (j0 != next_row) return printf("GROUP %d STARTS AT ROW %d, EXPECTED %d\n", g, j0, next_row), 1;
        next_row += acg::admm_group_rows(ty);
        for (int k = ty; k < 3; k++)
            if (t.grp[(size_t) g * 4 + 1 + k] != 0xFFFFFFFFu) return printf("GROUP %d: MEMBER %d OF A TYPE-%d GROUP\n", g, k, ty), 1;
        for (int r = 0; r < acg::admm_group_rows(ty); r++) {
            printf("R %d %g", j0 + r, acg::admm_row_b(ty, r));
            for (int k = 0; k < ty; k++) {
                const uint32_t mb = t.grp[(size_t) g * 4 + 1 + k];
                printf(" %u %d", mb & 0x3FFFFFFFu, acg::admm_row_plus(ty, r, (int) (mb >> 30)) ? 1 : -1);
            }
            printf("\n");
        }
    }
    if (next_row != t.n_con) return printf("ROWS %d != %d\n", next_row, t.n_con), 1;
    return 0;
}
