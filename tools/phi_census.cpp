// Developer tool: census of the phi fast path of the fixed-work fused sum-product sweeps (BpPass::phi_c / phi_v).
//   g++ -O2 -std=c++17 -Iinclude tools/phi_census.cpp acg_alp_ldpc_amd/csrc/code.cpp -o /tmp/phi_census
//   /tmp/phi_census data/H05.txt [frames=300] [sweeps=50] [L=32] [snr ...]      (default SNRs: -3 -2 +2)
// A float flooding run in the library's wave-group layout (bp_layout_build with absorption), all-zero codeword, AWGN from
// std::mt19937 per frame.  The sweeps are the SAT instances' arithmetic (same operand order, same word format; phi from the
// host's log2f / exp2f, so a few results differ in the last bit from the device).  A unit is (frame, sweep, pass, edge row):
// the L lanes of a frame are one wave half at L = 32.  A unit is "skipped" when every lane that stores in that row (and so
// would evaluate phi) takes the fast path:
//   check side, today: the exclude-self sum is exactly +0
//   check side, memo:  ... or, in an absorbed pass (BpPass::check_abs) and a row other than the absorbed edge, its bits are
//                      those of the absorbed variable's v->c magnitude (the phi memo)
//   check side, memo+: the same memo for every check with a degree-1 variable, absorbed or not (rows other than that edge)
//   variable side:     |input| >= 66
// Prints the skipped share of each side and of all phi units, and the frame error rate after the last sweep.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../acg_alp_ldpc_amd/csrc/ldpc_internal.hpp"

namespace acg {
void set_error(const std::string &msg) { fprintf(stderr, "%s\n", msg.c_str()); }
}

static uint32_t bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}
static float flt(uint32_t u) {
    float x;
    memcpy(&x, &u, 4);
    return x;
}
static const uint32_t SIGN = 0x80000000u, ONE = 1u;

// Dom<float>::phi (bp_core.inc) with the host's log2 / exp2
static float phi(float x) {
    const float w = x * x;
    float g = fmaf(w, -1.7256659564749327e-06f, 5.431033644982242e-05f);
    g = fmaf(g, w, -0.001618721877195048f);
    g = fmaf(g, w, 0.057762255617977924f);
    const float ps = fmaf(w, g, 1.5287663729448977f) - log2f(x);
    const float t = exp2f(-x);
    const float u = t * t;
    float r = fmaf(u, 0.40731721508362195f, 0.40423844622223065f);
    r = fmaf(r, u, 0.5773059513734762f);
    r = fmaf(r, u, 0.961795680143378f);
    const float pl = t * fmaf(u, r, 2.8853900817779268f);
    float o = fmaxf(ps, pl);
    if (std::isnan(ps) || std::isnan(pl)) o = NAN;
    return (x >= 66.0f) ? 0.0f : o;
}

struct Count {
    long units = 0, today = 0, memo = 0, memo_all = 0;
};

int main(int argc, char **argv) {
    if (argc < 2) return fprintf(stderr, "usage: phi_census <matrix.txt> [frames] [sweeps] [L] [snr ...]\n"), 1;
    const int frames = argc > 2 ? atoi(argv[2]) : 300, sweeps = argc > 3 ? atoi(argv[3]) : 50, L = argc > 4 ? atoi(argv[4]) : 32;
    std::vector<double> snrs;
    for (int i = 5; i < argc; i++) snrs.push_back(atof(argv[i]));
    if (snrs.empty()) snrs = {-3.0, -2.0, 2.0};
    std::vector<uint8_t> Hd;
    int m = 0, n = 0;
    acg::Code c;
    acg::BpLayout lay;
    if (!acg::code_read_txt(argv[1], Hd, m, n) || !acg::code_build(c, Hd.data(), m, n) ||
        !acg::bp_layout_build(c, L, lay, acg::BP_MAX_APASS))
        return fprintf(stderr, "cannot build %s\n", argv[1]), 1;
    auto cdeg = [&](int i) { return i < 0 ? 0 : c.row_ptr[i + 1] - c.row_ptr[i]; };
    auto vdeg = [&](int j) { return j < 0 ? 0 : c.col_ptr[j + 1] - c.col_ptr[j]; };
    const int nc = lay.n_cpass - lay.n_apass;
    // row of the degree-1 variable of the check in (pass, lane), -1 none (absorbed passes: their register row)
    std::vector<int> d1row((size_t) lay.n_cpass * L, -1);
    for (int p = 0; p < lay.n_cpass; p++)
        for (int l = 0; l < L; l++) {
            const int chk = lay.c_chk[(size_t) p * L + l];
            if (chk < 0) continue;
            for (int j = 0; j < cdeg(chk); j++)
                if (vdeg(c.edge_var[c.row_ptr[chk] + j]) == 1) d1row[(size_t) p * L + l] = p >= nc ? lay.c_maxdeg[p] - 1 : j;
        }
    printf("%s: m=%d n=%d L=%d, %d check passes (%d absorbed), %d variable passes; %d frames x %d sweeps\n", argv[1], m, n, L,
           lay.n_cpass, lay.n_apass, lay.n_vpass, frames, sweeps);
    printf("check rows per sweep:");
    for (int p = 0; p < lay.n_cpass; p++) printf(" %d", lay.c_maxdeg[p]);
    printf("   variable rows per sweep:");
    for (int p = 0; p < lay.n_vpass; p++) printf(" %d", lay.v_maxdeg[p]);
    printf("\n\n| SNR | check today | check memo | check memo, all deg-1 rows | variable | all phi units today | with memo | FER |\n");
    printf("|---|---|---|---|---|---|---|---|\n");
    for (double snr : snrs) {
        const double var = std::pow(10, -(snr / 10)) / 2, inv_var2 = 2.0 / var, sigma = std::sqrt(var);
        Count cc, vc;
        long fails = 0;
        std::vector<uint32_t> A(lay.a_words);
        std::vector<float> llr((size_t) lay.n_vpass * L), al((size_t) lay.n_apass * L);
        std::vector<uint32_t> aw((size_t) lay.n_apass * L), vhard((size_t) lay.n_vpass * L);
        for (int f = 0; f < frames; f++) {
            std::mt19937 rng((uint32_t) (f + 1));
            std::normal_distribution<double> nd(0.0, 1.0);
            std::vector<float> ch(n);
            for (int v = 0; v < n; v++) ch[v] = (float) ((1.0 + sigma * nd(rng)) * (inv_var2 * 1.44269504088896341));
            std::fill(A.begin(), A.end(), 0u);
            // var_init + the absorbed words
            for (int p = 0; p < lay.n_vpass; p++)
                for (int l = 0; l < L; l++) {
                    const int v = lay.v_var[(size_t) p * L + l];
                    const float y = v >= 0 ? ch[v] : 0.0f;
                    llr[(size_t) p * L + l] = y;
                    const uint32_t hard = y <= 0 ? ONE : 0;
                    const uint32_t ob = (bits(phi(fabsf(y))) & ~SIGN & ~ONE) | (y <= 0 ? (hard | SIGN) : hard);
                    for (int k = 0; k < vdeg(v); k++) A[lay.v_apos[(size_t) lay.v_idx_off[p] + (size_t) k * L + l]] = ob;
                }
            for (int s = 0; s < lay.n_apass * L; s++) {
                const int v = lay.a_var[s];
                al[s] = v >= 0 ? ch[v] : 0.0f;
                aw[s] = v >= 0 ? (bits(phi(fabsf(al[s]))) & ~SIGN & ~ONE) | (al[s] <= 0 ? (ONE | SIGN) : 0u) : 0u;
            }
            for (int it = 0; it < sweeps; it++) {
                // ---- check sweep
                for (int p = 0; p < lay.n_cpass; p++) {
                    const int D = lay.c_maxdeg[p];
                    const bool absd = p >= nc;
                    std::vector<char> all_t(D, 1), all_m(D, 1), all_a(D, 1), any(D, 0);
                    for (int l = 0; l < L; l++) {
                        const size_t sl = (size_t) p * L + l;
                        const int chk = lay.c_chk[sl], dg = cdeg(chk);
                        if (chk < 0) continue;
                        uint32_t x[16];
                        for (int j = 0; j < D; j++) x[j] = (absd && j == D - 1) ? aw[sl - (size_t) nc * L] : A[lay.c_off[p] + j * L + l];
                        uint32_t S = 0;
                        for (int j = 0; j < D; j++) S ^= x[j];
                        float mag[16], pre[16], es[16], s = 0, suf = 0;
                        for (int j = 0; j < D; j++) {
                            mag[j] = flt(x[j] & ~SIGN & ~ONE);
                            pre[j] = s;
                            s += mag[j];
                        }
                        for (int j = D - 1; j >= 0; j--) {
                            es[j] = pre[j] + suf;
                            suf += mag[j];
                        }
                        const int r1 = d1row[sl];
                        const uint32_t mb = r1 >= 0 ? (x[r1] & ~SIGN & ~ONE) : 0u;
                        for (int j = 0; j < D; j++) {
                            const bool store = absd ? (j == D - 1 ? dg >= 1 : dg >= j + 2) : dg > j;
                            if (!store) continue;
                            any[j] = 1;
                            const uint32_t e = bits(es[j]);
                            const bool t = e == 0;
                            const bool memo_here = r1 >= 0 && j != r1;
                            all_t[j] &= t;
                            all_m[j] &= t || (absd && memo_here && e == mb);
                            all_a[j] &= t || (memo_here && e == mb);
                            const float o = t ? INFINITY : phi(es[j]);
                            if (absd && j == D - 1) {
                                const float R = flt((bits(o) & ~SIGN) | ((S ^ x[j]) & SIGN));
                                uint32_t &w = aw[sl - (size_t) nc * L];
                                w = (w & ~ONE) | ((al[sl - (size_t) nc * L] + R <= 0.0f) ? ONE : 0u);
                            } else {
                                A[lay.c_off[p] + j * L + l] = (bits(o) & ~SIGN) | ((S ^ x[j]) & SIGN);
                            }
                        }
                    }
                    for (int j = 0; j < D; j++)
                        if (any[j]) {
                            cc.units++;
                            cc.today += all_t[j];
                            cc.memo += all_m[j];
                            cc.memo_all += all_a[j];
                        }
                }
                // ---- variable sweep
                for (int p = 0; p < lay.n_vpass; p++) {
                    const int D = lay.v_maxdeg[p];
                    std::vector<char> all_v(D, 1), any(D, 0);
                    for (int l = 0; l < L; l++) {
                        const size_t sl = (size_t) p * L + l;
                        const int v = lay.v_var[sl], dg = vdeg(v);
                        if (v < 0) continue;
                        int pos[16];
                        float cv[16], pre[16], s = 0, suf = 0, xs[16];
                        for (int k = 0; k < D; k++) {
                            pos[k] = lay.v_apos[(size_t) lay.v_idx_off[p] + (size_t) k * L + l];
                            cv[k] = flt(A[pos[k]]);
                        }
                        for (int k = 0; k < D; k++) {
                            pre[k] = s;
                            s += cv[k];
                        }
                        const float y = llr[sl];
                        const uint32_t hard = (y + s <= 0.0f) ? ONE : 0u;
                        vhard[sl] = hard;
                        for (int k = D - 1; k >= 0; k--) {
                            xs[k] = y + (pre[k] + suf);
                            suf += cv[k];
                        }
                        for (int k = 0; k < dg; k++) {
                            any[k] = 1;
                            const float ax = fabsf(xs[k]);
                            all_v[k] &= ax >= 66.0f;
                            A[pos[k]] = (bits(phi(ax)) & ~SIGN & ~ONE) | (xs[k] <= 0 ? (hard | SIGN) : hard);
                        }
                    }
                    for (int k = 0; k < D; k++)
                        if (any[k]) {
                            vc.units++;
                            vc.today += all_v[k];
                        }
                }
            }
            // syndrome of the last estimate
            std::vector<uint8_t> est(n, 0);
            for (size_t s = 0; s < vhard.size(); s++)
                if (lay.v_var[s] >= 0) est[lay.v_var[s]] = (uint8_t) vhard[s];
            for (size_t s = 0; s < aw.size(); s++)
                if (lay.a_var[s] >= 0) est[lay.a_var[s]] = (uint8_t) (aw[s] & ONE);
            bool bad = false;
            for (int i = 0; i < m && !bad; i++) {
                int x = 0;
                for (int e = c.row_ptr[i]; e < c.row_ptr[i + 1]; e++) x ^= est[c.edge_var[e]];
                bad = x != 0;
            }
            fails += bad;
        }
        const double u = (double) (cc.units + vc.units);
        printf("| %+.0f dB | %.1f %% | %.1f %% | %.1f %% | %.1f %% | %.1f %% | %.1f %% | %.1f %% |\n", snr, 100.0 * cc.today / cc.units,
               100.0 * cc.memo / cc.units, 100.0 * cc.memo_all / cc.units, 100.0 * vc.today / vc.units,
               100.0 * (cc.today + vc.today) / u, 100.0 * (cc.memo + vc.today) / u, 100.0 * fails / frames);
        fflush(stdout);
    }
    return 0;
}
