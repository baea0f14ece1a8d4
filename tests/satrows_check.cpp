// Host check of the census that decides which edge rows of a build-time fused BP instance keep their phi fast-path test
// (csrc/bp_sat_census.hpp); built and run by tests/test_satrows.py, once plainly and once under -fsanitize=address,undefined.
//   satrows_check <data/H05.txt>
//       the census of H05 at 32 lanes per frame and -2 dB (300 frames, 50 sweeps, stopped at the first state repeat) and the row
//       masks it gives at a list of thresholds
//   satrows_check probe <matrix.txt> <L> <snr dB> <symbols.f64> <frames> <rows>
//       runs the model on a batch of channel symbols (float64, frames x n, as decode_batch takes them) and reports what the rows
//       that <rows> clears (the registry's string, "c:0,0,0,1f,f/v:3f,...") meet as phi input: per side the number of inputs
//       that are exactly +0, of magnitude >= 66 (finite), +inf and NaN.  One line: "probe c <zero> <sat> <inf> <nan> v <...>".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../acg_alp_ldpc_amd/csrc/bp_sat_census.hpp"

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

// the layout the handle set-up builds (degree-1 variables absorbed)
static BpLayout layout(const Code &c, int L) {
    BpLayout lay;
    if (!bp_layout_build(c, L, lay) || !bp_layout_absorb(c, L, lay)) {
        fprintf(stderr, "no layout\n");
        exit(2);
    }
    return lay;
}

static uint32_t row_bits(int D) { return D >= 32 ? ~0u : ((1u << D) - 1u); }

struct Probe : SatCensusProbe {
    std::vector<uint32_t> keep[2];
    long zero[2] = {0, 0}, sat[2] = {0, 0}, inf[2] = {0, 0}, nan[2] = {0, 0};
    void input(int side, int pass, int row, float x) override {
        if ((keep[side][pass] >> row) & 1u) return;
        if (std::isnan(x)) nan[side]++;
        else if (std::isinf(x)) inf[side]++;
        else if (x >= 66.0f) sat[side]++;
        else if (sat_census::bits(x) == 0u) zero[side]++;
    }
};

static std::vector<uint32_t> masks(const std::string &s) {
    std::vector<uint32_t> v;
    size_t i = 0;
    while (i < s.size()) {
        size_t j = s.find(',', i);
        if (j == std::string::npos) j = s.size();
        v.push_back((uint32_t) strtoul(s.substr(i, j - i).c_str(), nullptr, 16));
        i = j + 1;
    }
    return v;
}

static int probe(int argc, char **argv) {
    if (argc < 8) return 2;
    std::vector<uint8_t> H;
    int m = 0, n = 0;
    Code c;
    if (!code_read_txt(argv[2], H, m, n) || !code_build(c, H.data(), m, n)) return 2;
    const BpLayout lay = layout(c, atoi(argv[3]));
    const double snr = atof(argv[4]), var = std::pow(10, -(snr / 10)) / 2;
    const int frames = atoi(argv[6]);
    std::string rows = argv[7];
    const size_t at = rows.find('@');
    if (at != std::string::npos) rows.resize(at);
    const size_t sl = rows.find("/v:");
    if (rows.compare(0, 2, "c:") != 0 || sl == std::string::npos) return 2;
    Probe pr;
    pr.keep[0] = masks(rows.substr(2, sl - 2));
    pr.keep[1] = masks(rows.substr(sl + 3));
    if ((int) pr.keep[0].size() != lay.n_cpass || (int) pr.keep[1].size() != lay.n_vpass) {
        fprintf(stderr, "the masks are not this layout's\n");
        return 2;
    }
    std::vector<double> y((size_t) frames * n);
    FILE *f = fopen(argv[5], "rb");
    if (!f || fread(y.data(), sizeof(double), y.size(), f) != y.size()) return 2;
    fclose(f);
    SatCensus cs = bp_sat_census_empty(lay);
    std::vector<float> llr(n);
    std::vector<uint8_t> est;
    for (int fr = 0; fr < frames; fr++) {
        for (int v = 0; v < n; v++) llr[v] = (float) (2 * y[(size_t) fr * n + v] / var * 1.44269504088896341);  // as the kernel's fp64-input path
        bp_sat_census_frame(c, lay, llr.data(), 50, false, cs, est, &pr);
    }
    printf("probe c %ld %ld %ld %ld v %ld %ld %ld %ld\n", pr.zero[0], pr.sat[0], pr.inf[0], pr.nan[0], pr.zero[1], pr.sat[1], pr.inf[1], pr.nan[1]);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "probe")) return probe(argc, argv);
    if (argc < 2) return 2;
    std::vector<uint8_t> H;
    int m = 0, n = 0;
    Code c;
    if (!code_read_txt(argv[1], H, m, n) || !code_build(c, H.data(), m, n)) return 2;
    const BpLayout lay = layout(c, 32);
    expect(lay.n_apass == 2 && lay.n_cpass == 5 && lay.n_vpass == 7, "H05 at L = 32: 5 check passes, 2 of them absorbed, 7 variable passes");
    const SatCensus cs = bp_sat_census(c, lay, 300, 50, -2.0, true);
    expect(cs.frames == 300 && cs.sweeps > 300 * 10 && cs.sweeps < 300 * 50, "frames stop at a state repeat: fewer than 50 sweeps per frame, more than 10");
    expect((int) cs.c.size() == 5 && (int) cs.v.size() == 7, "one census row list per pass");
    for (int p = 0; p < lay.n_cpass; p++) expect((int) cs.c[p].size() == lay.c_maxdeg[p], "a row per edge of a check pass");
    for (int p = 0; p < lay.n_vpass; p++) expect((int) cs.v[p].size() == lay.v_maxdeg[p], "a row per edge of a variable pass");
    for (const auto &pass : cs.c)
        for (const SatCensusRow &r : pass) expect(r.units > 0 && r.today <= r.memo && r.memo <= r.memo_all && r.memo_all <= r.units, "check row counts are ordered");
    // the rows that never fire: message rows 0-3 of check pass 2, row 0 of variable pass 6
    for (int j = 0; j < 4; j++) expect(cs.c[2][j].memo == 0, "check pass 2, rows 0-3: no unit is skipped");
    expect(cs.v[6][0].memo == 0, "variable pass 6, row 0: no unit is skipped");
    // the absorbed passes fire in a fifth of their units and more
    for (int p = 3; p < 5; p++)
        for (const SatCensusRow &r : cs.c[p]) expect(bp_sat_share(r) >= 20.0, "absorbed passes: every row is skipped in 20 % of its units or more");

    const double thresholds[] = {0.0, 1e-9, 0.5, 3.0, 10.0, 17.0, 20.0, 25.0, 60.0, 100.0, 101.0};
    for (double t : thresholds) {
        const SatRows r = bp_sat_rows(cs, t);
        expect((int) r.c.size() == 5 && (int) r.v.size() == 7, "a mask per pass");
        if (t <= 0) {
            for (uint32_t w : r.c) expect(w == ~0u, "-t 0: all ones (check side)");
            for (uint32_t w : r.v) expect(w == ~0u, "-t 0: all ones (variable side)");
        } else {
            expect((r.c[2] & 0xFu) == 0, "threshold > 0: rows 0-3 of check pass 2 are cleared");
            expect((r.v[6] & 1u) == 0, "threshold > 0: row 0 of variable pass 6 is cleared");
        }
        if (t <= 20.0) {
            expect((r.c[3] & row_bits(5)) == row_bits(5), "threshold <= 20: absorbed pass 3 keeps every row");
            expect((r.c[4] & row_bits(4)) == row_bits(4), "threshold <= 20: absorbed pass 4 keeps every row");
        }
        if (t > 100.0) {
            for (int p = 0; p < 5; p++) expect((r.c[p] & row_bits(lay.c_maxdeg[p])) == 0, "-t 101: every check row is cleared");
            for (int p = 0; p < 7; p++) expect((r.v[p] & row_bits(lay.v_maxdeg[p])) == 0, "-t 101: every variable row is cleared");
        }
    }
    // without the stop the saturated sweeps come back: every row is skipped at least as often
    const SatCensus full = bp_sat_census(c, lay, 40, 50, -2.0, false);
    expect(full.sweeps == 40 * 50, "without the stop every frame runs every sweep");
    if (fails) return 1;
    printf("ok %ld sweeps in %ld frames, %ld failing\n", cs.sweeps, cs.frames, cs.fails);
    return 0;
}
