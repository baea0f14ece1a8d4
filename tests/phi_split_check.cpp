// Host check of the one-series phi of the fused fixed-work sum-product sweeps (bp_core.inc: Dom<float>::phi_small / phi_large,
// BpPass::word_c / word_v with SPLIT), used by tests/test_phi_split.py.  Stand-alone, no HIP:
//   g++ -O2 -std=c++17 -pthread -Iinclude tests/phi_split_check.cpp acg_alp_ldpc_amd/csrc/code.cpp -o phi_split_check
//   phi_split_check census data/H05.txt     the census of csrc/bp_sat_census.hpp (H05, L = 32, 300 frames of at most 50 sweeps at
//                                           -2 dB, stopped at their first state repeat, thresholds 1 and 2): four lines
//                                           "<0 before | 1 behind the latch> <c|v> units skipped small large mixed" (per cent), then
//                                           "sweeps <per frame> <behind the latch per frame>"
//   phi_split_check series [stride]         the float model of the two series with the results of log2f / exp2f moved by 2 ulps in
//                                           the adverse direction: pl >= ps for every fp32 value in [2, 66), ps >= pl for every one
//                                           in (0, 1], every stride-th bit pattern (default 1: all 1.1e9, about a minute on eight
//                                           threads); prints "ok <patterns> <smallest relative gap large> <small>" or the first failure
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../acg_alp_ldpc_amd/csrc/bp_sat_census.hpp"

namespace acg {
void set_error(const std::string &msg) { fprintf(stderr, "%s\n", msg.c_str()); }
}
using namespace acg;

static float nudge(float v, int ulps) {
    for (int i = 0; i < (ulps < 0 ? -ulps : ulps); i++) v = nextafterf(v, ulps < 0 ? -INFINITY : INFINITY);
    return v;
}
// the two series of Dom<float>::phi with the transcendental's result handed in
static float series_small(float x, float lg) {
    const float w = x * x;
    float g = fmaf(w, -1.7256659564749327e-06f, 5.431033644982242e-05f);
    g = fmaf(g, w, -0.001618721877195048f);
    g = fmaf(g, w, 0.057762255617977924f);
    return fmaf(w, g, 1.5287663729448977f) - lg;
}
static float series_large(float t) {
    const float u = t * t;
    float r = fmaf(u, 0.40731721508362195f, 0.40423844622223065f);
    r = fmaf(r, u, 0.5773059513734762f);
    r = fmaf(r, u, 0.961795680143378f);
    return t * fmaf(u, r, 2.8853900817779268f);
}

static int census(const char *path) {
    std::vector<uint8_t> Hd;
    int m = 0, n = 0;
    Code c;
    BpLayout lay;
    if (!code_read_txt(path, Hd, m, n) || !code_build(c, Hd.data(), m, n) || !bp_layout_build(c, 32, lay, BP_MAX_APASS)) return fprintf(stderr, "cannot build %s\n", path), 1;
    SplitCensus sp = bp_split_census_empty(lay, 1.0f, 2.0f);
    const SatCensus cs = bp_sat_census(c, lay, 300, 50, -2.0, true, &sp);
    for (int b = 0; b < 2; b++)
        for (int side = 0; side < 2; side++) {
            SplitCensusRow t;
            for (const auto &pass : side ? sp.v[b] : sp.c[b])
                for (const SplitCensusRow &r : pass) t.units += r.units, t.skipped += r.skipped, t.small += r.small, t.large += r.large;
            const double u = t.units ? (double) t.units : 1.0;
            printf("%d %c %ld %.2f %.2f %.2f %.2f\n", b, side ? 'v' : 'c', t.units, 100.0 * t.skipped / u, 100.0 * t.small / u, 100.0 * t.large / u,
                   100.0 * (t.units - t.skipped - t.small - t.large) / u);
        }
    printf("sweeps %.2f %.2f\n", (double) cs.sweeps / 300, (double) sp.sweeps[1] / 300);
    // the latch sweep of a frame comes back without a second run of the model, and a caller that does not ask sees what it saw
    SatCensus a = bp_sat_census_empty(lay), b2 = bp_sat_census_empty(lay);
    std::vector<float> ch(c.n, 3.0f);
    std::vector<uint8_t> e1, e2;
    SplitCensus one = bp_split_census_empty(lay, 1.0f, 2.0f);
    const int r1 = bp_sat_census_frame(c, lay, ch.data(), 50, true, a, e1), r2 = bp_sat_census_frame(c, lay, ch.data(), 50, true, b2, e2, nullptr, &one);
    if (r1 != r2 || e1 != e2 || one.latch != 1) return fprintf(stderr, "latch sweep of a clean frame: %d (runs %d / %d)\n", one.latch, r1, r2), 1;
    return 0;
}

static int series(uint32_t stride) {
    struct Range { uint32_t lo, hi; bool large; };  // bit patterns [lo, hi)
    const Range ranges[2] = {{0x40000000u, 0x42840000u, true}, {0x00000001u, 0x3F800001u, false}};
    constexpr int NT = 8;
    std::atomic<uint64_t> count{0}, bad{0};
    std::atomic<uint32_t> first_bad{0xFFFFFFFFu};
    double gap[NT][2];
    std::vector<std::thread> th;
    for (int k = 0; k < NT; k++)
        th.emplace_back([&, k] {
            uint64_t cnt = 0;
            gap[k][0] = gap[k][1] = 1.0;
            for (const Range &r : ranges)
                for (uint64_t b = (uint64_t) r.lo + (uint64_t) k * stride; b < r.hi; b += (uint64_t) NT * stride) {
                    float x;
                    const uint32_t bb = (uint32_t) b;
                    memcpy(&x, &bb, 4);
                    // adverse: the series that has to win gets the smaller value, the other one the larger
                    const float ps = series_small(x, nudge(log2f(x), r.large ? -2 : 2));
                    const float pl = series_large(nudge(exp2f(-x), r.large ? -2 : 2));
                    const bool ok = r.large ? pl >= ps : ps >= pl;
                    if (!ok) {
                        bad++;
                        uint32_t f = first_bad.load();
                        while (bb < f && !first_bad.compare_exchange_weak(f, bb)) {
                        }
                    }
                    const double g = r.large ? ((double) pl - ps) / pl : ((double) ps - pl) / ps;
                    if (g < gap[k][r.large ? 0 : 1]) gap[k][r.large ? 0 : 1] = g;
                    cnt++;
                }
            count += cnt;
        });
    for (auto &t : th) t.join();
    double gl = 1.0, gs = 1.0;
    for (int k = 0; k < NT; k++) gl = gap[k][0] < gl ? gap[k][0] : gl, gs = gap[k][1] < gs ? gap[k][1] : gs;
    if (bad.load()) return printf("FAIL %llu of %llu patterns, first 0x%08x\n", (unsigned long long) bad.load(), (unsigned long long) count.load(), first_bad.load()), 1;
    printf("ok %llu %.3g %.3g\n", (unsigned long long) count.load(), gl, gs);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 3 && !strcmp(argv[1], "census")) return census(argv[2]);
    if (argc >= 2 && !strcmp(argv[1], "series")) return series(argc > 2 ? (uint32_t) strtoul(argv[2], nullptr, 10) : 1u);
    return fprintf(stderr, "usage: phi_split_check census <H05.txt> | series [stride]\n"), 2;
}
