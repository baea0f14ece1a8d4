// Developer tool: census of the phi fast path of the fixed-work fused sum-product sweeps (BpPass::word_c / word_v).
//   g++ -O2 -std=c++17 -Iinclude tools/phi_census.cpp acg_alp_ldpc_amd/csrc/code.cpp -o /tmp/phi_census
//   /tmp/phi_census [--stop] [--rows] [--split lo,hi] data/H05.txt [frames=300] [sweeps=50] [L=32] [snr ...]      (default SNRs: -3 -2 +2)
// The float model, what a unit is and when it counts as skipped: acg_alp_ldpc_amd/csrc/bp_sat_census.hpp, which the generator of
// the static-policy instances (tools/bp_spec_gen.cpp) runs as well.
// Prints the skipped share of each side and of all phi units, and the frame error rate after the last sweep.
//   --stop: a frame ends at its first exact state repeat (what the freeze leaves of a fixed-work run)
//   --rows: also the skipped share (memo included) of every edge row of every pass, and the sweeps run per frame
//   --split lo,hi: the census of the one-series phi (SplitCensus; the kernel's thresholds are 1,2): per side, before and behind a
//           frame's latch, the units skipped by today's tests, those whose evaluating lanes all lie at or below lo, all at or
//           above hi, and the mixed ones; with --rows the same per edge row (check side: with the memo hits of the absorbed passes
//           taken out, as the default decoder does).  The table of DESIGN §3 is --stop --split 1,2 on 300 frames at -2 dB.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../acg_alp_ldpc_amd/csrc/bp_sat_census.hpp"

namespace acg {
void set_error(const std::string &msg) { fprintf(stderr, "%s\n", msg.c_str()); }
}

int main(int argc, char **argv) {
    bool stop = false, rows = false, split = false;
    float lo = 1.0f, hi = 2.0f;
    while (argc > 1 && argv[1][0] == '-' && argv[1][1] == '-') {
        if (!strcmp(argv[1], "--stop")) stop = true;
        else if (!strcmp(argv[1], "--rows")) rows = true;
        else if (!strcmp(argv[1], "--split") && argc > 2 && sscanf(argv[2], "%f,%f", &lo, &hi) == 2) {
            split = true;
            argv++;
            argc--;
        }
        else return fprintf(stderr, "unknown option %s\n", argv[1]), 1;
        argv++;
        argc--;
    }
    if (argc < 2) return fprintf(stderr, "usage: phi_census [--stop] [--rows] [--split lo,hi] <matrix.txt> [frames] [sweeps] [L] [snr ...]\n"), 1;
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
    printf("%s: m=%d n=%d L=%d, %d check passes (%d absorbed), %d variable passes; %d frames x %d sweeps\n", argv[1], m, n, L,
           lay.n_cpass, lay.n_apass, lay.n_vpass, frames, sweeps);
    printf("check rows per sweep:");
    for (int p = 0; p < lay.n_cpass; p++) printf(" %d", lay.c_maxdeg[p]);
    printf("   variable rows per sweep:");
    for (int p = 0; p < lay.n_vpass; p++) printf(" %d", lay.v_maxdeg[p]);
    printf("\n\n| SNR | check today | check memo | check memo, all deg-1 rows | variable | all phi units today | with memo | FER |\n");
    printf("|---|---|---|---|---|---|---|---|\n");
    std::string detail;
    for (double snr : snrs) {
        acg::SplitCensus sp = acg::bp_split_census_empty(lay, lo, hi);
        const acg::SatCensus cs = acg::bp_sat_census(c, lay, frames, sweeps, snr, stop, split ? &sp : nullptr);
        acg::SatCensusRow cc, vc;
        auto sum = [](const std::vector<std::vector<acg::SatCensusRow>> &side, acg::SatCensusRow &t) {
            for (const auto &pass : side)
                for (const acg::SatCensusRow &r : pass) t.units += r.units, t.today += r.today, t.memo += r.memo, t.memo_all += r.memo_all;
        };
        sum(cs.c, cc);
        sum(cs.v, vc);
        const double u = (double) (cc.units + vc.units);
        printf("| %+.0f dB | %.1f %% | %.1f %% | %.1f %% | %.1f %% | %.1f %% | %.1f %% | %.1f %% |\n", snr, 100.0 * cc.today / cc.units,
               100.0 * cc.memo / cc.units, 100.0 * cc.memo_all / cc.units, 100.0 * vc.today / vc.units,
               100.0 * (cc.today + vc.today) / u, 100.0 * (cc.memo + vc.today) / u, 100.0 * cs.fails / frames);
        fflush(stdout);
        if (split) {
            char buf[256];
            snprintf(buf, sizeof buf, "\n%+.0f dB, split %g / %g: %.2f sweeps per frame, %.2f of them behind the latch\n"
                     "| sweeps | side | units | skipped | all <= %g | all >= %g | mixed |\n|---|---|---|---|---|---|---|\n", snr, lo, hi,
                     (double) cs.sweeps / frames, (double) sp.sweeps[1] / frames, lo, hi);
            detail += buf;
            auto line = [&](const char *what, const char *side, const acg::SplitCensusRow &r) {
                const double u = r.units ? (double) r.units : 1.0;
                snprintf(buf, sizeof buf, "| %s | %s | %ld | %.1f %% | %.1f %% | %.1f %% | %.1f %% |\n", what, side, r.units, 100.0 * r.skipped / u,
                         100.0 * r.small / u, 100.0 * r.large / u, 100.0 * (r.units - r.skipped - r.small - r.large) / u);
                detail += buf;
            };
            auto memo = [](const acg::SplitCensusRow &r) {
                acg::SplitCensusRow m = r;
                m.skipped = r.skipped_memo, m.small = r.small_memo, m.large = r.large_memo;
                return m;
            };
            for (int b = 0; b < 2; b++)
                for (int side = 0; side < 2; side++) {
                    acg::SplitCensusRow t;
                    for (const auto &pass : side ? sp.v[b] : sp.c[b])
                        for (const acg::SplitCensusRow &r : pass)
                            t.units += r.units, t.skipped += r.skipped, t.small += r.small, t.large += r.large, t.skipped_memo += r.skipped_memo,
                                t.small_memo += r.small_memo, t.large_memo += r.large_memo;
                    line(b ? "behind the latch" : "before the latch, or never latched", side ? "variable" : "check", t);
                    if (!side) line(b ? "behind the latch" : "before the latch, or never latched", "check, memo hits taken out", memo(t));
                }
            if (rows)
                for (int b = 0; b < 2; b++)
                    for (int side = 0; side < 2; side++) {
                        const auto &ps = side ? sp.v[b] : sp.c[b];
                        for (size_t p = 0; p < ps.size(); p++)
                            for (size_t j = 0; j < ps[p].size(); j++)
                                line(b ? "behind" : "before", ((side ? "variable pass " : "check pass ") + std::to_string(p) + " row " + std::to_string(j)).c_str(), side ? ps[p][j] : memo(ps[p][j]));
                    }
        }
        if (rows) {
            char buf[64];
            snprintf(buf, sizeof buf, "\n%+.0f dB: %.2f sweeps per frame\n", snr, (double) cs.sweeps / frames);
            detail += buf;
            for (int side = 0; side < 2; side++) {
                const auto &ps = side ? cs.v : cs.c;
                for (size_t p = 0; p < ps.size(); p++) {
                    detail += (side ? "var pass " : "check pass ") + std::to_string(p) + ":";
                    for (const acg::SatCensusRow &r : ps[p]) {
                        snprintf(buf, sizeof buf, " %.1f", acg::bp_sat_share(r));
                        detail += buf;
                    }
                    detail += "\n";
                }
            }
        }
    }
    fputs(detail.c_str(), stdout);
    return 0;
}
