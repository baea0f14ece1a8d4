// Developer tool: census of the phi fast path of the fixed-work fused sum-product sweeps (BpPass::word_c / word_v).
//   g++ -O2 -std=c++17 -Iinclude tools/phi_census.cpp acg_alp_ldpc_amd/csrc/code.cpp -o /tmp/phi_census
//   /tmp/phi_census [--stop] [--rows] data/H05.txt [frames=300] [sweeps=50] [L=32] [snr ...]      (default SNRs: -3 -2 +2)
// The float model, what a unit is and when it counts as skipped: acg_alp_ldpc_amd/csrc/bp_sat_census.hpp, which the generator of
// the static-policy instances (tools/bp_spec_gen.cpp) runs as well.
// Prints the skipped share of each side and of all phi units, and the frame error rate after the last sweep.
//   --stop: a frame ends at its first exact state repeat (what the freeze leaves of a fixed-work run)
//   --rows: also the skipped share (memo included) of every edge row of every pass, and the sweeps run per frame
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
    bool stop = false, rows = false;
    while (argc > 1 && argv[1][0] == '-' && argv[1][1] == '-') {
        if (!strcmp(argv[1], "--stop")) stop = true;
        else if (!strcmp(argv[1], "--rows")) rows = true;
        else return fprintf(stderr, "unknown option %s\n", argv[1]), 1;
        argv++;
        argc--;
    }
    if (argc < 2) return fprintf(stderr, "usage: phi_census [--stop] [--rows] <matrix.txt> [frames] [sweeps] [L] [snr ...]\n"), 1;
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
        const acg::SatCensus cs = acg::bp_sat_census(c, lay, frames, sweeps, snr, stop);
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
