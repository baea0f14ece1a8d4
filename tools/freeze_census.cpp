// Developer tool: census of the freeze path of the fixed-work fused sum-product kernels (bp_fused_body FREEZE).
//   g++ -O2 -std=c++17 -Iinclude tools/freeze_census.cpp acg_alp_ldpc_amd/csrc/code.cpp -o /tmp/freeze_census
//   /tmp/freeze_census data/H05.txt [frames=300] [sweeps=50] [L=32] [first=6] [period=2] [snr ... | constsum]   (default SNRs: -3 -2 +2)
// The run of tools/phi_census.cpp: a float flooding run in the library's wave-group layout (bp_layout_build with absorption),
// all-zero codeword, AWGN from std::mt19937 per frame, the SAT instances' arithmetic with phi from the host's log2f / exp2f
// (a few results differ in the last bit from the device).  The state of a frame after a sweep is what the kernel compares:
// every word of the message array A and the absorbed variables' words aw.  Per SNR it reports
//   latch:   the sweep whose estimate first has a zero syndrome (the kernel's out_now)
//   repeat:  the first sweep whose state equals the previous sweep's, bit for bit (latched frames only)
//   cadence: with the first snapshot `first` sweeps behind the latch and a compare + new snapshot every `period` sweeps (the
//            kernel's schedule: no detection behind the last sweep), the sweeps a frame executes and the detections it pays
//   gate:    the kernel's detection in full, for the cadence given and for every cadence of the grid the built-in one was chosen
//            from.  A lane sums the words it would compare (the quads l, l + L, ... of A and its own aw); the first detection
//            behind a latch only writes; a later one is "rejected" when a lane's sum differs from the one taken at the snapshot
//            (the group only writes) and "passed" otherwise (the group loads and compares).  A passed detection whose compare
//            fails is a collision of the sum.  With the word `constsum` among the SNRs every lane's sum is a constant, so every
//            detection passes: the sweep at which a frame stops must not depend on it (the compare alone decides).
//            Rows: "gate <snr> <first>,<period> <sweeps run> <frozen frames> <first> <rejected> <passed> <collisions>" (totals
//            over the frames, sweeps run as a mean).
// and the property the kernel's freeze stands on in this model: a frame stopped at its first exact repeat has, after the last
// sweep, the hard decisions it latched ("stopped frames whose final decisions differ from the latch": must be 0).
#include <algorithm>
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

// one cadence of the kernel's detection with the checksum gate in front of the compare
struct Cadence {
    int first, period;
    // per frame
    int due = 0, stop = 0;
    bool have = false;
    std::vector<uint32_t> snap, sum;
    // totals
    long run = 0, frozen = 0, n_first = 0, n_rejected = 0, n_passed = 0, n_collisions = 0;
};
static const int GRID[][2] = {{1, 1}, {1, 2}, {2, 1}, {2, 2}, {3, 1}, {4, 1}, {4, 2}, {5, 3}, {6, 1}, {6, 2}, {7, 2}, {8, 1}, {8, 2},
                              {8, 3}, {8, 4}, {9, 2}, {10, 1}, {10, 2}, {12, 4}};

// Dom<float>::phi (bp_core.inc) with the host's log2 / exp2, and the fast path's constants (BpPass::phi_c / phi_v)
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

int main(int argc, char **argv) {
    if (argc < 2) return fprintf(stderr, "usage: freeze_census <matrix.txt> [frames] [sweeps] [L] [first] [period] [snr ...]\n"), 1;
    const int frames = argc > 2 ? atoi(argv[2]) : 300, sweeps = argc > 3 ? atoi(argv[3]) : 50, L = argc > 4 ? atoi(argv[4]) : 32;
    const int first = argc > 5 ? atoi(argv[5]) : 6, period = argc > 6 ? atoi(argv[6]) : 2;
    std::vector<double> snrs;
    bool constsum = false;
    for (int i = 7; i < argc; i++) {
        if (!strcmp(argv[i], "constsum")) constsum = true;
        else snrs.push_back(atof(argv[i]));
    }
    if (snrs.empty()) snrs = {-3.0, -2.0, 2.0};
    if (frames < 1 || sweeps < 1 || first < 1 || period < 1) return fprintf(stderr, "frames, sweeps, first, period must be >= 1\n"), 1;
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
    printf("%s: m=%d n=%d L=%d, %d check passes (%d absorbed), %d variable passes; %d frames x %d sweeps; state = %d words; "
           "cadence first=%d period=%d\n\n",
           argv[1], m, n, L, lay.n_cpass, lay.n_apass, lay.n_vpass, frames, sweeps, lay.a_words + lay.n_apass * L, first, period);
    printf("| SNR | FER | latched | latch sweep (mean) | latched frames with an exact repeat | lag latch -> repeat (mean / p90 / max) | "
           "sweeps run, stop at first repeat | sweeps run, cadence | frozen, cadence | detections per frame, cadence |\n");
    printf("|---|---|---|---|---|---|---|---|---|---|\n");
    long differ_total = 0;
    std::string gate_rows;
    for (double snr : snrs) {
        std::vector<Cadence> cads(1);
        cads[0].first = first, cads[0].period = period;
        for (const auto &gp : GRID)
            if (gp[0] != first || gp[1] != period) {
                cads.emplace_back();
                cads.back().first = gp[0], cads.back().period = gp[1];
            }
        const double var = std::pow(10, -(snr / 10)) / 2, inv_var2 = 2.0 / var, sigma = std::sqrt(var);
        long fails = 0, latched_n = 0, repeat_n = 0, frozen_n = 0, detections = 0, differ = 0;
        double latch_sum = 0, run_first = 0, run_cad = 0;
        std::vector<int> lags;
        std::vector<uint32_t> A(lay.a_words), prev, snap;
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
            int latch = 0, repeat = 0, stop_cad = 0, due = 0, ndet = 0;  // sweep numbers, 1-based; 0 = never
            for (auto &cd : cads) cd.due = cd.stop = 0, cd.have = false;
            bool have_snap = false;
            std::vector<uint8_t> est(n, 0), est_latch;
            prev.clear();
            for (int it = 1; it <= sweeps; it++) {
                // ---- check sweep (BpPass::check_sat / check_abs)
                for (int p = 0; p < lay.n_cpass; p++) {
                    const int D = lay.c_maxdeg[p];
                    const bool absd = p >= nc;
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
                        for (int j = 0; j < D; j++) {
                            const bool store = absd ? (j == D - 1 ? dg >= 1 : dg >= j + 2) : dg > j;
                            if (!store) continue;
                            const float o = bits(es[j]) == 0 ? INFINITY : phi(es[j]);
                            if (absd && j == D - 1) {
                                const float R = flt((bits(o) & ~SIGN) | ((S ^ x[j]) & SIGN));
                                uint32_t &w = aw[sl - (size_t) nc * L];
                                w = (w & ~ONE) | ((al[sl - (size_t) nc * L] + R <= 0.0f) ? ONE : 0u);
                            } else {
                                A[lay.c_off[p] + j * L + l] = (bits(o) & ~SIGN) | ((S ^ x[j]) & SIGN);
                            }
                        }
                    }
                }
                // ---- variable sweep (BpPass::var_at)
                for (int p = 0; p < lay.n_vpass; p++) {
                    const int D = lay.v_maxdeg[p];
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
                            const float ax = fabsf(xs[k]);
                            A[pos[k]] = (bits(phi(ax)) & ~SIGN & ~ONE) | (xs[k] <= 0 ? (hard | SIGN) : hard);
                        }
                    }
                }
                // ---- the estimate of this sweep and its syndrome
                for (size_t s = 0; s < vhard.size(); s++)
                    if (lay.v_var[s] >= 0) est[lay.v_var[s]] = (uint8_t) vhard[s];
                for (size_t s = 0; s < aw.size(); s++)
                    if (lay.a_var[s] >= 0) est[lay.a_var[s]] = (uint8_t) (aw[s] & ONE);
                if (!latch) {
                    bool bad = false;
                    for (int i = 0; i < m && !bad; i++) {
                        int x = 0;
                        for (int e = c.row_ptr[i]; e < c.row_ptr[i + 1]; e++) x ^= est[c.edge_var[e]];
                        bad = x != 0;
                    }
                    if (!bad) {
                        latch = it;
                        est_latch = est;
                        due = it + first;
                        for (auto &cd : cads) cd.due = it + cd.first;
                    }
                }
                // ---- the state the kernel compares
                std::vector<uint32_t> cur(A);
                cur.insert(cur.end(), aw.begin(), aw.end());
                if (latch && it > latch && !repeat && cur == prev) repeat = it;
                if (latch && it == due && it < sweeps && !stop_cad) {  // the kernel's detection (none behind the last sweep)
                    ndet++;
                    if (have_snap && cur == snap) stop_cad = it;
                    snap = cur;
                    have_snap = true;
                    due = it + period;
                }
                // ---- the same detection as the kernel runs it: the lanes' sums first, the compare only where they allow it
                std::vector<uint32_t> sum;
                for (auto &cd : cads) {
                    if (!latch || it != cd.due || it >= sweeps || cd.stop) continue;
                    if (sum.empty()) {
                        sum.assign(L, constsum ? 0x5EEDu : 0u);
                        if (!constsum) {
                            for (int q = 0; q < lay.a_words / 4; q++)
                                for (int e = 0; e < 4; e++) sum[q % L] += A[4 * q + e];
                            for (size_t x = 0; x < aw.size(); x++) sum[x % L] += aw[x];
                        }
                    }
                    if (!cd.have) cd.n_first++;
                    else if (sum != cd.sum) cd.n_rejected++;
                    else {
                        cd.n_passed++;
                        if (cur == cd.snap) cd.stop = it;
                        else cd.n_collisions++;
                    }
                    cd.snap = cur;
                    cd.sum = sum;
                    cd.have = true;
                    cd.due = it + cd.period;
                }
                prev.swap(cur);
            }
            for (auto &cd : cads) {
                cd.run += cd.stop ? cd.stop : sweeps;
                cd.frozen += cd.stop != 0;
            }
            if (cads[0].stop != stop_cad) return fprintf(stderr, "frame %d: the gated detection stops at %d, the plain one at %d\n", f, cads[0].stop, stop_cad), 2;
            fails += !latch;
            if (latch) {
                latched_n++;
                latch_sum += latch;
                if (repeat) {
                    repeat_n++;
                    lags.push_back(repeat - latch);
                    differ += est != est_latch;
                }
            }
            run_first += repeat ? repeat : sweeps;
            run_cad += stop_cad ? stop_cad : sweeps;
            frozen_n += stop_cad != 0;
            detections += ndet;
        }
        std::sort(lags.begin(), lags.end());
        double lag_mean = 0;
        for (int x : lags) lag_mean += x;
        printf("| %+.0f dB | %.3f | %ld | %.1f | %.1f %% | %.1f / %d / %d | %.2f of %d | %.2f of %d | %.1f %% | %.2f |\n", snr,
               (double) fails / frames, latched_n, latched_n ? latch_sum / latched_n : 0.0, latched_n ? 100.0 * repeat_n / latched_n : 0.0,
               lags.empty() ? 0.0 : lag_mean / lags.size(), lags.empty() ? 0 : lags[(lags.size() * 9) / 10 < lags.size() ? (lags.size() * 9) / 10 : lags.size() - 1],
               lags.empty() ? 0 : lags.back(), run_first / frames, sweeps, run_cad / frames, sweeps, 100.0 * frozen_n / frames,
               (double) detections / frames);
        fflush(stdout);
        differ_total += differ;
        for (const auto &cd : cads) {
            char row[200];
            snprintf(row, sizeof row, "gate %+.0f %d,%d %.3f %ld %ld %ld %ld %ld\n", snr, cd.first, cd.period, (double) cd.run / frames, cd.frozen,
                     cd.n_first, cd.n_rejected, cd.n_passed, cd.n_collisions);
            gate_rows += row;
        }
    }
    printf("\nstopped frames whose final decisions differ from the latch: %ld\n", differ_total);
    printf("\ngate (%s), %d frames: snr first,period sweeps-run frozen first rejected passed collisions\n%s", constsum ? "constant sum" : "sum of the lane's words",
           frames, gate_rows.c_str());
    return 0;
}
