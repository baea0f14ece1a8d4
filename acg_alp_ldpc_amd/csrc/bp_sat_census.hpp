// Census of the phi fast path of the fixed-work fused sum-product sweeps (BpPass::word_c / word_v in bp_core.inc), row by
// row, and the row masks a static pass policy takes from it.  Host only, no HIP: shared by tools/phi_census.cpp, the generator
// (tools/bp_spec_gen.cpp) and the host tests.  Not part of the ABI.
//
// The model is a float flooding run in the library's wave-group layout (bp_layout_build with absorption), the all-zero codeword,
// AWGN from std::mt19937 seeded per frame.  The sweeps are the SAT instances' arithmetic (same operand order, same word format;
// phi from the host's log2f / exp2f, so a few results differ in the last bit from the device).  A unit is (frame, sweep, pass,
// edge row): the L lanes of a frame, one wave half at L = 32.  A unit is "skipped" when every lane that stores in that row (and
// so would evaluate phi) takes the fast path:
//   check side, today: the exclude-self sum is exactly +0
//   check side, memo:  ... or, in an absorbed pass (BpPass::check_abs) and a row other than the absorbed edge, its bits are
//                      those of the absorbed variable's v->c magnitude (the phi memo)
//   check side, memo+: the same memo for every check with a degree-1 variable, absorbed or not (rows other than that edge)
//   variable side:     |input| >= 66
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>

#include "ldpc_internal.hpp"

namespace acg {

struct SatCensusRow {
    long units = 0, today = 0, memo = 0, memo_all = 0;  // variable side: today == memo == memo_all
};

struct SatCensus {
    std::vector<std::vector<SatCensusRow>> c, v;  // [pass][edge row]; absorbed check passes: row D - 1 is the register edge
    long frames = 0, fails = 0, sweeps = 0;       // fails: frames whose last estimate fails the syndrome; sweeps: run, all frames
};

namespace sat_census {
constexpr uint32_t SIGN = 0x80000000u, ONE = 1u;
inline uint32_t bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}
inline float flt(uint32_t u) {
    float x;
    memcpy(&x, &u, 4);
    return x;
}
// Dom<float>::phi (bp_core.inc) with the host's log2 / exp2
inline float phi(float x) {
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
}  // namespace sat_census

// What a frame of the model meets, for the tests that drive a row through phi's end cases: called for every phi input of a lane
// that stores, with the side (0 check, 1 variable), the pass, the row and the input.
struct SatCensusProbe {
    virtual void input(int side, int pass, int row, float x) = 0;
    virtual ~SatCensusProbe() = default;
};

// Census of the one-series phi (BpPass::word_c / word_v with SPLIT): the units that still evaluate phi, by where their
// evaluating lanes (those that store and do not take a fast path) lie: every one at or below lo (check side: phi_small alone would
// do), every one at or above hi (variable side: phi_large alone), or mixed (NaN counts as mixed).  Kept apart for the sweeps before
// a frame's latch — the first estimate that passes the syndrome — and behind it, where a fixed-work decoder spends most of its
// sweeps.  Counted twice on the check side: with the +0 rule as the only fast path (a decoder under ACG_BP_NO_PHIMEMO=1), and with
// the memo hits of the absorbed passes taken out as well (the default decoder; *_memo).  The variable side has one rule.
struct SplitCensusRow {
    long units = 0, skipped = 0, small = 0, large = 0;  // mixed = units - skipped - small - large
    long skipped_memo = 0, small_memo = 0, large_memo = 0;
};
struct SplitCensus {
    float lo = 1.0f, hi = 2.0f;                             // in the log2(e)-scaled domain
    std::vector<std::vector<SplitCensusRow>> c[2], v[2];   // [0 before the latch or never latched, 1 behind it][pass][edge row]
    long sweeps[2] = {0, 0};                                // sweeps run before / behind the latch, all frames
    int latch = -1;  // of the last frame: the sweeps it had run when its estimate first passed the syndrome; -1: it never did
};

// One frame of the model from channel LLRs in the log2(e)-scaled domain (llr_of_var[n]); counts go to cs.  stop_at_repeat: the
// frame ends at its first exact state repeat (the message words and the absorbed words after a sweep equal those after one of
// the eight sweeps before it: every later state is one already seen), as a latched frame does on the device (the freeze).
// Returns the number of sweeps run; est[n]: the last hard decisions.  split: also the census of the one-series phi and the
// frame's latch sweep (SplitCensus::latch).
inline int bp_sat_census_frame(const Code &c, const BpLayout &lay, const float *llr_of_var, int sweeps, bool stop_at_repeat, SatCensus &cs,
                               std::vector<uint8_t> &est, SatCensusProbe *probe = nullptr, SplitCensus *split = nullptr) {
    using namespace sat_census;
    const int L = lay.L, n = c.n;
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
    std::vector<uint32_t> A(lay.a_words, 0u);
    std::vector<float> llr((size_t) lay.n_vpass * L), al((size_t) lay.n_apass * L);
    std::vector<uint32_t> aw((size_t) lay.n_apass * L), vhard((size_t) lay.n_vpass * L, 0u);
    // var_init + the absorbed words
    for (int p = 0; p < lay.n_vpass; p++)
        for (int l = 0; l < L; l++) {
            const int v = lay.v_var[(size_t) p * L + l];
            const float y = v >= 0 ? llr_of_var[v] : 0.0f;
            llr[(size_t) p * L + l] = y;
            const uint32_t hard = y <= 0 ? ONE : 0;
            vhard[(size_t) p * L + l] = hard;
            const uint32_t ob = (bits(phi(fabsf(y))) & ~SIGN & ~ONE) | (y <= 0 ? (hard | SIGN) : hard);
            for (int k = 0; k < vdeg(v); k++) A[lay.v_apos[(size_t) lay.v_idx_off[p] + (size_t) k * L + l]] = ob;
        }
    for (int s = 0; s < lay.n_apass * L; s++) {
        const int v = lay.a_var[s];
        al[s] = v >= 0 ? llr_of_var[v] : 0.0f;
        aw[s] = v >= 0 ? (bits(phi(fabsf(al[s]))) & ~SIGN & ~ONE) | (al[s] <= 0 ? (ONE | SIGN) : 0u) : 0u;
    }
    constexpr int HIST = 8;
    std::vector<std::vector<uint32_t>> hist;  // the states after the last HIST sweeps (A, then aw)
    int run = 0;
    int behind = 0;  // split: the frame has latched
    if (split) split->latch = -1;
    for (int it = 0; it < sweeps; it++) {
        // ---- check sweep
        for (int p = 0; p < lay.n_cpass; p++) {
            const int D = lay.c_maxdeg[p];
            const bool absd = p >= nc;
            std::vector<char> all_t(D, 1), all_m(D, 1), all_a(D, 1), any(D, 0), all_lo(D, 1), all_hi(D, 1), memo_lo(D, 1), memo_hi(D, 1);
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
                    if (probe) probe->input(0, p, j, es[j]);
                    const uint32_t e = bits(es[j]);
                    const bool t = e == 0;
                    const bool memo_here = r1 >= 0 && j != r1;
                    all_t[j] &= t;
                    all_m[j] &= t || (absd && memo_here && e == mb);
                    all_a[j] &= t || (memo_here && e == mb);
                    if (split && !t) {
                        all_lo[j] &= es[j] <= split->lo;
                        all_hi[j] &= es[j] >= split->hi;
                        if (!(absd && memo_here && e == mb)) {
                            memo_lo[j] &= es[j] <= split->lo;
                            memo_hi[j] &= es[j] >= split->hi;
                        }
                    }
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
                    SatCensusRow &r = cs.c[p][j];
                    r.units++;
                    r.today += all_t[j];
                    r.memo += all_m[j];
                    r.memo_all += all_a[j];
                    if (split) {
                        SplitCensusRow &q = split->c[behind][p][j];
                        q.units++;
                        if (all_t[j]) q.skipped++;
                        else if (all_lo[j]) q.small++;
                        else if (all_hi[j]) q.large++;
                        if (all_m[j]) q.skipped_memo++;
                        else if (memo_lo[j]) q.small_memo++;
                        else if (memo_hi[j]) q.large_memo++;
                    }
                }
        }
        // ---- variable sweep
        for (int p = 0; p < lay.n_vpass; p++) {
            const int D = lay.v_maxdeg[p];
            std::vector<char> all_v(D, 1), any(D, 0), all_lo(D, 1), all_hi(D, 1);
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
                    if (probe) probe->input(1, p, k, ax);
                    all_v[k] &= ax >= 66.0f;
                    if (split && !(ax >= 66.0f)) {
                        all_lo[k] &= ax <= split->lo;
                        all_hi[k] &= ax >= split->hi;
                    }
                    A[pos[k]] = (bits(phi(ax)) & ~SIGN & ~ONE) | (xs[k] <= 0 ? (hard | SIGN) : hard);
                }
            }
            for (int k = 0; k < D; k++)
                if (any[k]) {
                    SatCensusRow &r = cs.v[p][k];
                    r.units++;
                    r.today += all_v[k];
                    r.memo += all_v[k];
                    r.memo_all += all_v[k];
                    if (split) {
                        SplitCensusRow &q = split->v[behind][p][k];
                        q.units++;
                        if (all_v[k]) q.skipped++, q.skipped_memo++;
                        else if (all_lo[k]) q.small++, q.small_memo++;
                        else if (all_hi[k]) q.large++, q.large_memo++;
                    }
                }
        }
        run = it + 1;
        if (split) {
            split->sweeps[behind]++;
            if (!behind) {
                // the estimate of this sweep against the syndrome, as the head of the kernel's next trip takes it
                std::vector<uint8_t> e(n, 0);
                for (size_t s = 0; s < vhard.size(); s++)
                    if (lay.v_var[s] >= 0) e[lay.v_var[s]] = (uint8_t) vhard[s];
                for (size_t s = 0; s < aw.size(); s++)
                    if (lay.a_var[s] >= 0) e[lay.a_var[s]] = (uint8_t) (aw[s] & ONE);
                bool bad = false;
                for (int i = 0; i < c.m && !bad; i++) {
                    int x = 0;
                    for (int k = c.row_ptr[i]; k < c.row_ptr[i + 1]; k++) x ^= e[c.edge_var[k]];
                    bad = x != 0;
                }
                if (!bad) behind = 1, split->latch = run;
            }
        }
        if (stop_at_repeat) {
            std::vector<uint32_t> st(A);
            st.insert(st.end(), aw.begin(), aw.end());
            bool seen = false;
            for (const auto &h : hist) seen |= h == st;
            if (seen) break;
            if ((int) hist.size() == HIST) hist.erase(hist.begin());
            hist.push_back(std::move(st));
        }
    }
    est.assign(n, 0);
    for (size_t s = 0; s < vhard.size(); s++)
        if (lay.v_var[s] >= 0) est[lay.v_var[s]] = (uint8_t) vhard[s];
    for (size_t s = 0; s < aw.size(); s++)
        if (lay.a_var[s] >= 0) est[lay.a_var[s]] = (uint8_t) (aw[s] & ONE);
    return run;
}

inline SatCensus bp_sat_census_empty(const BpLayout &lay) {
    SatCensus cs;
    cs.c.resize(lay.n_cpass);
    cs.v.resize(lay.n_vpass);
    for (int p = 0; p < lay.n_cpass; p++) cs.c[p].resize(lay.c_maxdeg[p]);
    for (int p = 0; p < lay.n_vpass; p++) cs.v[p].resize(lay.v_maxdeg[p]);
    return cs;
}

inline SplitCensus bp_split_census_empty(const BpLayout &lay, float lo, float hi) {
    SplitCensus sp;
    sp.lo = lo;
    sp.hi = hi;
    for (int b = 0; b < 2; b++) {
        sp.c[b].resize(lay.n_cpass);
        sp.v[b].resize(lay.n_vpass);
        for (int p = 0; p < lay.n_cpass; p++) sp.c[b][p].resize(lay.c_maxdeg[p]);
        for (int p = 0; p < lay.n_vpass; p++) sp.v[b][p].resize(lay.v_maxdeg[p]);
    }
    return sp;
}

// `frames` frames of `sweeps` sweeps at most, at `snr` dB: frame f draws its noise from std::mt19937(f + 1)
// split (from bp_split_census_empty): the census of the one-series phi of the same frames
inline SatCensus bp_sat_census(const Code &c, const BpLayout &lay, int frames, int sweeps, double snr, bool stop_at_repeat, SplitCensus *split = nullptr) {
    SatCensus cs = bp_sat_census_empty(lay);
    const double var = std::pow(10, -(snr / 10)) / 2, inv_var2 = 2.0 / var, sigma = std::sqrt(var);
    std::vector<float> ch(c.n);
    std::vector<uint8_t> est;
    for (int f = 0; f < frames; f++) {
        std::mt19937 rng((uint32_t) (f + 1));
        std::normal_distribution<double> nd(0.0, 1.0);
        for (int v = 0; v < c.n; v++) ch[v] = (float) ((1.0 + sigma * nd(rng)) * (inv_var2 * 1.44269504088896341));
        cs.sweeps += bp_sat_census_frame(c, lay, ch.data(), sweeps, stop_at_repeat, cs, est, nullptr, split);
        bool bad = false;
        for (int i = 0; i < c.m && !bad; i++) {
            int x = 0;
            for (int e = c.row_ptr[i]; e < c.row_ptr[i + 1]; e++) x ^= est[c.edge_var[e]];
            bad = x != 0;
        }
        cs.fails += bad;
        cs.frames++;
    }
    return cs;
}

// per cent of a row's units that are skipped with the tests the kernel has (the memo included); a row without units: 0
inline double bp_sat_share(const SatCensusRow &r) { return r.units ? 100.0 * (double) r.memo / (double) r.units : 0.0; }

// The row masks of a static pass policy (c_sat_rows / v_sat_rows): bit j of pass p set = the row keeps its fast-path test.  A
// row is cleared when its skipped share is below threshold_pct; a threshold <= 0 keeps every row, one above 100 clears all.
struct SatRows {
    std::vector<uint32_t> c, v;
};
inline SatRows bp_sat_rows(const SatCensus &cs, double threshold_pct) {
    SatRows m;
    auto side = [&](const std::vector<std::vector<SatCensusRow>> &rows, std::vector<uint32_t> &out) {
        for (const auto &pass : rows) {
            uint32_t bitsv = ~0u;
            for (size_t j = 0; j < pass.size(); j++)
                if (threshold_pct > 0 && bp_sat_share(pass[j]) < threshold_pct) bitsv &= ~(1u << j);
            out.push_back(bitsv);
        }
    };
    side(cs.c, m.c);
    side(cs.v, m.v);
    return m;
}

}  // namespace acg
