// N3 — check-matrix local search: the reference's optimize_H.cpp (quasi-cyclic protograph of Z x Z circulants, one
// random block mutated per proposal, accepted when the QP-ADMM FER at -3 dB over 1000 frames drops) on the device.
//   acg_optimize_h [--init data/H05.txt | --random 8,14] [--Z 20] [--iters 10000] [--tests 1000] [--snr -3]
//                  [--alpha 1.95 --mu 0.5 --admm-iters 1000] [--seed 239] [--out optimalH.txt] [--noise host|device]
//                  [--batch K]                           score K proposals per call (acg_ldpc_mc_run_codes), drawn from the
//                                                        current matrix as if each were rejected; the first one that improves
//                                                        is accepted, the generator rewinds to the state behind its draw and the
//                                                        proposals behind it are discarded: stdout, the saved matrix and the
//                                                        proposal sequence are those of --batch 1 (the default) for any K
//                  [--dump-proposals N [--accept-all]]   host only: print "row col present shift" of the first N proposals
//                                                        (every one rejected, or every one accepted) and stop — pinned against
//                                                        the reference's own random_permute in tests/test_drivers.py
//                  [--dump-proposals N --batch K --accept-every J]   the same through the batched generator, every J-th
//                                                        proposal "accepted" (0 = none)
// Every proposal is a fresh H: graph analysis, generator (GetOrtogonal) and decoder are rebuilt per proposal through
// the C ABI; a proposal whose generator does not exist scores FER = 1 (optimize_H.cpp:17-19).
#include <algorithm>
#include <chrono>
#include <iostream>
#include <random>

#include "common.hpp"

struct QcMatrix {  // quasi-cyclic description: block mask + one shift per present block
    int Z = 0, R = 0, C = 0;
    std::vector<uint8_t> present;  // R*C
    std::vector<int> shift;        // R*C

    std::vector<uint8_t> dense() const {  // row i*Z+k has its one at column j*Z + (shift + k) mod Z
        std::vector<uint8_t> H((size_t) R * Z * C * Z, 0);
        for (int i = 0; i < R; i++)
            for (int j = 0; j < C; j++)
                if (present[(size_t) i * C + j])
                    for (int k = 0; k < Z; k++)
                        H[(size_t) (i * Z + k) * (C * Z) + (size_t) j * Z + (shift[(size_t) i * C + j] + k) % Z] = 1;
        return H;
    }

    // inverse of dense(): fails (false) if some block is not a single circulant
    bool from_dense(const std::vector<uint8_t> &H, int m, int n, int z) {
        if (m % z || n % z) return false;
        Z = z;
        R = m / z;
        C = n / z;
        present.assign((size_t) R * C, 0);
        shift.assign((size_t) R * C, 0);
        for (int i = 0; i < R; i++)
            for (int j = 0; j < C; j++) {
                int s = -1;
                for (int k = 0; k < Z; k++)
                    for (int l = 0; l < Z; l++)
                        if (H[(size_t) (i * Z + k) * n + (size_t) j * Z + l]) {
                            const int ns = (l - k + Z) % Z;
                            if (s >= 0 && s != ns) return false;
                            s = ns;
                        }
                if (s >= 0) {
                    present[(size_t) i * C + j] = 1;
                    shift[(size_t) i * C + j] = s;
                }
            }
        return dense() == H;
    }

    // one mutation (optimize_H.cpp:66-75): pick a block; flip its presence if it is absent or with probability 1/2;
    // redraw its shift.  at_out (optional): the block that was drawn
    template <typename Gen>
    QcMatrix mutated(Gen &rnd, size_t *at_out = nullptr) const {
        QcMatrix q = *this;
        const int i = (int) (rnd() % (unsigned) R);
        const int j = (int) (rnd() % (unsigned) C);
        const size_t at = (size_t) i * C + j;
        if (!q.present[at] || rnd() % 2 == 0) q.present[at] = !q.present[at];
        q.shift[at] = (int) (rnd() % (unsigned) Z);
        if (at_out) *at_out = at;
        return q;
    }
};

struct Scorer {
    double alpha, mu, snr;
    int iters;
    int64_t tests;
    int noise;
    mutable double host_s = 0, device_s = 0;  // code, generator, codewords; decoder handle + Monte-Carlo run
    // FER(H) of optimize_H.cpp:16-25: codewords from GetOrtogonal + mt19937(239)
    double fer(const QcMatrix &q, int64_t ntests) const {
        const auto t0 = std::chrono::steady_clock::now();
        const int m = q.R * q.Z, n = q.C * q.Z;
        std::vector<uint8_t> H = q.dense();
        acg_ldpc_code *code = nullptr;
        if (acg_ldpc_code_from_dense(H.data(), m, n, &code)) drv::die("code_from_dense");
        bool ok;
        std::vector<uint8_t> cws = drv::make_codewords(code, nullptr, 239u, ntests, &ok);
        double f = 1.0;
        const auto t1 = std::chrono::steady_clock::now();
        host_s += std::chrono::duration<double>(t1 - t0).count();
        if (ok) {
            int nv, nc, nz;
            double e_min, e_max;
            acg_ldpc_code_admm_shape(code, &nv, &nc, &nz, &e_min, &e_max);
            if (!(e_min * mu <= alpha)) {
                acg_ldpc_params p;
                acg_ldpc_params_default(&p);
                p.algo = ACG_LDPC_QPADMM;
                p.alpha = alpha;
                p.mu = mu;
                p.max_iter = iters;
                p.eps_stop = 1e-5;
                p.fast_setup = 1;  // one decoder per proposal: skip the static LDS placement search
                acg_ldpc_decoder *d = nullptr;
                if (acg_ldpc_decoder_create(code, &p, &d)) drv::die("create");
                f = drv::run_mc(d, cws, n, snr, ntests, noise, 1).fer();
                acg_ldpc_decoder_destroy(d);
            }
        }
        device_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
        acg_ldpc_code_destroy(code);
        return f;
    }
};

// A proposal drawn ahead of its predecessors' scores: the candidate, the block that was drawn, and the generator as it stood
// behind the draw (where the search continues when this proposal is the one accepted)
struct Proposal {
    QcMatrix q;
    size_t at = 0;
    std::mt19937 rnd_after;
};

// K proposals in order, each drawn from q — what the sequential loop draws as long as every one of them is rejected
static std::vector<Proposal> draw_batch(const QcMatrix &q, std::mt19937 &rnd, int K) {
    std::vector<Proposal> out((size_t) K);
    for (Proposal &pr : out) {
        pr.q = q.mutated(rnd, &pr.at);
        pr.rnd_after = rnd;
    }
    return out;
}

static double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// FER of every proposal of a batch in one acg_ldpc_mc_run_codes call.  As Scorer::fer: a proposal without a generator, or
// whose QP-ADMM guard fires, scores 1 and is not submitted.
struct BatchScorer {
    const Scorer &sc;
    acg_ldpc_evaluator *ev = nullptr;
    double host_s = 0, device_s = 0;  // building codes, generators and codewords; inside acg_ldpc_mc_run_codes

    explicit BatchScorer(const Scorer &s) : sc(s) {
        acg_ldpc_params p;
        acg_ldpc_params_default(&p);
        p.algo = ACG_LDPC_QPADMM;
        p.alpha = sc.alpha;
        p.mu = sc.mu;
        p.max_iter = sc.iters;
        p.eps_stop = 1e-5;
        if (acg_ldpc_evaluator_create(&p, &ev)) drv::die("evaluator_create");
    }
    ~BatchScorer() { acg_ldpc_evaluator_destroy(ev); }

    std::vector<double> fer(const std::vector<Proposal> &props, int64_t ntests) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<double> f(props.size(), 1.0);
        std::vector<acg_ldpc_code *> codes;
        std::vector<std::vector<uint8_t>> cws;
        std::vector<size_t> who;
        for (size_t j = 0; j < props.size(); j++) {
            const QcMatrix &q = props[j].q;
            const int m = q.R * q.Z, n = q.C * q.Z;
            std::vector<uint8_t> H = q.dense();
            acg_ldpc_code *code = nullptr;
            if (acg_ldpc_code_from_dense(H.data(), m, n, &code)) drv::die("code_from_dense");
            bool ok;
            std::vector<uint8_t> cw = drv::make_codewords(code, nullptr, 239u, ntests, &ok);
            int nv, nc, nz;
            double e_min, e_max;
            acg_ldpc_code_admm_shape(code, &nv, &nc, &nz, &e_min, &e_max);
            if (!ok || e_min * sc.mu <= sc.alpha) {
                acg_ldpc_code_destroy(code);
                continue;
            }
            codes.push_back(code);
            cws.push_back(std::move(cw));
            who.push_back(j);
        }
        host_s += seconds_since(t0);
        if (!codes.empty()) {
            const auto t1 = std::chrono::steady_clock::now();
            const int n = props[0].q.C * props[0].q.Z;
            std::vector<acg_ldpc_mc_cfg> cfgs(codes.size());
            std::vector<acg_ldpc_mc_result> res(codes.size());
            for (size_t k = 0; k < codes.size(); k++) {
                std::memset(&cfgs[k], 0, sizeof cfgs[k]);
                cfgs[k].frames = ntests;
                cfgs[k].snr = sc.snr;
                cfgs[k].seed = 1;
                cfgs[k].noise = sc.noise;
                cfgs[k].codewords = cws[k].data();
                cfgs[k].n_codewords = (int64_t) (cws[k].size() / (size_t) n);
            }
            if (acg_ldpc_mc_run_codes(ev, codes.data(), (int32_t) codes.size(), cfgs.data(), res.data())) drv::die("acg_ldpc_mc_run_codes");
            for (size_t k = 0; k < codes.size(); k++) {
                drv::McOut o;
                o.r = res[k];
                f[who[k]] = o.fer();
                acg_ldpc_code_destroy(codes[k]);
            }
            device_s += seconds_since(t1);
        }
        return f;
    }
};

int main(int argc, char **argv) {
    drv::Args a{argc, argv};
    const int Z = (int) a.integer("--Z", 20);
    Scorer sc{a.num("--alpha", 1.95), a.num("--mu", 0.5), a.num("--snr", -3.0), (int) a.integer("--admm-iters", 1000),
              a.integer("--tests", 1000),
              std::strcmp(a.get("--noise", "host"), "device") ? ACG_LDPC_NOISE_HOST_MT19937 : ACG_LDPC_NOISE_DEVICE_PHILOX};
    const char *out = a.get("--out", "optimalH.txt");
    std::mt19937 rnd((uint32_t) a.integer("--seed", 239));  // optimize_H.cpp:132
    const int K = (int) std::max(1L, a.integer("--batch", 1));
    QcMatrix q;
    if (a.get("--init")) {
        acg_ldpc_code *code = nullptr;
        if (acg_ldpc_code_load_txt(a.get("--init"), &code)) drv::die("read_pcm");
        int m, n, E;
        acg_ldpc_code_dims(code, &m, &n, &E);
        std::vector<uint8_t> H((size_t) m * n);
        acg_ldpc_code_dense(code, H.data());
        acg_ldpc_code_destroy(code);
        if (!q.from_dense(H, m, n, Z)) {
            std::fprintf(stderr, "%s is not quasi-cyclic with %d x %d circulants\n", a.get("--init"), Z, Z);
            return 1;
        }
    } else {
        // random start (optimize_H.cpp:106-122): density-1/2 block mask, uniform shifts, redrawn until a generator exists
        std::vector<double> rc = drv::parse_list(a.get("--random", "8,14"));
        q.Z = Z;
        q.R = (int) rc[0];
        q.C = (int) rc[1];
        for (;;) {
            q.present.assign((size_t) q.R * q.C, 0);
            q.shift.assign((size_t) q.R * q.C, 0);
            for (size_t k = 0; k < q.present.size(); k++) {
                q.present[k] = rnd() % 2;
                q.shift[k] = (int) (rnd() % (unsigned) Z);
            }
            std::vector<uint8_t> H = q.dense();
            acg_ldpc_code *code = nullptr;
            if (acg_ldpc_code_from_dense(H.data(), q.R * Z, q.C * Z, &code)) drv::die("code");
            std::vector<uint8_t> G((size_t) (q.C - q.R) * Z * q.C * Z);
            const int rcg = acg_ldpc_code_generator(code, G.data());
            acg_ldpc_code_destroy(code);
            if (rcg == 0) break;
        }
    }
    if (a.has("--check-qc")) {  // host-only: print the protograph (shift or -1 per block) and stop
        std::printf("Z=%d R=%d C=%d\n", q.Z, q.R, q.C);
        for (int i = 0; i < q.R; i++) {
            for (int j = 0; j < q.C; j++) std::printf("%d%c", q.present[(size_t) i * q.C + j] ? q.shift[(size_t) i * q.C + j] : -1, j + 1 == q.C ? '\n' : ' ');
        }
        return 0;
    }
    if (a.has("--dump-proposals")) {  // host-only: the proposal sequence of optimize_H.cpp:89-104 without scoring
        const int cnt = (int) a.integer("--dump-proposals", 16);
        const long J = a.integer("--accept-every", a.has("--accept-all") ? 1 : 0);  // every J-th proposal is "accepted"
        auto accepted = [J](int it) { return J > 0 && (it + 1) % J == 0; };
        auto print = [&q](const QcMatrix &cand, size_t at) {
            std::printf("%d %d %d %d\n", (int) (at / (size_t) q.C), (int) (at % (size_t) q.C), (int) cand.present[at], cand.shift[at]);
        };
        for (int it = 0; it < cnt && K == 1; it++) {
            size_t at = 0;
            QcMatrix cand = q.mutated(rnd, &at);
            print(cand, at);
            if (accepted(it)) q = cand;
        }
        for (int it = 0; it < cnt && K > 1;) {  // the batched generator of the search loop below
            std::vector<Proposal> props = draw_batch(q, rnd, std::min(K, cnt - it));
            int used = (int) props.size();
            for (int j = 0; j < (int) props.size(); j++) {
                print(props[(size_t) j].q, props[(size_t) j].at);
                if (accepted(it + j)) {
                    q = props[(size_t) j].q;
                    rnd = props[(size_t) j].rnd_after;
                    used = j + 1;
                    break;
                }
            }
            it += used;
        }
        return 0;
    }
    std::cout.precision(5);
    std::cout << std::fixed;
    double error = sc.fer(q, sc.tests);
    std::cout << "initial FER=" << error << std::endl;
    const int iters = (int) a.integer("--iters", 10000);
    const auto t_search = std::chrono::steady_clock::now();
    auto accept = [&](const QcMatrix &cand, double e) {  // optimize_H.cpp:96-101
        q = cand;
        error = e;
        std::cout << "accept, FER=" << error << std::endl;
        std::vector<uint8_t> H = q.dense();
        acg_ldpc_code *code = nullptr;
        if (acg_ldpc_code_from_dense(H.data(), q.R * Z, q.C * Z, &code)) drv::die("code");
        if (acg_ldpc_code_save_txt(code, out)) drv::die("save_matrix");
        acg_ldpc_code_destroy(code);
    };
    long speculated = 0, discarded = 0;
    double host_s = 0, device_s = 0;
    const double host0 = sc.host_s, device0 = sc.device_s;  // (the initial FER is not part of the search)
    for (int it = 0; it < iters && K == 1; it++) {
        QcMatrix cand = q.mutated(rnd);
        const double e = sc.fer(cand, sc.tests);
        std::cout << "\tproposal: FER=" << e << std::endl;
        if (e < error) accept(cand, e);
    }
    if (K == 1) host_s = sc.host_s - host0, device_s = sc.device_s - device0;
    if (K > 1) {
        BatchScorer bs(sc);
        for (int it = 0; it < iters;) {
            std::vector<Proposal> props = draw_batch(q, rnd, std::min(K, iters - it));
            const std::vector<double> e = bs.fer(props, sc.tests);
            int used = (int) props.size();
            for (int j = 0; j < (int) props.size(); j++) {
                std::cout << "\tproposal: FER=" << e[(size_t) j] << std::endl;
                if (e[(size_t) j] < error) {  // the proposals behind it were drawn from a matrix that is no longer current
                    accept(props[(size_t) j].q, e[(size_t) j]);
                    rnd = props[(size_t) j].rnd_after;
                    used = j + 1;
                    break;
                }
            }
            speculated += (long) props.size();
            discarded += (long) props.size() - used;
            it += used;
        }
        host_s = bs.host_s;
        device_s = bs.device_s;
    }
    // (stderr: stdout stays the reference's)
    std::fprintf(stderr, "[acg_optimize_h] batch=%d proposals=%d scored=%ld discarded=%ld search_s=%.3f host_s=%.3f device_s=%.3f\n", K, iters,
                 K > 1 ? speculated : (long) iters, discarded, seconds_since(t_search), host_s, device_s);
    if (a.has("--final-tests")) std::cout << sc.fer(q, a.integer("--final-tests", 10000)) << std::endl;  // optimize_H.cpp:135
    return 0;
}
