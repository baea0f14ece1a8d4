// Shared helpers of the "next row" drivers: thin C++ callers of the C ABI that replace the
// reference's main.cpp / qpadmm_params.cpp / optimize_H.cpp loops.  No decoding logic lives here.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "acg_ldpc.h"

namespace drv {

inline void die(const char *what) {
    std::fprintf(stderr, "%s: %s\n", what, acg_ldpc_last_error());
    std::exit(1);
}

struct Args {
    int argc;
    char **argv;
    const char *get(const char *key, const char *def = nullptr) const {
        for (int i = 1; i + 1 < argc; i++)
            if (!std::strcmp(argv[i], key)) return argv[i + 1];
        return def;
    }
    bool has(const char *key) const {
        for (int i = 1; i < argc; i++)
            if (!std::strcmp(argv[i], key)) return true;
        return false;
    }
    double num(const char *key, double def) const {
        const char *v = get(key);
        return v ? std::atof(v) : def;
    }
    long integer(const char *key, long def) const {
        const char *v = get(key);
        return v ? std::atol(v) : def;
    }
};

inline std::vector<double> parse_list(const char *s) {
    std::vector<double> out;
    std::string cur;
    for (const char *p = s;; ++p) {
        if (*p == ',' || *p == 0) {
            if (!cur.empty()) out.push_back(std::atof(cur.c_str()));
            cur.clear();
            if (*p == 0) break;
        } else
            cur.push_back(*p);
    }
    return out;
}

// "3,10-12,40" -> 3 10 11 12 40 (comma-separated indices and a-b ranges, a <= b); false for anything else
inline bool parse_index_list(const char *s, std::vector<long> &out) {
    const char *p = s;
    while (*p) {
        char *end = nullptr;
        if (*p < '0' || *p > '9') return false;
        const long a = std::strtol(p, &end, 10);
        long b = a;
        p = end;
        if (*p == '-') {
            ++p;
            if (*p < '0' || *p > '9') return false;
            b = std::strtol(p, &end, 10);
            p = end;
        }
        if (b < a || b - a > (1L << 24)) return false;
        for (long v = a; v <= b; v++) out.push_back(v);
        if (*p == ',') {
            if (!*++p) return false;
        } else if (*p)
            return false;
    }
    return !out.empty();
}

struct McOut {
    acg_ldpc_mc_result r;
    double fer() const { return (double) (r.total - r.correct) / (double) r.total; }            // experiment.h:59
    double avg_time() const { return r.time_sec / (double) r.total; }                           // :61
    double mean_hamming() const { return (double) r.sum_hamming / (double) r.total; }           // :63
    double mean_hamming_ok() const { return (double) r.sum_hamming_ok / (double) (r.correct > 1 ? r.correct : 1); }
    double mean_hamming_wrong() const {
        const int64_t w = r.total - r.correct;
        return (double) r.sum_hamming_wrong / (double) (w > 1 ? w : 1);
    }
};

// multithread_experiment (experiment.h:125-139) on the device
inline McOut run_mc(acg_ldpc_decoder *dec, const std::vector<uint8_t> &codewords, int n, double snr, int64_t frames,
                    int noise, uint64_t seed) {
    acg_ldpc_mc_cfg cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.frames = frames;
    cfg.snr = snr;
    cfg.seed = seed;
    cfg.noise = noise;
    cfg.codewords = codewords.empty() ? nullptr : codewords.data();
    cfg.n_codewords = codewords.empty() ? 0 : (int64_t) (codewords.size() / (size_t) n);
    McOut o;
    if (acg_ldpc_mc_run(dec, &cfg, &o.r)) die("acg_ldpc_mc_run");
    return o;
}

// acg_ldpc_mc_run_detail: the counters, and the stored events with their XOR rows left out (the drivers log records only)
struct DetailOut {
    acg_ldpc_mc_detail d;
    std::vector<acg_ldpc_mc_event> events;
    double fer() const { return (double) (d.base.total - d.base.correct) / (double) d.base.total; }
    double ber(int n) const { return (double) d.bit_errors / ((double) d.base.total * (double) n); }  // over returned words (acg_ldpc.h)
    double avg_syndrome_weight() const {
        return (double) d.sum_syndrome_weight / (double) (d.noncodeword_frames > 1 ? d.noncodeword_frames : 1);
    }
};

// shards -> one result: acg_ldpc_mc_detail_merge for the counters; events concatenated, sorted by frame, cut to cap
inline DetailOut merge_details(const std::vector<DetailOut> &part, int64_t cap) {
    DetailOut tot;
    std::memset(&tot.d, 0, sizeof tot.d);
    tot.d.min_pseudo_weight = -1;
    tot.d.min_pseudo_frame = -1;
    for (const DetailOut &p : part) {
        acg_ldpc_mc_detail_merge(&tot.d, &p.d);
        tot.events.insert(tot.events.end(), p.events.begin(), p.events.end());
    }
    std::stable_sort(tot.events.begin(), tot.events.end(),
                     [](const acg_ldpc_mc_event &x, const acg_ldpc_mc_event &y) { return x.frame < y.frame; });
    if ((int64_t) tot.events.size() > cap) tot.events.resize((size_t) cap);
    tot.d.n_stored = (int64_t) tot.events.size();
    return tot;
}

inline const char *event_kind_name(int32_t kind) {
    return kind == ACG_LDPC_EVENT_PSEUDO ? "PSEUDO" : kind == ACG_LDPC_EVENT_NO_WORD ? "NO_WORD" : kind == ACG_LDPC_EVENT_NONCODEWORD ? "NONCODEWORD" : "?";
}

// codewords the way every reference driver makes them: G = GetOrtogonal(H) (or a G file), gen_random_codewords(G, mt19937(seed))
inline std::vector<uint8_t> make_codewords(const acg_ldpc_code *code, const char *gpath, uint32_t seed, int64_t count, bool *ok) {
    int m, n, E;
    acg_ldpc_code_dims(code, &m, &n, &E);
    std::vector<uint8_t> G;
    int k = n - m;
    *ok = true;
    if (gpath) {
        acg_ldpc_code *g = nullptr;
        if (acg_ldpc_code_load_txt(gpath, &g)) die("load G");
        int gm, gn, ge;
        acg_ldpc_code_dims(g, &gm, &gn, &ge);
        if (gn != n) {
            std::fprintf(stderr, "G has %d columns, H has %d\n", gn, n);
            std::exit(1);
        }
        k = gm;
        G.resize((size_t) gm * gn);
        acg_ldpc_code_dense(g, G.data());
        acg_ldpc_code_destroy(g);
    } else {
        G.resize((size_t) k * n);
        const int rc = acg_ldpc_code_generator(code, G.data());
        if (rc == 1) {
            *ok = false;  // GetOrtogonal's {TMatrix(), false}
            return {};
        }
        if (rc) die("generator");
    }
    std::vector<uint8_t> cw((size_t) count * n);
    if (acg_ldpc_gen_codewords(G.data(), k, n, seed, count, cw.data())) die("gen_codewords");
    return cw;
}

// One decoder handle per GPU; a Monte-Carlo run is cut into contiguous global frame ranges, one per handle, run from
// one host thread per device and merged with acg_ldpc_mc_merge (experiment.h:70-78) — frames are independent, so
// nothing but seven counters crosses devices.  Device k of `gpus` maps to ordinal k % device_count, so
// the sharding logic can be exercised on a one-GPU box.
struct MultiGpu {
    std::vector<acg_ldpc_decoder *> dec;

    // quant != null: the fixed-point layered min-sum engine with that quantiser, in LDS or (streamed) in device memory;
    // layered_streamed (quant null): the streamed float layered engine
    void create(const acg_ldpc_code *code, acg_ldpc_params p, int gpus, int device_count, const acg_ldpc_quant *quant = nullptr,
                bool streamed = false, bool layered_streamed = false) {
        for (int k = 0; k < gpus; k++) {
            p.device = device_count > 0 ? k % device_count : -1;
            acg_ldpc_decoder *d = nullptr;
            if (layered_streamed) {
                if (acg_ldpc_decoder_create_layered_streamed(code, &p, &d)) die("acg_ldpc_decoder_create_layered_streamed");
            } else if (quant && streamed) {
                if (acg_ldpc_decoder_create_quantized_streamed(code, &p, quant, &d)) die("acg_ldpc_decoder_create_quantized_streamed");
            } else if (quant) {
                if (acg_ldpc_decoder_create_quantized(code, &p, quant, &d)) die("acg_ldpc_decoder_create_quantized");
            } else if (acg_ldpc_decoder_create(code, &p, &d))
                die("acg_ldpc_decoder_create");
            dec.push_back(d);
        }
    }
    void destroy() {
        for (auto *d : dec) acg_ldpc_decoder_destroy(d);
        dec.clear();
    }
    const char *name() const { return acg_ldpc_decoder_name(dec[0]); }

    // rm != null: a rate-matched run (acg_ldpc_mc_run_rm) with that pattern of n bytes
    McOut run(const std::vector<uint8_t> &codewords, int n, double snr, int64_t frames, int noise, uint64_t seed,
              const std::vector<uint8_t> *rm = nullptr) const {
        const char *call = rm ? "acg_ldpc_mc_run_rm" : "acg_ldpc_mc_run";
        const int W = (int) dec.size();
        std::vector<McOut> part((size_t) W);
        std::vector<std::string> err((size_t) W);
        std::vector<std::thread> th;
        for (int r = 0; r < W; r++)
            th.emplace_back([&, r] {
                const int64_t lo = frames * r / W, hi = frames * (r + 1) / W;
                acg_ldpc_mc_cfg cfg;
                std::memset(&cfg, 0, sizeof cfg);
                cfg.frames = hi - lo;
                cfg.first_frame = lo;  // seeds derive from the GLOBAL frame index: same frames for any W
                cfg.snr = snr;
                cfg.seed = seed;
                cfg.noise = noise;
                cfg.codewords = codewords.empty() ? nullptr : codewords.data();
                cfg.n_codewords = codewords.empty() ? 0 : (int64_t) (codewords.size() / (size_t) n);
                const int rc = rm ? acg_ldpc_mc_run_rm(dec[(size_t) r], &cfg, rm->data(), &part[(size_t) r].r)
                                  : acg_ldpc_mc_run(dec[(size_t) r], &cfg, &part[(size_t) r].r);
                if (rc) err[(size_t) r] = acg_ldpc_last_error();
            });
        for (auto &t : th) t.join();
        McOut tot;
        std::memset(&tot.r, 0, sizeof tot.r);
        double wall = 0;
        for (int r = 0; r < W; r++) {
            if (!err[(size_t) r].empty()) {
                std::fprintf(stderr, "%s (shard %d): %s\n", call, r, err[(size_t) r].c_str());
                std::exit(1);
            }
            wall = wall > part[(size_t) r].r.time_sec ? wall : part[(size_t) r].r.time_sec;
            acg_ldpc_mc_merge(&tot.r, &part[(size_t) r].r);
        }
        tot.r.time_sec = wall;  // shards run concurrently: the slowest one is the wall time
        return tot;
    }

    // the same through acg_ldpc_mc_run_detail: every shard keeps up to cap events of its own range, merged as merge_details says
    DetailOut run_detail(const std::vector<uint8_t> &codewords, int n, double snr, int64_t frames, int noise, uint64_t seed,
                         int64_t cap) const {
        const int W = (int) dec.size();
        std::vector<DetailOut> part((size_t) W);
        std::vector<std::string> err((size_t) W);
        std::vector<std::thread> th;
        for (int r = 0; r < W; r++)
            th.emplace_back([&, r] {
                const int64_t lo = frames * r / W, hi = frames * (r + 1) / W;
                acg_ldpc_mc_cfg cfg;
                std::memset(&cfg, 0, sizeof cfg);
                cfg.frames = hi - lo;
                cfg.first_frame = lo;
                cfg.snr = snr;
                cfg.seed = seed;
                cfg.noise = noise;
                cfg.codewords = codewords.empty() ? nullptr : codewords.data();
                cfg.n_codewords = codewords.empty() ? 0 : (int64_t) (codewords.size() / (size_t) n);
                DetailOut &o = part[(size_t) r];
                o.events.resize((size_t) cap);
                if (acg_ldpc_mc_run_detail(dec[(size_t) r], &cfg, &o.d, cap ? o.events.data() : nullptr, nullptr, cap))
                    err[(size_t) r] = acg_ldpc_last_error();
                else
                    o.events.resize((size_t) o.d.n_stored);
            });
        for (auto &t : th) t.join();
        double wall = 0;
        for (int r = 0; r < W; r++) {
            if (!err[(size_t) r].empty()) {
                std::fprintf(stderr, "acg_ldpc_mc_run_detail (shard %d): %s\n", r, err[(size_t) r].c_str());
                std::exit(1);
            }
            wall = wall > part[(size_t) r].d.base.time_sec ? wall : part[(size_t) r].d.base.time_sec;
        }
        DetailOut tot = merge_details(part, cap);
        tot.d.base.time_sec = wall;
        return tot;
    }
};

}  // namespace drv
