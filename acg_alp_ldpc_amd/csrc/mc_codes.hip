// C ABI of libacg_ldpc_hip.so (include/acg_ldpc.h), part 3b: Monte-Carlo over a batch of parity-check matrices, on an object
// of its own (the evaluator) with its own ring and tables; what it shares with the runs on a decoder handle is mc.hip's.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "handle.hpp"

using namespace acg;

// The local search of optimize_H.cpp:89-104 scores a fresh H per proposal.  An evaluator scores a batch of them in one
// call: the codes that the workgroup-per-frame QP-ADMM kernel accepts decode in ONE launch per launch shape (codes
// instance of admm_block_kernel, virtual frame g = code * frames + f), with their tables in one device buffer written by
// one copy; nothing is allocated, created or destroyed per code.
struct acg_ldpc_evaluator {
    acg_ldpc_params p;
    int device = 0;
    int cu_count = 256;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around the decode launch of the chunk in flight
    mutable std::mutex mu;  // (mutable: acg_ldpc_evaluator_describe reads `last` under it)
    static constexpr int WORK_RING = 32;  // per-launch work counters, as acg_ldpc_decoder::work_ring
    DeviceBuf work_ring;
    uint64_t launch_seq = 0;
    DeviceBuf st_y, st_bits, st_ok, st_iters;  // symbols [code][frame][n] and decode outputs of the chunk in flight
    DeviceBuf noise;     // host-noise mode: the deviates [frame][n] of the frame block in flight, shared by every code
    PinnedBuf pin_tab;   // host image of tab
    DeviceBuf tab;       // the chunk in flight: AdmmDevTables[codes] | CodeRef[codes] | per code: its tables, its sent words
    DeviceBuf counters;  // [codes of the call][MC_NCOUNTERS]
    std::string last = "qpadmm mc_codes=none";  // what the last run did (acg_ldpc_evaluator_describe)
};

static int acg_ldpc_evaluator_create_impl(const acg_ldpc_params *params, acg_ldpc_evaluator **out) {
    if (!params || !out) {
        set_error("null argument");
        return 1;
    }
    if (params->algo != ACG_LDPC_QPADMM) {
        set_error("acg_ldpc_evaluator_create needs QP-ADMM parameters");
        return 1;
    }
    if (params->max_iter < 0) {
        set_error("max_iter must be >= 0");
        return 1;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available: libacg_ldpc_hip has no CPU fallback");
        return 20;
    }
    int dev = params->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (dev >= ndev) {
        set_error("device ordinal out of range");
        return 1;
    }
    struct Drop { void operator()(acg_ldpc_evaluator *x) const { acg_ldpc_evaluator_destroy(x); } };
    std::unique_ptr<acg_ldpc_evaluator, Drop> own(new acg_ldpc_evaluator());
    acg_ldpc_evaluator *ev = own.get();
    ev->p = *params;
    ev->p.fast_setup = 1;  // (the contract: every code as on a decoder created with fast_setup = 1)
    ev->device = dev;
    HIP_OK(hipSetDevice(dev));
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, dev));
    ev->cu_count = prop.multiProcessorCount;
    HIP_OK(hipStreamCreateWithFlags(&ev->stream, hipStreamNonBlocking));
    HIP_OK(hipEventCreate(&ev->ev0));
    HIP_OK(hipEventCreate(&ev->ev1));
    if (int rc = ev->work_ring.reserve(sizeof(unsigned long long) * acg_ldpc_evaluator::WORK_RING)) return rc;
    *out = own.release();
    return 0;
}

static int acg_ldpc_mc_run_codes_impl(acg_ldpc_evaluator *ev, const acg_ldpc_code *const *codes, int32_t n_codes,
                                      const acg_ldpc_mc_cfg *cfgs, acg_ldpc_mc_result *res) {
    if (n_codes < 1) {
        set_error("acg_ldpc_mc_run_codes: n_codes must be >= 1");
        return 1;
    }
    if (!ev || !codes || !cfgs || !res) {
        set_error("null argument");
        return 1;
    }
    for (int32_t k = 0; k < n_codes; k++) {
        if (!codes[k]) {
            set_error("null argument");
            return 1;
        }
        if (codes[k]->c.m != codes[0]->c.m || codes[k]->c.n != codes[0]->c.n) {
            set_error("acg_ldpc_mc_run_codes: codes of different m or n");
            return 1;
        }
        if (check_mc_cfg(&cfgs[k])) return 1;
        if (cfgs[k].frames != cfgs[0].frames || cfgs[k].first_frame != cfgs[0].first_frame || !(cfgs[k].snr == cfgs[0].snr) ||
            cfgs[k].seed != cfgs[0].seed || cfgs[k].noise != cfgs[0].noise) {
            set_error("acg_ldpc_mc_run_codes: frames, first_frame, snr, seed and noise must be equal in every cfg");
            return 1;
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::memset(res, 0, sizeof(*res) * (size_t) n_codes);
    std::lock_guard<std::mutex> lk(ev->mu);
    HIP_OK(hipSetDevice(ev->device));
    const acg_ldpc_params &p = ev->p;
    const acg_ldpc_mc_cfg &cfg = cfgs[0];
    const int n = codes[0]->c.n, m = codes[0]->c.m, nwords = (n + 31) / 32;
    const int host = cfg.noise == ACG_LDPC_NOISE_HOST_MT19937 ? 1 : 0;
    // parameters whose decoder handle runs the workgroup-per-frame kernel on the codes that kernel accepts
    const bool eligible = p.engine != ACG_LDPC_ENGINE_STREAMED && (p.lanes_per_frame == 0 || p.lanes_per_frame == 256) && p.max_iter > 0 &&
                          p.precision != ACG_LDPC_PREC_F16;
    struct Item {
        int32_t k;
        std::unique_ptr<AdmmDevice, acg_ldpc_decoder::AdmmDrop> plan;
        std::vector<unsigned char> blob;
    };
    std::vector<Item> items;                 // the codes that decode in shared launches
    std::vector<int32_t> guard, per_code;    // guard codes (qp_admm.h:108-114); codes that take a decoder handle of their own
    for (int32_t k = 0; k < n_codes && cfg.frames > 0; k++) {
        const Code &c = codes[k]->c;
        double e_min = 1e9;
        for (double e : c.admm.e) e_min = std::min(e_min, e);
        if (e_min * p.mu <= p.alpha) {
            guard.push_back(k);
            continue;
        }
        Item it;
        it.k = k;
        std::string why;
        if (eligible) it.plan.reset(admm_codes_plan(c, p, it.blob, why));
        if (it.plan) items.push_back(std::move(it));
        else per_code.push_back(k);
    }
    // launch groups: the codes of one launch shape, in the order given; group -1 = the guard codes (classified, never decoded)
    std::vector<std::pair<int, std::vector<const Item *>>> groups;
    for (const Item &it : items) {
        const int shape = admm_codes_shape(it.plan.get());
        size_t g = 0;
        while (g < groups.size() && groups[g].first != shape) g++;
        if (g == groups.size()) groups.push_back({shape, {}});
        groups[g].second.push_back(&it);
    }
    const int n_groups = (int) groups.size();
    std::vector<Item> guard_items(guard.size());
    if (!guard.empty()) {
        groups.push_back({-1, {}});
        for (size_t j = 0; j < guard.size(); j++) {
            guard_items[j].k = guard[j];
            groups.back().second.push_back(&guard_items[j]);
        }
    }
    int rc = 0, n_chunks = 0;
    if (!groups.empty()) {
        const int64_t budget = mc_grid_budget();
        const size_t counter_bytes = (size_t) n_codes * MC_NCOUNTERS * sizeof(unsigned long long);
        if ((rc = ev->counters.reserve(counter_bytes))) return rc;
        unsigned long long *counters = ev->counters.as<unsigned long long>();
        HIP_OK(hipMemsetAsync(counters, 0, counter_bytes, ev->stream));
        const size_t TB = admm_codes_tables_bytes();
        auto up = [](size_t x) { return (x + 255) & ~(size_t) 255; };
        // (one block is kept: with frames <= budget — the search's 1000 — it is drawn and uploaded once per call.  With more
        // frames than the budget a chunk is one code and every code redraws the blocks: correct, and not the case this serves)
        std::vector<double> nz;          // host noise of the frame block [nz_first, nz_first + nz_fc)
        int64_t nz_first = -1, nz_fc = 0;
        bool nz_on_device = false;
        std::vector<size_t> blob_off, cw_off;
        for (const auto &grp : groups) {
            const bool decode = grp.first >= 0;
            const int64_t n_grp = (int64_t) grp.second.size();
            const PointChunks pc = point_chunks(budget, cfg.frames, n_grp);   // (the points are the codes of the group)
            const int64_t fb = pc.fb, npc = pc.npc;
            for (int64_t c0 = 0; c0 < n_grp; c0 += npc) {
                const int64_t np = std::min(npc, n_grp - c0);
                const Item *const *chunk = grp.second.data() + c0;
                // ---- the chunk's tables: one host image, one copy (the stream is idle here: every chunk ends with a synchronisation)
                size_t total = up((size_t) np * TB) + up((size_t) np * sizeof(CodeRef)), lds = 0;
                blob_off.assign((size_t) np, 0);
                cw_off.assign((size_t) np, 0);
                for (int64_t j = 0; j < np; j++) {
                    const acg_ldpc_mc_cfg &cj = cfgs[chunk[j]->k];
                    blob_off[(size_t) j] = total;
                    total += up(chunk[j]->blob.size());
                    cw_off[(size_t) j] = total;
                    if (cj.codewords) total += up((size_t) cj.n_codewords * nwords * sizeof(uint32_t));
                    if (decode) lds = std::max(lds, admm_codes_lds(chunk[j]->plan.get()));
                }
                if ((rc = ev->tab.reserve(total)) || (rc = ev->pin_tab.reserve(total))) return rc;
                unsigned char *hp = ev->pin_tab.as<unsigned char>(), *dp = ev->tab.as<unsigned char>();
                std::memset(hp, 0, total);
                CodeRef *refs_h = reinterpret_cast<CodeRef *>(hp + up((size_t) np * TB));
                const CodeRef *refs = reinterpret_cast<const CodeRef *>(dp + up((size_t) np * TB));
                for (int64_t j = 0; j < np; j++) {
                    const Item &it = *chunk[j];
                    const acg_ldpc_mc_cfg &cj = cfgs[it.k];
                    CodeRef &r = refs_h[j];
                    r.cw_packed = nullptr;
                    r.n_cw = 1;
                    r.row_ptr = r.edge_var = nullptr;
                    r.counters = counters + (size_t) it.k * MC_NCOUNTERS;
                    if (decode) {
                        std::memcpy(hp + blob_off[(size_t) j], it.blob.data(), it.blob.size());
                        admm_codes_tables(it.plan.get(), (uintptr_t) (dp + blob_off[(size_t) j]), hp + (size_t) j * TB);
                        size_t rp = 0, evr = 0;
                        admm_codes_csr(it.plan.get(), &rp, &evr);
                        r.row_ptr = reinterpret_cast<const int32_t *>(dp + blob_off[(size_t) j] + rp);
                        r.edge_var = reinterpret_cast<const int32_t *>(dp + blob_off[(size_t) j] + evr);
                    }
                    if (cj.codewords) {
                        pack_codewords(cj.codewords, cj.n_codewords, n, reinterpret_cast<uint32_t *>(hp + cw_off[(size_t) j]));
                        r.cw_packed = reinterpret_cast<const uint32_t *>(dp + cw_off[(size_t) j]);
                        r.n_cw = cj.n_codewords;
                    }
                }
                HIP_OK(hipMemcpyAsync(dp, hp, total, hipMemcpyHostToDevice, ev->stream));
                int grid_cap = 0;
                if (decode) {
                    std::string why;
                    grid_cap = admm_codes_grid_cap(chunk[0]->plan.get(), lds, ev->cu_count, why);
                    if (grid_cap <= 0) {
                        set_error(why);
                        return 10;
                    }
                    n_chunks++;
                }
                const size_t vf = (size_t) (np * fb);
                if ((rc = ev->st_y.reserve(vf * n * (host ? sizeof(double) : sizeof(float))))) return rc;
                if (decode && ((rc = ev->st_bits.reserve(vf * nwords * sizeof(uint32_t))) || (rc = ev->st_ok.reserve(vf)) ||
                               (rc = ev->st_iters.reserve(vf * sizeof(int32_t)))))
                    return rc;
                for (int64_t f0 = 0; f0 < cfg.frames; f0 += fb) {
                    const int64_t fc = std::min(fb, cfg.frames - f0), first = cfg.first_frame + f0;
                    // ---- symbols [code][frame][n]: one noise block serves every code
                    if (host) {
                        if (nz_first != first || nz_fc != fc) {
                            nz.resize((size_t) fc * n);
                            noise_host(n, first, fc, cfg.snr, nz.data());
                            nz_first = first;
                            nz_fc = fc;
                            nz_on_device = false;
                        }
                        if (!nz_on_device) {
                            if ((rc = ev->noise.reserve(nz.size() * sizeof(double)))) return rc;
                            HIP_OK(hipMemcpyAsync(ev->noise.p, nz.data(), nz.size() * sizeof(double), hipMemcpyHostToDevice, ev->stream));
                            nz_on_device = true;
                        }
                        HIP_OK(codes_symbols_launch(ev->noise.as<double>(), ev->st_y.as<double>(), fc, np, n, nwords, first, refs, ev->stream));
                    } else {
                        for (int64_t j = 0; j < np; j++)
                            HIP_OK(awgn_launch(ev->st_y.as<float>() + (size_t) j * fc * n, fc, n, nwords, first, cfg.seed, refs_h[j].cw_packed,
                                               refs_h[j].n_cw, (float) channel_sigma(cfg.snr), ev->stream));
                    }
                    if (!decode) {
                        HIP_OK(classify_codes_launch(ev->st_y.p, host, nullptr, nullptr, nullptr, fc, np, n, nwords, first, refs, m, ev->stream));
                        HIP_OK(hipStreamSynchronize(ev->stream));
                        continue;
                    }
                    DecodeArgs a = decode_args(ev->st_y.p, host, np * fc, cfg.snr);
                    a.out_bits = ev->st_bits.as<uint32_t>();
                    a.out_ok = ev->st_ok.as<uint8_t>();
                    a.out_iters = ev->st_iters.as<int32_t>();
                    a.max_iter = p.max_iter;
                    a.early_exit = p.early_exit;
                    a.ms_scale = (float) p.ms_scale;
                    a.work_counter = ev->work_ring.as<unsigned long long>() + (ev->launch_seq++ % acg_ldpc_evaluator::WORK_RING);
                    HIP_OK(hipMemsetAsync(a.work_counter, 0, sizeof(unsigned long long), ev->stream));
                    HIP_OK(hipEventRecord(ev->ev0, ev->stream));
                    HIP_OK(admm_codes_launch(chunk[0]->plan.get(), dp, (uint32_t) fc, lds, grid_cap, a, ev->stream));
                    HIP_OK(hipEventRecord(ev->ev1, ev->stream));
                    HIP_OK(classify_codes_launch(ev->st_y.p, host, a.out_bits, a.out_ok, a.out_iters, fc, np, n, nwords, first, refs, m, ev->stream));
                    HIP_OK(hipStreamSynchronize(ev->stream));
                    float ms = 0;
                    if (hipEventElapsedTime(&ms, ev->ev0, ev->ev1) == hipSuccess)
                        for (int64_t j = 0; j < np; j++) res[chunk[j]->k].kernel_ms += (double) ms / (double) np;
                }
            }
        }
        std::vector<unsigned long long> h((size_t) n_codes * MC_NCOUNTERS);
        HIP_OK(hipMemcpy(h.data(), counters, counter_bytes, hipMemcpyDeviceToHost));
        for (const auto &grp : groups)
            for (const Item *it : grp.second) {
                const double kms = res[it->k].kernel_ms;
                counters_to_result(&h[(size_t) it->k * MC_NCOUNTERS], &res[it->k]);
                res[it->k].kernel_ms = kms;
            }
    }
    // codes the shared launches do not take: a decoder handle of their own, on this evaluator's stream
    for (size_t j = 0; j < per_code.size() && !rc; j++) {
        const int32_t k = per_code[j];
        acg_ldpc_decoder *d = nullptr;
        if ((rc = acg_ldpc_decoder_create_impl(codes[k], &p, &d, ev->stream))) break;
        rc = acg_ldpc_mc_run_impl(d, &cfgs[k], &res[k]);
        const std::string keep = rc ? last_error() : std::string();
        acg_ldpc_decoder_destroy(d);
        if (rc) set_error(keep);
    }
    char b[256];
    if (n_groups > 0 || (eligible && per_code.empty()))
        snprintf(b, sizeof b, "qpadmm mc_codes=single-launch groups=%d chunks=%d codes=%d guard=%d per_code=%d", n_groups, n_chunks, (int) n_codes,
                 (int) guard.size(), (int) per_code.size());
    else
        snprintf(b, sizeof b, "qpadmm mc_codes=per-code codes=%d guard=%d per_code=%d", (int) n_codes, (int) guard.size(), (int) per_code.size());
    ev->last = b;
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int32_t k = 0; k < n_codes; k++) res[k].time_sec = wall;
    return rc;
}

extern "C" {

int acg_ldpc_evaluator_create(const acg_ldpc_params *params, acg_ldpc_evaluator **out) {
    return guarded([&] { return acg_ldpc_evaluator_create_impl(params, out); });
}

void acg_ldpc_evaluator_destroy(acg_ldpc_evaluator *ev) {
    if (!ev) return;
    (void) hipSetDevice(ev->device);
    if (ev->stream) (void) hipStreamSynchronize(ev->stream);
    if (ev->ev0) (void) hipEventDestroy(ev->ev0);
    if (ev->ev1) (void) hipEventDestroy(ev->ev1);
    if (ev->stream) (void) hipStreamDestroy(ev->stream);
    delete ev;  // (the buffers belong to its members)
}

int acg_ldpc_mc_run_codes(acg_ldpc_evaluator *ev, const acg_ldpc_code *const *codes, int32_t n_codes, const acg_ldpc_mc_cfg *cfgs,
                          acg_ldpc_mc_result *res) {
    return guarded([&] { return acg_ldpc_mc_run_codes_impl(ev, codes, n_codes, cfgs, res); });
}

int32_t acg_ldpc_evaluator_describe(const acg_ldpc_evaluator *ev, char *buf, int32_t cap) {
    if (!ev) return 0;
    std::string s;
    {
        std::lock_guard<std::mutex> lk(ev->mu);  // (a run on another thread writes it)
        s = ev->last;
    }
    return copy_text(s, buf, cap);
}

}  // extern "C"
