// C ABI of libacg_ldpc_hip.so (include/acg_ldpc.h), part 3: Monte-Carlo on a decoder handle.  The two host loops the runs share
// — frames in chunks (mc_frames), points x frame blocks (mc_points) — and their callers: acg_ldpc_mc_run, the detail run, the run
// for punctured and shortened codes; the QP-ADMM parameter grid and the quantiser grid of the fixed-point engine.  Then the run
// through a cascade (cascade.hip) and the generators (device AWGN, host codewords and transmit).  The evaluator: mc_codes.hip.
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <random>

#include "handle.hpp"

using namespace acg;

// ---------------------------------------------------------------- Monte-Carlo
int acg::check_mc_cfg(const acg_ldpc_mc_cfg *cfg) {
    if (!(cfg->frames < 0 || (cfg->codewords && cfg->n_codewords <= 0))) return 0;
    set_error("bad mc cfg");
    return 1;
}

int64_t acg::env_frames(const char *name) {
    const char *e = getenv(name);
    return std::max<int64_t>(0, e ? atoll(e) : 0);
}

// one byte per bit -> packed words, ORed into out[n_codewords][(n + 31) / 32] (the caller zeroes it)
void acg::pack_codewords(const uint8_t *codewords, int64_t n_codewords, int n, uint32_t *out) {
    const int nwords = (n + 31) / 32;
    for (int64_t f = 0; f < n_codewords; f++)
        for (int v = 0; v < n; v++)
            if (codewords[(size_t) f * n + v]) out[(size_t) f * nwords + (v >> 5)] |= 1u << (v & 31);
}

static int ensure_codewords(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg) {
    if (!cfg->codewords || cfg->n_codewords <= 0) return 0;
    // the device copy is keyed on the CONTENT of the host array (a pointer can be recycled for different words)
    // (hashed 8 bytes at a time in four independent lanes: the byte-wise loop took 2.5 ms for 8192 x 280 codewords — more than
    // an early-exit launch over a million frames — on every Monte-Carlo call)
    uint64_t h = 1469598103934665603ull;
    {
        const uint8_t *pb = cfg->codewords;
        const size_t nb = (size_t) cfg->n_codewords * (size_t) d->c.n;
        uint64_t hl[4] = {h, h ^ 0x9E3779B97F4A7C15ull, h ^ 0xC2B2AE3D27D4EB4Full, h ^ 0x165667B19E3779F9ull};
        size_t i = 0;
        for (; i + 32 <= nb; i += 32)
            for (int k = 0; k < 4; k++) {
                uint64_t w;
                std::memcpy(&w, pb + i + 8 * k, 8);
                // any non-zero byte means bit 1 (the reference reads '1' cells, others are 0): normalise every byte to 0 / 1
                w |= w >> 4;
                w |= w >> 2;
                w |= w >> 1;
                w &= 0x0101010101010101ull;
                hl[k] = (hl[k] ^ w) * 1099511628211ull;
                hl[k] ^= hl[k] >> 29;
            }
        for (; i < nb; i++) hl[0] = (hl[0] ^ (uint64_t) (pb[i] != 0)) * 1099511628211ull;
        h = ((hl[0] * 31 + hl[1]) * 31 + hl[2]) * 31 + hl[3];
    }
    if (d->cw_dev.p && d->cw_hash == h && d->cw_count == cfg->n_codewords) return 0;
    d->cw_dev.reset();  // (hipFree waits for the device: no launch still reads the old words when the new ones are copied)
    const int n = d->c.n, nwords = (n + 31) / 32;
    std::vector<uint32_t> packed((size_t) cfg->n_codewords * nwords, 0u);
    pack_codewords(cfg->codewords, cfg->n_codewords, n, packed.data());
    if (int rc = d->cw_dev.reserve(packed.size() * sizeof(uint32_t))) return rc;
    HIP_OK(hipMemcpy(d->cw_dev.p, packed.data(), packed.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    d->cw_hash = h;
    d->cw_count = cfg->n_codewords;
    return 0;
}

// the sent words as the kernels take them: (packed device copy, count), or (null, 1) for the all-zero word
struct SentWords {
    const uint32_t *dev;
    int64_t n;
};
static SentWords sent_words(const acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg) {
    if (!cfg->codewords) return {nullptr, 1};
    return {d->cw_dev.as<uint32_t>(), cfg->n_codewords};
}

void acg::counters_to_result(const unsigned long long *c, acg_ldpc_mc_result *r) {
    r->correct = (int64_t) c[MC_CORRECT];
    r->pseudo = (int64_t) c[MC_PSEUDO];
    r->total = (int64_t) c[MC_TOTAL];
    r->sum_hamming = (int64_t) c[MC_HAM];
    r->sum_hamming_ok = (int64_t) c[MC_HAM_OK];
    r->sum_hamming_wrong = (int64_t) c[MC_HAM_WRONG];
    r->sum_iters = (int64_t) c[MC_ITERS];
}

// The noise of experiment.h:90-99 (single-threaded order): frame g (0-based global index) is seeded mt19937(g+1) and draws its
// n deviates from libstdc++ normal_distribution(0, sigma) in index order (channel.h:18-26)
void acg::noise_host(int n, int64_t first, int64_t fc, double snr, double *out) {
    const double sigma = channel_sigma(snr);
    for (int64_t f = 0; f < fc; f++) {
        std::mt19937 rnd((uint32_t) (first + f + 1));
        std::normal_distribution<double> dst(0, sigma);
        for (int i = 0; i < n; i++) out[(size_t) f * n + i] = dst(rnd);
    }
}

// Bit-exact transmit of experiment.h:90-99: that noise, and per symbol the single IEEE addition (+-1.0) + deviate
// (channel.h:24); codewords == null sends the all-zero word
static void transmit_host(const uint8_t *codewords, int64_t n_codewords, int n, int64_t first_frame, int64_t frames, double snr, double *y) {
    noise_host(n, first_frame, frames, snr, y);
    for (int64_t f = 0; f < frames; f++) {
        const uint8_t *cw = codewords ? codewords + (size_t) ((first_frame + f) % n_codewords) * n : nullptr;
        for (int i = 0; i < n; i++) y[(size_t) f * n + i] = ((cw && cw[i]) ? -1.0 : 1.0) + y[(size_t) f * n + i];
    }
}

// the device generator's symbols of frames [first, first + fc) of cfg, the sent words from the handle's copy.  Caller holds d->mu.
static int awgn_frames(const acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, int64_t first, int64_t fc, float *dst, hipStream_t s) {
    const SentWords cw = sent_words(d, cfg);
    HIP_OK(awgn_launch(dst, fc, d->c.n, (d->c.n + 31) / 32, first, cfg->seed, cw.dev, cw.n, (float) channel_sigma(cfg->snr), s));
    return 0;
}

// Channel symbols of frames [first, first + fc) of cfg into the device buffer dst, on stream s: doubles from mt19937
// (experiment.h:90-99, as mc_run_host_noise; yh is the host image, which the copy reads until s is synchronised) or floats from
// the device generator (awgn_frames, which the loops that run device noise only call directly).  Caller holds d->mu.
static int mc_symbols(const acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, int64_t first, int64_t fc, void *dst, hipStream_t s, std::vector<double> &yh) {
    if (cfg->noise != ACG_LDPC_NOISE_HOST_MT19937) return awgn_frames(d, cfg, first, fc, static_cast<float *>(dst), s);
    yh.resize((size_t) fc * d->c.n);
    transmit_host(cfg->codewords, cfg->n_codewords, d->c.n, first, fc, cfg->snr, yh.data());
    HIP_OK(hipMemcpyAsync(dst, yh.data(), yh.size() * sizeof(double), hipMemcpyHostToDevice, s));
    return 0;
}

extern "C" void acg_ldpc_mc_merge(acg_ldpc_mc_result *a, const acg_ldpc_mc_result *b) {
    // merge_exp_results, experiment.h:70-78
    a->correct += b->correct;
    a->pseudo += b->pseudo;
    a->total += b->total;
    a->sum_hamming += b->sum_hamming;
    a->sum_hamming_ok += b->sum_hamming_ok;
    a->sum_hamming_wrong += b->sum_hamming_wrong;
    a->sum_iters += b->sum_iters;
    a->time_sec += b->time_sec;
    a->kernel_ms += b->kernel_ms;
}

// `chunk` frames as a developer / test variable lowers them: ACG_MC_CHUNK, ACG_MC_DETAIL_CHUNK, ACG_MC_RM_CHUNK (README)
static int64_t lowered_chunk(int64_t chunk, const char *name) {
    const int64_t v = env_frames(name);
    return v ? std::min(chunk, v) : chunk;
}

// where a detail run (acg_ldpc_mc_run_detail) collects what goes beyond the seven counters
struct DetailSink {
    acg_ldpc_mc_detail *out;
    acg_ldpc_mc_event *events;
    uint32_t *words;
    int64_t cap;
};

// a pseudo frame of weight w >= 1: the running minimum keeps the lowest frame among equal weights (a weight <= 0 in *o means
// "none yet": -1 as the API reports it, or 0 in an accumulator the caller zeroed)
static void detail_min_pseudo(acg_ldpc_mc_detail *o, int32_t w, int64_t frame) {
    if (o->min_pseudo_weight <= 0 || w < o->min_pseudo_weight || (w == o->min_pseudo_weight && frame < o->min_pseudo_frame)) {
        o->min_pseudo_weight = w;
        o->min_pseudo_frame = frame;
    }
}

static int mc_run_host_noise(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, acg_ldpc_mc_result *res, DetailSink *ds = nullptr) {
    // Bit-exact experiment.h:80-123: transmit_host, decoded on the device, classified on the host.
    const int n = d->c.n;
    const int64_t chunk_max = ds ? lowered_chunk(1 << 16, "ACG_MC_DETAIL_CHUNK") : 1 << 16;
    std::vector<double> y;
    std::vector<uint8_t> bits, ok;
    std::vector<int32_t> iters;
    for (int64_t f0 = 0; f0 < cfg->frames; f0 += chunk_max) {
        const int64_t fc = std::min(chunk_max, cfg->frames - f0);
        y.resize((size_t) fc * n);
        bits.resize((size_t) fc * n);
        ok.resize((size_t) fc);
        iters.resize((size_t) fc);
        transmit_host(cfg->codewords, cfg->n_codewords, n, cfg->first_frame + f0, fc, cfg->snr, y.data());
        if (int rc = acg_ldpc_decode_batch(d, y.data(), fc, cfg->snr, bits.data(), ok.data(), iters.data())) return rc;
        res->kernel_ms += acg_ldpc_decoder_last_kernel_ms(d);
        for (int64_t f = 0; f < fc; f++) {
            const int64_t gidx = cfg->first_frame + f0 + f;
            const uint8_t *cw = cfg->codewords ? cfg->codewords + (size_t) (gidx % cfg->n_codewords) * n : nullptr;
            const uint8_t *b = &bits[(size_t) f * n];
            bool is_correct = false, is_pseudo = false;
            if (ok[f] && code_is_codeword(d->c, b)) {  // experiment.h:110-111
                bool eq = true;
                for (int i = 0; i < n; i++) eq &= (b[i] == (cw ? cw[i] : 0));
                if (eq) {
                    res->correct++;
                    is_correct = true;
                } else {
                    res->pseudo++;
                    is_pseudo = true;
                }
            }
            res->total++;
            int h = 0;
            for (int i = 0; i < n; i++) {
                const bool c1 = cw && cw[i];
                const double yv = y[(size_t) f * n + i];
                if (!c1 && yv <= 0) h++;
                if (c1 && yv > 0) h++;
            }
            res->sum_hamming += h;
            if (is_correct) res->sum_hamming_ok += h;
            else res->sum_hamming_wrong += h;
            res->sum_iters += iters[f];
            if (ds) {   // the detail run's extension of experiment.h:109-120
                acg_ldpc_mc_detail *o = ds->out;
                int dist = 0, synw = 0;
                if (ok[f]) {
                    o->word_frames++;
                    for (int i = 0; i < n; i++) dist += (b[i] != 0) != (cw && cw[i]);
                    o->bit_errors += dist;
                    if (!is_correct && !is_pseudo) {
                        for (int c = 0; c < d->c.m; c++) {
                            int sy = 0;
                            for (int e = d->c.row_ptr[c]; e < d->c.row_ptr[c + 1]; e++) sy ^= b[d->c.edge_var[e]] != 0;
                            synw += sy;
                        }
                        o->noncodeword_frames++;
                        o->sum_syndrome_weight += synw;
                    }
                }
                if (is_pseudo) detail_min_pseudo(o, dist, gidx);
                if (!is_correct && o->n_stored < ds->cap) {
                    const int64_t k = o->n_stored++;
                    acg_ldpc_mc_event &ev = ds->events[k];
                    ev.frame = gidx;
                    ev.kind = is_pseudo ? ACG_LDPC_EVENT_PSEUDO : ok[f] ? ACG_LDPC_EVENT_NONCODEWORD : ACG_LDPC_EVENT_NO_WORD;
                    ev.iters = iters[f];
                    ev.raw_errors = h;
                    ev.bit_errors = dist;
                    ev.syndrome_weight = synw;
                    ev.reserved = 0;
                    if (ds->words) {
                        const int nwords = (n + 31) / 32;
                        uint32_t *row = ds->words + (size_t) k * nwords;
                        std::fill(row, row + nwords, 0u);
                        if (ok[f])
                            for (int i = 0; i < n; i++)
                                if ((b[i] != 0) != (cw && cw[i])) row[i >> 5] |= 1u << (i & 31);
                    }
                }
            }
        }
    }
    return 0;
}

// ---------------------------------------------------------------- frames in chunks on one handle
// The host loop of the device-noise runs that decode through the handle's ordinary launch: the unfused route of acg_ldpc_mc_run,
// the detail run, the rate-matched run.  It owns the lock, the codewords, the chunk size — max(256, min(frames, 2^31 /
// (4 n))) frames, lowered by the developer variable chunk_env — the chunk's channel elements (elem bytes each) in d->mc_y, its
// three staged outputs, the loop, the synchronisation that ends a chunk, and the chunks' kernel times (res->kernel_ms).  The caller's:
//   prepare(rows)          its own buffers for chunks of up to `rows` frames: all is reserved before the first enqueue
//   enqueue(first, fc, c)  frames [first, first + fc) on d->stream: generator -> decode_chunk into c -> classifier (-> its copies)
//   done(first, fc, c)     host work behind the chunk's synchronisation (the detail run's), or no_chunk_work
// counted: the classifier counts into d->counters, zeroed here and read into res behind the last chunk; else the caller's own.
// frames == 0 returns at once: nothing is locked, the device is not touched, and the results stay as the caller zeroed them.
template <class Prepare, class Enqueue, class Done>
static int mc_frames(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, size_t elem, const char *chunk_env, acg_ldpc_mc_result *res, bool counted,
                     Prepare prepare, Enqueue enqueue, Done done) {
    if (cfg->frames == 0) return 0;
    std::lock_guard<std::recursive_mutex> lk(d->mu);
    HIP_OK(hipSetDevice(d->device));
    if (int rc = ensure_codewords(d, cfg)) return rc;
    const int64_t cap = (int64_t) (1ull << 31) / ((int64_t) d->c.n * 4);
    const int64_t chunk = lowered_chunk(std::max<int64_t>(256, std::min<int64_t>(cfg->frames, cap)), chunk_env), rows = std::min(chunk, cfg->frames);
    int rc = 0;
    if ((rc = d->mc_y.reserve((size_t) rows * d->c.n * elem)) || (rc = reserve_outputs(d, rows)) || (rc = prepare(rows))) return rc;
    if (counted) HIP_OK(hipMemsetAsync(d->counters.p, 0, sizeof(unsigned long long) * MC_NCOUNTERS, d->stream));
    float kms = 0;
    for (int64_t f0 = 0; f0 < cfg->frames; f0 += chunk) {
        const int64_t fc = std::min(chunk, cfg->frames - f0), first = cfg->first_frame + f0;
        Chunk c;
        if ((rc = enqueue(first, fc, c))) return rc;
        HIP_OK(hipStreamSynchronize(d->stream));
        kms += chunk_ms(d, c);
        if ((rc = done(first, fc, c))) return rc;
    }
    res->kernel_ms = kms;
    if (!counted) return 0;
    unsigned long long h[MC_NCOUNTERS];
    HIP_OK(hipMemcpy(h, d->counters.p, sizeof(h), hipMemcpyDeviceToHost));
    counters_to_result(h, res);
    return 0;
}
static int no_chunk_work(int64_t, int64_t, const Chunk &) { return 0; }

// The handles whose acg_ldpc_mc_run takes the unfused route (AWGN kernel -> decode -> classify kernel in the chunks of mc_frames, all
// on the device) instead of one fused launch: the engines without an in-kernel generator, and the workgroup-per-frame QP-ADMM kernel,
// whose fused Monte-Carlo variant needs 156 VGPRs (3 waves/SIMD) against 117 (4) for the plain decode: 1.6 M vs 2.7 M frames/s.
static bool mc_unfused(const acg_ldpc_decoder *d) {
    return d->streamed || d->streaml || d->pair || d->osd || d->layered_wg != acg_ldpc_decoder::LayeredWg::none ||
           (d->layered && getenv("ACG_LAY_UNFUSED_MC")) || (d->admm && admm_device_unfused_mc(d->admm.get(), nullptr, nullptr));
}

int acg::acg_ldpc_mc_run_impl(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, acg_ldpc_mc_result *res) {
    if (!d || !cfg || !res) {
        set_error("null argument");
        return 1;
    }
    if (check_mc_cfg(cfg)) return 1;
    std::memset(res, 0, sizeof(*res));
    const auto t0 = std::chrono::steady_clock::now();
    int rc = 0;
    if (cfg->noise == ACG_LDPC_NOISE_HOST_MT19937) {
        rc = mc_run_host_noise(d, cfg, res);
    } else if (mc_unfused(d)) {
        const int32_t *csr_row = nullptr, *csr_col = nullptr;
        if (d->admm) (void) admm_device_unfused_mc(d->admm.get(), &csr_row, &csr_col);
        const int n = d->c.n, nwords = (n + 31) / 32;
        auto enqueue = [&](int64_t first, int64_t fc, Chunk &c) {
            float *mc_y = d->mc_y.as<float>();
            if (int e = awgn_frames(d, cfg, first, fc, mc_y, d->stream)) return e;
            if (int e = decode_chunk(d, mc_y, 0, fc, cfg->snr, c)) return e;
            const SentWords cw = sent_words(d, cfg);
            HIP_OK(classify_grid_launch(mc_y, 0, c.a.out_bits, c.a.out_ok, c.a.out_iters, fc, 1, n, nwords, first, cw.dev, cw.n, d->counters_dev(),
                                        csr_row, csr_col, d->c.m, d->stream));
            return 0;
        };
        rc = mc_frames(d, cfg, sizeof(float), "ACG_MC_CHUNK", res, true, [](int64_t) { return 0; }, enqueue, no_chunk_work);
    } else {
        std::lock_guard<std::recursive_mutex> lk(d->mu);
        HIP_OK(hipSetDevice(d->device));
        if ((rc = ensure_codewords(d, cfg))) return rc;
        HIP_OK(hipMemsetAsync(d->counters.p, 0, sizeof(unsigned long long) * MC_NCOUNTERS, d->stream));
        DecodeArgs a = decode_args(nullptr, 0, cfg->frames, cfg->snr);
        a.mc = 1;
        a.seed = cfg->seed;
        a.first_frame = cfg->first_frame;
        a.cw_packed = sent_words(d, cfg).dev;
        a.n_cw = sent_words(d, cfg).n;
        a.counters = d->counters_dev();
        if ((rc = launch_decode(d, a, d->stream))) return rc;
        const int slot = d->last_slot;   // this launch's own event pair (d->mu is held)
        unsigned long long h[MC_NCOUNTERS];
        HIP_OK(hipMemcpyAsync(h, d->counters.p, sizeof(h), hipMemcpyDeviceToHost, d->stream));
        HIP_OK(hipStreamSynchronize(d->stream));
        counters_to_result(h, res);
        float ms = 0;
        if (cfg->frames > 0 && slot >= 0 && hipEventElapsedTime(&ms, d->ring_ev0[slot], d->ring_ev[slot]) == hipSuccess) res->kernel_ms = ms;
    }
    res->time_sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

extern "C" int acg_ldpc_mc_run(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, acg_ldpc_mc_result *res) {
    return guarded([&] { return acg_ldpc_mc_run_impl(d, cfg, res); });
}

// ---------------------------------------------------------------- Monte-Carlo detail run
// Device noise: mc_frames, a chunk being AWGN kernel -> plain decode (launch_decode with a.y set: every engine has it) ->
// classify_detail_kernel, with the counters copied to pinned memory behind it.  Events: the kernel leaves one kind byte per
// frame; while fewer than cap events are stored the host reads those bytes, takes the lowest non-correct frames of the chunk,
// and gather_events_kernel writes their records and XOR rows from the chunk's still-resident symbols and outputs — the one
// second synchronisation a chunk can have.  Chunks run in ascending frame order, so the stored events are the cap lowest
// frames whatever the chunk size.  Caller holds nothing.
static int mc_run_detail_device(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, DetailSink &ds) {
    acg_ldpc_mc_detail *o = ds.out;
    const int32_t *csr_row = nullptr, *csr_col = nullptr;
    if (d->admm) (void) admm_device_unfused_mc(d->admm.get(), &csr_row, &csr_col);
    const int n = d->c.n, nwords = (n + 31) / 32;
    unsigned long long *cnt = nullptr, *cnt_h = nullptr;
    uint8_t *kind = nullptr;
    bool want_events = false;
    auto prepare = [&](int64_t rows) {
        const size_t fcap = (size_t) rows, ecap = (size_t) std::min<int64_t>(ds.cap, rows);   // ecap: events one chunk can add
        int e = 0;
        if ((e = d->det_counters.reserve(DET_NCOUNTERS * sizeof(unsigned long long))) ||
            (e = d->det_counters_h.reserve(DET_NCOUNTERS * sizeof(unsigned long long))) || (e = d->det_kind.reserve(fcap)))
            return e;
        if (ds.cap > 0 && ((e = d->det_kind_h.reserve(fcap)) || (e = d->det_sel.reserve(ecap * sizeof(int32_t))) ||
                           (e = d->det_sel_h.reserve(ecap * sizeof(int32_t))) || (e = d->det_events.reserve(ecap * sizeof(acg_ldpc_mc_event))) ||
                           (ds.words && (e = d->det_words.reserve(ecap * nwords * sizeof(uint32_t))))))
            return e;
        cnt = d->det_counters.as<unsigned long long>();
        cnt_h = d->det_counters_h.as<unsigned long long>();
        kind = d->det_kind.as<uint8_t>();
        HIP_OK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * DET_NCOUNTERS, d->stream));
        return 0;
    };
    auto enqueue = [&](int64_t first, int64_t fc, Chunk &c) {
        float *mc_y = d->mc_y.as<float>();
        HIP_OK(hipMemsetAsync(cnt + DET_MIN_PSEUDO, 0xFF, sizeof(unsigned long long), d->stream));
        if (int e = awgn_frames(d, cfg, first, fc, mc_y, d->stream)) return e;
        if (int e = decode_chunk(d, mc_y, 0, fc, cfg->snr, c)) return e;
        const SentWords cw = sent_words(d, cfg);
        HIP_OK(classify_detail_launch(mc_y, c.a.out_bits, c.a.out_ok, c.a.out_iters, fc, n, nwords, first, cw.dev, cw.n, cnt, kind, csr_row, csr_col,
                                      d->c.m, d->stream));
        want_events = o->n_stored < ds.cap;
        if (want_events) HIP_OK(hipMemcpyAsync(d->det_kind_h.p, kind, (size_t) fc, hipMemcpyDeviceToHost, d->stream));
        HIP_OK(hipMemcpyAsync(cnt_h, cnt, sizeof(unsigned long long) * DET_NCOUNTERS, hipMemcpyDeviceToHost, d->stream));
        return 0;
    };
    auto done = [&](int64_t first, int64_t fc, const Chunk &c) {
        counters_to_result(cnt_h, &o->base);   // (the running sums: the last chunk's stand)
        o->word_frames = (int64_t) cnt_h[DET_WORD_FRAMES];
        o->bit_errors = (int64_t) cnt_h[DET_BIT_ERRORS];
        o->noncodeword_frames = (int64_t) cnt_h[DET_NONCODEWORD];
        o->sum_syndrome_weight = (int64_t) cnt_h[DET_SYNDROME];
        if (cnt_h[DET_MIN_PSEUDO] != ~0ull)
            detail_min_pseudo(o, (int32_t) (cnt_h[DET_MIN_PSEUDO] >> 32), first + (int64_t) (cnt_h[DET_MIN_PSEUDO] & 0xFFFFFFFFull));
        if (!want_events) return 0;
        const uint8_t *kh = d->det_kind_h.as<uint8_t>();
        int32_t *sel = d->det_sel_h.as<int32_t>();
        const int64_t room = ds.cap - o->n_stored;
        int n_sel = 0;
        for (int64_t f = 0; f < fc && n_sel < room; f++)
            if (kh[f]) sel[n_sel++] = (int32_t) f;
        if (n_sel == 0) return 0;
        const SentWords cw = sent_words(d, cfg);
        HIP_OK(hipMemcpyAsync(d->det_sel.p, sel, (size_t) n_sel * sizeof(int32_t), hipMemcpyHostToDevice, d->stream));
        HIP_OK(gather_events_launch(d->det_sel.as<int32_t>(), n_sel, d->mc_y.as<float>(), c.a.out_bits, c.a.out_ok, c.a.out_iters, kind, n, nwords,
                                    first, cw.dev, cw.n, csr_row, csr_col, d->c.m, d->det_events.as<acg_ldpc_mc_event>(),
                                    ds.words ? d->det_words.as<uint32_t>() : nullptr, d->stream));
        HIP_OK(hipMemcpyAsync(ds.events + o->n_stored, d->det_events.p, (size_t) n_sel * sizeof(acg_ldpc_mc_event), hipMemcpyDeviceToHost, d->stream));
        if (ds.words)
            HIP_OK(hipMemcpyAsync(ds.words + (size_t) o->n_stored * nwords, d->det_words.p, (size_t) n_sel * nwords * sizeof(uint32_t),
                                  hipMemcpyDeviceToHost, d->stream));
        HIP_OK(hipStreamSynchronize(d->stream));
        o->n_stored += n_sel;
        return 0;
    };
    return mc_frames(d, cfg, sizeof(float), "ACG_MC_DETAIL_CHUNK", &o->base, false, prepare, enqueue, done);
}

static int acg_ldpc_mc_run_detail_impl(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, acg_ldpc_mc_detail *out,
                                       acg_ldpc_mc_event *events, uint32_t *words, int64_t cap) {
    if (!d || !cfg || !out) {
        set_error("null argument");
        return 1;
    }
    if (cap < 0 || (cap > 0 && !events)) {
        set_error("acg_ldpc_mc_run_detail: cap must be >= 0, and events non-null when cap > 0");
        return 1;
    }
    if (check_mc_cfg(cfg)) return 1;
    std::memset(out, 0, sizeof(*out));
    out->min_pseudo_weight = -1;
    out->min_pseudo_frame = -1;
    const auto t0 = std::chrono::steady_clock::now();
    DetailSink ds{out, events, words, cap};
    int rc = 0;
    if (cfg->noise == ACG_LDPC_NOISE_HOST_MT19937) rc = mc_run_host_noise(d, cfg, &out->base, &ds);
    else rc = mc_run_detail_device(d, cfg, ds);
    out->n_events = out->base.total - out->base.correct;
    out->base.time_sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

extern "C" int acg_ldpc_mc_run_detail(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, acg_ldpc_mc_detail *out, acg_ldpc_mc_event *events,
                                      uint32_t *words, int64_t cap) {
    return guarded([&] { return acg_ldpc_mc_run_detail_impl(d, cfg, out, events, words, cap); });
}

extern "C" void acg_ldpc_mc_detail_merge(acg_ldpc_mc_detail *a, const acg_ldpc_mc_detail *b) {
    acg_ldpc_mc_merge(&a->base, &b->base);
    a->word_frames += b->word_frames;
    a->bit_errors += b->bit_errors;
    a->noncodeword_frames += b->noncodeword_frames;
    a->sum_syndrome_weight += b->sum_syndrome_weight;
    a->n_events += b->n_events;
    if (b->min_pseudo_weight > 0) detail_min_pseudo(a, b->min_pseudo_weight, b->min_pseudo_frame);
    if (a->min_pseudo_weight <= 0) a->min_pseudo_weight = -1, a->min_pseudo_frame = -1;
}

// ---------------------------------------------------------------- points x frame blocks on one handle
// virtual frames (points x frames) one launch of a grid covers, and so the size of its per-frame outputs: the staging of a
// 65536-frame decode.  ACG_MC_GRID_BUDGET: developer / test override (README, developer variables).
int64_t acg::mc_grid_budget() {
    const int64_t v = env_frames("ACG_MC_GRID_BUDGET");
    return v ? std::min<int64_t>(v, (int64_t) 1 << 30) : 65536;
}

PointChunks acg::point_chunks(int64_t budget, int64_t frames, int64_t points) {
    const int64_t fb = std::min(frames, budget);
    return {fb, std::max<int64_t>(1, std::min(budget / fb, points))};
}

// The host loop of the grids that decode `points` points from the same frames in shared launches: the single-launch path of the
// QP-ADMM parameter grid, and the quantiser grid.  Frames in blocks of fb, points in chunks of npc: a block's symbols
// are drawn once, into d->st_y; a launch decodes np * fc virtual frames into the staged outputs, and classify_grid_kernel adds
// them to rows [c0, c0 + np) of d->grid_counters.  `rows` >= points rows are zeroed before and read into h behind the loop, the
// points' into res[res_of[j]] (null: res[j]) with their share of each chunk's kernel time; the others are the caller's.  The caller's:
//   block(first, fc, counters)  what it enqueues once per block behind the symbols (the parameter grid's guard row)
//   decode(c0, np, fc, c)       points [c0, c0 + np) over the block's fc frames: what their launch needs, and decode_chunk into c
// Caller holds d->mu and has set the device; cfg->frames > 0.
struct PointsRun {
    int64_t budget, points, rows;
    const int32_t *res_of, *csr_row, *csr_col;   // (csr: for QP-ADMM, whose flag is not IsCodeword; or null)
};
template <class Block, class Decode>
static int mc_points(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, const PointsRun &run, acg_ldpc_mc_result *res,
                     std::vector<unsigned long long> &h, Block block, Decode decode) {
    int rc = ensure_codewords(d, cfg);
    if (rc) return rc;
    const int n = d->c.n, nwords = (n + 31) / 32;
    const int host = cfg->noise == ACG_LDPC_NOISE_HOST_MT19937 ? 1 : 0;
    const SentWords cw = sent_words(d, cfg);
    const auto [fb, npc] = point_chunks(run.budget, cfg->frames, run.points);
    if ((rc = d->st_y.reserve((size_t) fb * n * sizeof(double))) || (rc = reserve_outputs(d, npc * fb))) return rc;
    const size_t counter_bytes = (size_t) run.rows * MC_NCOUNTERS * sizeof(unsigned long long);
    if ((rc = d->grid_counters.reserve(counter_bytes))) return rc;
    unsigned long long *counters = d->grid_counters.as<unsigned long long>();
    HIP_OK(hipMemsetAsync(counters, 0, counter_bytes, d->stream));
    auto res_of = [&](int64_t j) -> acg_ldpc_mc_result & { return res[run.res_of ? run.res_of[j] : j]; };
    std::vector<double> yh;
    for (int64_t f0 = 0; f0 < cfg->frames; f0 += fb) {
        const int64_t fc = std::min(fb, cfg->frames - f0), first = cfg->first_frame + f0;
        if ((rc = mc_symbols(d, cfg, first, fc, d->st_y.p, d->stream, yh))) return rc;
        if ((rc = block(first, fc, counters))) return rc;
        for (int64_t c0 = 0; c0 < run.points; c0 += npc) {
            const int64_t np = std::min(npc, run.points - c0);
            Chunk c;
            if ((rc = decode(c0, np, fc, c))) return rc;
            HIP_OK(classify_grid_launch(d->st_y.p, host, c.a.out_bits, c.a.out_ok, c.a.out_iters, fc, np, n, nwords, first, cw.dev, cw.n,
                                        counters + (size_t) c0 * MC_NCOUNTERS, run.csr_row, run.csr_col, d->c.m, d->stream));
            HIP_OK(hipStreamSynchronize(d->stream));
            const float ms = chunk_ms(d, c);
            for (int64_t j = 0; j < np; j++) res_of(c0 + j).kernel_ms += (double) ms / (double) np;
        }
        HIP_OK(hipStreamSynchronize(d->stream));  // (yh is rewritten by the next block)
    }
    h.resize((size_t) run.rows * MC_NCOUNTERS);
    HIP_OK(hipMemcpy(h.data(), counters, counter_bytes, hipMemcpyDeviceToHost));
    for (int64_t j = 0; j < run.points; j++) counters_to_result(&h[(size_t) j * MC_NCOUNTERS], &res_of(j));
    return 0;
}

// ---------------------------------------------------------------- Monte-Carlo over a QP-ADMM parameter grid
static int acg_ldpc_mc_run_grid_impl(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, const double *alpha, const double *mu,
                                     int32_t n_points, acg_ldpc_mc_result *res) {
    if (!d || !cfg) {
        set_error("null argument");
        return 1;
    }
    if (!d->admm) {
        set_error("acg_ldpc_mc_run_grid needs a QP-ADMM decoder");
        return 1;
    }
    if (n_points < 1) {
        set_error("acg_ldpc_mc_run_grid: n_points must be >= 1");
        return 1;
    }
    if (!alpha || !mu || !res) {
        set_error("null argument");
        return 1;
    }
    if (check_mc_cfg(cfg)) return 1;
    const auto t0 = std::chrono::steady_clock::now();
    std::memset(res, 0, sizeof(*res) * (size_t) n_points);
    std::lock_guard<std::recursive_mutex> lk(d->mu);
    HIP_OK(hipSetDevice(d->device));
    const double e_min = admm_device_e_min(d->admm.get());
    std::vector<int32_t> run, guard;  // the points that decode, and the guard points (qp_admm.h:108-114)
    for (int32_t k = 0; k < n_points; k++) (e_min * mu[k] <= alpha[k] ? guard : run).push_back(k);
    const int64_t n_run = (int64_t) run.size();
    const bool any_guard = !guard.empty();
    const bool single_launch = admm_device_has_grid_kernel(d->admm.get());
    int rc = 0;
    if (cfg->frames > 0 && (any_guard || (single_launch && n_run > 0))) {
        // mc_points over the points that decode in shared launches (none without the grid kernel: they follow below), with
        // one more counter row, n_run, that every guard point shares: a block's raw symbols classified once, without outputs
        const int n = d->c.n, nwords = (n + 31) / 32;
        const int host = cfg->noise == ACG_LDPC_NOISE_HOST_MT19937 ? 1 : 0;
        const int32_t *csr_row = nullptr, *csr_col = nullptr;
        (void) admm_device_unfused_mc(d->admm.get(), &csr_row, &csr_col);
        const PointsRun pr{mc_grid_budget(), single_launch ? n_run : 0, n_run + 1, run.data(), csr_row, csr_col};
        std::vector<unsigned long long> h;
        std::vector<double> ca, cm;
        std::vector<unsigned char> pt, inv;
        auto guard_row = [&](int64_t first, int64_t fc, unsigned long long *counters) {
            const SentWords cw = sent_words(d, cfg);
            if (any_guard)
                HIP_OK(classify_grid_launch(d->st_y.p, host, nullptr, nullptr, nullptr, fc, 1, n, nwords, first, cw.dev, cw.n,
                                            counters + (size_t) n_run * MC_NCOUNTERS, csr_row, csr_col, d->c.m, d->stream));
            return 0;
        };
        // the chunk's per-point tables, bound to the handle for the one launch that reads them
        auto decode = [&](int64_t c0, int64_t np, int64_t fc, Chunk &c) {
            ca.resize((size_t) np);
            cm.resize((size_t) np);
            for (int64_t j = 0; j < np; j++) {
                ca[(size_t) j] = alpha[run[(size_t) (c0 + j)]];
                cm[(size_t) j] = mu[run[(size_t) (c0 + j)]];
            }
            admm_grid_tables(d->admm.get(), ca.data(), cm.data(), (int) np, pt, inv);
            const size_t pt_bytes = (pt.size() + 255) & ~(size_t) 255;
            if (int e = d->grid_tab.reserve(pt_bytes + inv.size())) return e;
            unsigned char *tab = d->grid_tab.as<unsigned char>();
            // (the stream is idle here: the previous chunk ended with a synchronisation, so pt / inv may be rewritten)
            HIP_OK(hipMemcpyAsync(tab, pt.data(), pt.size(), hipMemcpyHostToDevice, d->stream));
            HIP_OK(hipMemcpyAsync(tab + pt_bytes, inv.data(), inv.size(), hipMemcpyHostToDevice, d->stream));
            admm_grid_bind(d->admm.get(), tab, tab + pt_bytes, (uint32_t) fc);
            const int e = decode_chunk(d, d->st_y.p, host, np * fc, cfg->snr, c);
            admm_grid_bind(d->admm.get(), nullptr, nullptr, 0);   // (released on the error path too)
            return e;
        };
        if ((rc = mc_points(d, cfg, pr, res, h, guard_row, decode))) return rc;
        for (int32_t k : guard) counters_to_result(&h[(size_t) n_run * MC_NCOUNTERS], &res[k]);
    }
    if (!single_launch && n_run > 0) {
        // one point after another on this handle: acg_ldpc_mc_run with the handle re-parameterised in place
        HIP_OK(hipStreamSynchronize(d->stream));
        const double alpha0 = d->p.alpha, mu0 = d->p.mu;
        std::string err;
        for (int64_t j = 0; j < n_run && !rc; j++) {
            const int32_t k = run[(size_t) j];
            if (!admm_device_set_point(d->admm.get(), alpha[k], mu[k], err)) {
                set_error(err);
                rc = 10;
                break;
            }
            rc = acg_ldpc_mc_run_impl(d, cfg, &res[k]);  // (synchronises the stream before it returns)
        }
        const std::string first_err = rc ? last_error() : std::string();
        if (!admm_device_set_point(d->admm.get(), alpha0, mu0, err) && !rc) {
            set_error(err);
            rc = 10;
        } else if (rc) {
            set_error(first_err);
        }
    }
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int32_t k = 0; k < n_points; k++) res[k].time_sec = wall;
    return rc;
}

extern "C" int acg_ldpc_mc_run_grid(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, const double *alpha, const double *mu, int32_t n_points,
                                    acg_ldpc_mc_result *res) {
    return guarded([&] { return acg_ldpc_mc_run_grid_impl(d, cfg, alpha, mu, n_points, res); });
}

// ---------------------------------------------------------------- Monte-Carlo over a grid of quantisers
// The fixed-point layered min-sum engine's counterpart of the parameter grid above: mc_points, with bp_layered_q_kernel's grid
// form reading point k's quantiser from row k of a 32-byte-per-point device table.  The table of the whole call is written
// once; a chunk's launch points at its first row.  No guard points: every quantiser is checked before anything is launched.
// The arguments are checked before the handle is read.
static int acg_ldpc_mc_run_quants_impl(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, const acg_ldpc_quant *quants, int32_t n_points,
                                       acg_ldpc_mc_result *res) {
    if (!d || !cfg || !quants || !res) {
        set_error("null argument");
        return 1;
    }
    if (n_points < 1) {
        set_error("acg_ldpc_mc_run_quants: n_points must be >= 1");
        return 1;
    }
    if (d->streamq) {
        set_error("acg_ldpc_mc_run_quants: the streamed quantized engine has no grid form (use a decoder of acg_ldpc_decoder_create_quantized)");
        return 3;
    }
    if (d->layered_wg != acg_ldpc_decoder::LayeredWg::q || !d->kernel_qgrid) {
        set_error("acg_ldpc_mc_run_quants needs a decoder of acg_ldpc_decoder_create_quantized");
        return 3;
    }
    if (check_mc_cfg(cfg)) return 1;
    for (int32_t k = 0; k < n_points; k++)
        if (int rc = acg_ldpc_quant_check(&quants[k])) {
            set_error("acg_ldpc_mc_run_quants: quants[" + std::to_string(k) + "]: " + last_error());
            return rc;
        }
    const auto t0 = std::chrono::steady_clock::now();
    std::memset(res, 0, sizeof(*res) * (size_t) n_points);
    if (cfg->frames == 0) return 0;
    std::lock_guard<std::recursive_mutex> lk(d->mu);
    HIP_OK(hipSetDevice(d->device));
    const int host = cfg->noise == ACG_LDPC_NOISE_HOST_MT19937 ? 1 : 0;
    constexpr size_t ROW = 8 * sizeof(int32_t);   // inv_step ... offset: QuantArgs without the two pointers of the integer entrance
    static_assert(offsetof(QuantArgs, c_in) == ROW, "the quantiser table holds the head of QuantArgs");
    std::vector<unsigned char> tab_h((size_t) n_points * ROW);
    for (int32_t k = 0; k < n_points; k++) {
        const QuantArgs qa = quant_args(quants[k]);
        std::memcpy(&tab_h[(size_t) k * ROW], &qa, ROW);
    }
    if (int rc = d->grid_tab.reserve(tab_h.size())) return rc;
    // (the stream is idle: every call on this handle ends with a synchronisation, so the table may be rewritten)
    HIP_OK(hipMemcpy(d->grid_tab.p, tab_h.data(), tab_h.size(), hipMemcpyHostToDevice));
    // a counter row per point, row k into res[k]; the budget stays within the kernel's 32-bit virtual frame
    const PointsRun pr{std::min<int64_t>(mc_grid_budget(), ((int64_t) 1 << 30) - 1), n_points, n_points, nullptr, nullptr, nullptr};
    std::vector<unsigned long long> h;
    auto decode = [&](int64_t c0, int64_t np, int64_t fc, Chunk &c) {
        const QuantGridArgs g{d->grid_tab.as<const int32_t>() + (size_t) c0 * 8, (uint32_t) fc};
        return decode_chunk(d, d->st_y.p, host, np * fc, cfg->snr, c, &g);
    };
    if (int rc = mc_points(d, cfg, pr, res, h, [](int64_t, int64_t, unsigned long long *) { return 0; }, decode)) return rc;
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (int32_t k = 0; k < n_points; k++) res[k].time_sec = wall;
    return 0;
}

extern "C" int acg_ldpc_mc_run_quants(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, const acg_ldpc_quant *quants, int32_t n_points,
                                      acg_ldpc_mc_result *res) {
    return guarded([&] { return acg_ldpc_mc_run_quants_impl(d, cfg, quants, n_points, res); });
}

// ---------------------------------------------------------------- Monte-Carlo through a cascade
// The unfused route, chunk by chunk, a Monte-Carlo chunk being one chunk of the cascade's device path (cascade_chunk_dev): noise
// (AWGN kernel, or transmit_host and a copy) -> stage 0 -> classification into row `first` -> select / gather / stage 1 / scatter
// -> classification of the merged outputs into row `total`.  The frames of stage 1 had ok = 0 after stage 0 and so count as
// neither correct nor pseudo in `first`: second_correct and second_pseudo are the differences of the two rows.  The sweeps of
// stage 1 are summed from its compact outputs (cascade_sum_iters_launch) into the word behind the two rows.
static int cascade_mc_run_impl(acg_ldpc_cascade *c, const acg_ldpc_mc_cfg *cfg, acg_ldpc_cascade_result *res) {
    if (!c || !cfg || !res) {
        set_error("null argument");
        return 1;
    }
    if (check_mc_cfg(cfg)) return 1;
    std::memset(res, 0, sizeof(*res));
    const auto t0 = std::chrono::steady_clock::now();
    acg_ldpc_decoder *d0 = c->stage[0].get(), *d1 = c->stage[1].get();
    std::lock_guard<std::mutex> lk(c->mu);
    std::lock_guard<std::recursive_mutex> lk0(d0->mu);
    std::lock_guard<std::recursive_mutex> lk1(d1->mu);
    const int n = d0->c.n, nwords = (n + 31) / 32;
    const int host = cfg->noise == ACG_LDPC_NOISE_HOST_MT19937 ? 1 : 0;
    const size_t row = (size_t) n * (host ? sizeof(double) : sizeof(float));
    const int64_t chunk = cascade_chunk_frames(cfg->frames, row);
    cascade_begin(c, chunk);
    if (cfg->frames == 0) return 0;
    HIP_OK(hipSetDevice(c->device));
    int rc = 0;
    if ((rc = ensure_codewords(d0, cfg))) return rc;
    if ((rc = cascade_ensure(c, chunk, row))) return rc;
    const size_t fcap = (size_t) chunk;
    if ((rc = c->mc_y.reserve(fcap * row)) || (rc = c->mc_bits.reserve(fcap * nwords * sizeof(uint32_t))) || (rc = c->mc_ok.reserve(fcap)) ||
        (rc = c->mc_iters.reserve(fcap * sizeof(int32_t))))
        return rc;
    constexpr size_t NC = 2 * MC_NCOUNTERS + 1;
    if ((rc = c->mc_counters.reserve(NC * sizeof(unsigned long long)))) return rc;
    unsigned long long *counters = c->mc_counters.as<unsigned long long>();
    hipStream_t s = d0->stream;
    HIP_OK(hipMemsetAsync(counters, 0, NC * sizeof(unsigned long long), s));
    // QP-ADMM's flag is not IsCodeword (qp_admm.h:177): its frames are classified with the CSR walk.  Row `first` as
    // acg_ldpc_mc_run classifies for stage 0; row `total` with the walk where either stage needs it (a word BP returned with
    // ok = 1 passes it by definition)
    const int32_t *row0 = nullptr, *col0 = nullptr, *row1 = nullptr, *col1 = nullptr;
    if (d0->admm) (void) admm_device_unfused_mc(d0->admm.get(), &row0, &col0);
    if (d1->admm) (void) admm_device_unfused_mc(d1->admm.get(), &row1, &col1);
    const int32_t *rowt = row0 ? row0 : row1, *colt = row0 ? col0 : col1;
    const SentWords cw = sent_words(d0, cfg);
    uint32_t *bits = c->mc_bits.as<uint32_t>();
    uint8_t *ok = c->mc_ok.as<uint8_t>();
    int32_t *iters = c->mc_iters.as<int32_t>();
    std::vector<double> yh;
    for (int64_t f0 = 0; f0 < cfg->frames; f0 += chunk) {
        const int64_t fc = std::min(chunk, cfg->frames - f0), first = cfg->first_frame + f0;
        if ((rc = mc_symbols(d0, cfg, first, fc, c->mc_y.p, s, yh))) return rc;
        CascadeHooks hooks;
        hooks.first_done = [&] {
            HIP_OK(classify_grid_launch(c->mc_y.p, host, bits, ok, iters, fc, 1, n, nwords, first, cw.dev, cw.n, counters, row0, col0, d0->c.m, s));
            return 0;
        };
        hooks.second_done = [&](int64_t K) {
            HIP_OK(cascade_sum_iters_launch(c->c_iters.as<int32_t>(), (int32_t) K, counters + 2 * MC_NCOUNTERS, s));
            return 0;
        };
        if ((rc = cascade_chunk_dev(c, c->mc_y.p, host, fc, cfg->snr, bits, ok, iters, nullptr, s, &hooks))) return rc;
        HIP_OK(classify_grid_launch(c->mc_y.p, host, bits, ok, iters, fc, 1, n, nwords, first, cw.dev, cw.n, counters + MC_NCOUNTERS, rowt, colt,
                                    d0->c.m, s));
        HIP_OK(hipStreamSynchronize(s));   // (the chunk's buffers and yh are rewritten by the next one)
        if ((rc = cascade_settle(c))) return rc;
    }
    unsigned long long h[NC];
    HIP_OK(hipMemcpy(h, counters, sizeof(h), hipMemcpyDeviceToHost));
    counters_to_result(h, &res->first);
    counters_to_result(h + MC_NCOUNTERS, &res->total);
    res->second_frames = c->last_second;
    res->second_correct = res->total.correct - res->first.correct;
    res->second_pseudo = res->total.pseudo - res->first.pseudo;
    res->second_sum_iters = (int64_t) h[2 * MC_NCOUNTERS];
    res->first.kernel_ms = c->last_ms[0];
    res->second_kernel_ms = c->last_ms[1];
    res->total.kernel_ms = (double) c->last_ms[0] + (double) c->last_ms[1];
    res->total.time_sec = res->first.time_sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

extern "C" int acg_ldpc_cascade_mc_run(acg_ldpc_cascade *c, const acg_ldpc_mc_cfg *cfg, acg_ldpc_cascade_result *res) {
    return guarded([&] { return cascade_mc_run_impl(c, cfg, res); });
}

extern "C" void acg_ldpc_cascade_merge(acg_ldpc_cascade_result *a, const acg_ldpc_cascade_result *b) {
    acg_ldpc_mc_merge(&a->total, &b->total);
    acg_ldpc_mc_merge(&a->first, &b->first);
    a->second_frames += b->second_frames;
    a->second_correct += b->second_correct;
    a->second_pseudo += b->second_pseudo;
    a->second_sum_iters += b->second_sum_iters;
    a->second_kernel_ms += b->second_kernel_ms;
}

static int acg_ldpc_awgn_dev_impl(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, float *y_dev, void *stream) {
    if (!d || !cfg || !y_dev) {
        set_error("null argument");
        return 1;
    }
    std::lock_guard<std::recursive_mutex> lk(d->mu);
    HIP_OK(hipSetDevice(d->device));
    if (int rc = ensure_codewords(d, cfg)) return rc;
    return awgn_frames(d, cfg, cfg->first_frame, cfg->frames, y_dev, stream ? (hipStream_t) stream : d->stream);
}

extern "C" int acg_ldpc_awgn_dev(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, float *y_dev, void *stream) {
    return guarded([&] { return acg_ldpc_awgn_dev_impl(d, cfg, y_dev, stream); });
}

// ---------------------------------------------------------------- Monte-Carlo for punctured and shortened codes
// What the two calls refuse, in the order the header states; `sink` is res or out_dev.  0: the handle takes channel values.
static int rm_check(const acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, const uint8_t *pattern, const void *sink, const char *call) {
    if (!d || !cfg || !sink) {
        set_error("null argument");
        return 1;
    }
    if (check_mc_cfg(cfg)) return 1;
    if (cfg->noise == ACG_LDPC_NOISE_HOST_MT19937) {
        set_error(std::string(call) + ": device noise only (ACG_LDPC_NOISE_DEVICE_PHILOX)");
        return 1;
    }
    for (int v = 0; pattern && v < d->c.n; v++)
        if (pattern[v] > ACG_LDPC_RM_SHORTENED) {
            set_error(std::string(call) + ": pattern[" + std::to_string(v) + "] = " + std::to_string((int) pattern[v]) +
                      " is not ACG_LDPC_RM_SENT, _PUNCTURED or _SHORTENED");
            return 1;
        }
    if (!d->streaml && d->layered_wg != acg_ldpc_decoder::LayeredWg::q) {
        set_error(std::string(call) + " needs a decoder of acg_ldpc_decoder_create_layered_streamed, acg_ldpc_decoder_create_quantized or "
                  "acg_ldpc_decoder_create_quantized_streamed");
        return 3;
    }
    return 0;
}

// the pattern of this call into the handle's copy -> its device address, null for an all-sent run.  s: the stream the
// generator is about to run on — what it still holds may read the previous pattern, so it is waited for first (calls on
// different streams of the caller's are the caller's to order, as for the codewords).  Caller holds d->mu.
static int rm_pattern_dev(acg_ldpc_decoder *d, const uint8_t *pattern, hipStream_t s, const uint8_t **out) {
    *out = nullptr;
    if (!pattern) return 0;
    if (d->rm_pattern.p) HIP_OK(hipStreamSynchronize(s));
    if (int rc = d->rm_pattern.reserve((size_t) (d->c.n + 3) & ~(size_t) 3)) return rc;
    HIP_OK(hipMemcpy(d->rm_pattern.p, pattern, (size_t) d->c.n, hipMemcpyHostToDevice));
    *out = d->rm_pattern.as<uint8_t>();
    return 0;
}

// the generator launch of frames [first, first + fc) of cfg on stream s
static int rm_channel(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, const uint8_t *pat_dev, int64_t first, int64_t fc, void *out,
                      int32_t *raw, hipStream_t s) {
    const SentWords cw = sent_words(d, cfg);
    const double var = acg_ldpc_llr_variance(cfg->snr);
    HIP_OK(rm_channel_launch(out, d->streaml ? nullptr : &d->qargs, raw, fc, d->c.n, (d->c.n + 31) / 32, first, cfg->seed, cw.dev, cw.n,
                             (float) channel_sigma(cfg->snr), 2.0 / var, pat_dev, s));
    return 0;
}

static int acg_ldpc_rm_channel_dev_impl(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, const uint8_t *pattern, void *out_dev,
                                        int32_t *raw_dev, void *stream) {
    if (int rc = rm_check(d, cfg, pattern, out_dev, "acg_ldpc_rm_channel_dev")) return rc;
    if (cfg->frames == 0) return 0;
    std::lock_guard<std::recursive_mutex> lk(d->mu);
    HIP_OK(hipSetDevice(d->device));
    if (int rc = ensure_codewords(d, cfg)) return rc;
    const hipStream_t s = stream ? (hipStream_t) stream : d->stream;
    const uint8_t *pat_dev = nullptr;
    if (int rc = rm_pattern_dev(d, pattern, s, &pat_dev)) return rc;
    return rm_channel(d, cfg, pat_dev, cfg->first_frame, cfg->frames, out_dev, raw_dev, s);
}

extern "C" int acg_ldpc_rm_channel_dev(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, const uint8_t *pattern, void *out_dev, int32_t *raw_dev,
                                       void *stream) {
    return guarded([&] { return acg_ldpc_rm_channel_dev_impl(d, cfg, pattern, out_dev, raw_dev, stream); });
}

// mc_frames, a chunk being rm_channel_kernel (channel values into mc_y, raw-error counts) -> the handle's channel-value
// entrance on its ordinary launch path -> classify_rm_kernel.
static int acg_ldpc_mc_run_rm_impl(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, const uint8_t *pattern, acg_ldpc_mc_result *res) {
    if (int rc = rm_check(d, cfg, pattern, res, "acg_ldpc_mc_run_rm")) return rc;
    std::memset(res, 0, sizeof(*res));
    const auto t0 = std::chrono::steady_clock::now();
    const int n = d->c.n, nwords = (n + 31) / 32;
    const uint8_t *pat_dev = nullptr;
    auto prepare = [&](int64_t rows) {
        if (int e = rm_pattern_dev(d, pattern, d->stream, &pat_dev)) return e;
        return d->rm_raw.reserve((size_t) rows * sizeof(int32_t));
    };
    auto enqueue = [&](int64_t first, int64_t fc, Chunk &c) {
        int32_t *raw = d->rm_raw.as<int32_t>();
        if (int e = rm_channel(d, cfg, pat_dev, first, fc, d->mc_y.p, raw, d->stream)) return e;
        const QuantIo qio{d->mc_y.as<int16_t>(), nullptr};
        const StreamLayIo lio{d->mc_y.as<float>(), nullptr};
        // (no symbols, no channel: the channel-value entrances read neither)
        if (int e = decode_chunk(d, nullptr, 0, fc, 0.0, c, d->streaml ? DecodeIo(&lio) : DecodeIo(&qio))) return e;
        const SentWords cw = sent_words(d, cfg);
        HIP_OK(classify_rm_launch(raw, c.a.out_bits, c.a.out_ok, c.a.out_iters, fc, n, nwords, first, cw.dev, cw.n, d->counters_dev(), d->stream));
        return 0;
    };
    if (int rc = mc_frames(d, cfg, d->streaml ? sizeof(float) : sizeof(int16_t), "ACG_MC_RM_CHUNK", res, true, prepare, enqueue, no_chunk_work)) return rc;
    res->time_sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

extern "C" int acg_ldpc_mc_run_rm(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, const uint8_t *pattern, acg_ldpc_mc_result *res) {
    return guarded([&] { return acg_ldpc_mc_run_rm_impl(d, cfg, pattern, res); });
}

// ---------------------------------------------------------------- host generators
static int acg_ldpc_gen_codewords_impl(const uint8_t *G, int32_t k, int32_t n, uint32_t seed, int64_t count, uint8_t *out) {
    if (!G || !out || k <= 0 || n <= 0 || count < 0) {
        set_error("bad argument");
        return 1;
    }
    std::mt19937 rnd(seed);  // main.cpp:63
    for (int64_t f = 0; f < count; f++) {
        uint8_t *res = out + (size_t) f * n;
        std::memset(res, 0, (size_t) n);
        for (int i = 0; i < k; i++)
            if (rnd() % 2 == 0) {  // channel.h:33
                const uint8_t *row = G + (size_t) i * n;
                for (int j = 0; j < n; j++) res[j] ^= (row[j] ? 1 : 0);
            }
    }
    return 0;
}

extern "C" int acg_ldpc_gen_codewords(const uint8_t *G, int32_t k, int32_t n, uint32_t seed, int64_t count, uint8_t *out) {
    return guarded([&] { return acg_ldpc_gen_codewords_impl(G, k, n, seed, count, out); });
}

static int acg_ldpc_transmit_host_impl(const uint8_t *codewords, int64_t n_codewords, int32_t n, int64_t first_frame,
                           int64_t frames, double snr, double *y) {
    if (!y || n <= 0 || frames < 0 || (codewords && n_codewords <= 0)) {
        set_error("bad argument");
        return 1;
    }
    transmit_host(codewords, n_codewords, n, first_frame, frames, snr, y);
    return 0;
}

extern "C" int acg_ldpc_transmit_host(const uint8_t *codewords, int64_t n_codewords, int32_t n, int64_t first_frame,
                                      int64_t frames, double snr, double *y) {
    return guarded([&] { return acg_ldpc_transmit_host_impl(codewords, n_codewords, n, first_frame, frames, snr, y); });
}

