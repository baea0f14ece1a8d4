// acg_ldpc_decoder.hpp — C++ mirror of the reference's Decoder operator interface over the C ABI.
//
// Same class names, constructor arguments, decode() signature and return convention as the reference:
//   class Decoder                          algo/algo.h:6-11
//   class BeliefPropagationDecoder(int)    algo/bp.h:208-222      name() == "BP"
//   class QPADMMDecoder(a, mu, it, eps)    algo/qp_admm.h:180-194 name() == "QP-ADMM"
// so experiment.h / main.cpp style callers compile unchanged against these types.  Build-added, not in the
// reference: MinSumDecoder ("MS") and QuantizedMinSumDecoder ("QMS", fixed-point layered min-sum).
// Header-only; link with -lacg_ldpc_hip.  The analysed graph is cached on the CONTENT of H, because the reference passes H
// to every call (SURVEY §8b "Inputs"); the cache is a small LRU (kMaxHandles), because the reference's optimize_H loop
// hands a NEW H per proposal to one shared decoder (optimize_H.cpp:16-25,89-104).
#pragma once

#include <algorithm>
#include <cassert>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "acg_ldpc.h"

namespace acg_ldpc {

typedef std::vector<bool> TCodeword;       // utils/codeword.h:17
typedef std::vector<TCodeword> TMatrix;    // utils/codeword.h:18
typedef std::vector<double> TFVector;      // utils/channel.h:8

class Decoder {  // algo/algo.h:6-11
public:
    virtual ~Decoder() {}
    virtual std::pair<TCodeword, bool> decode(const TMatrix &H, const TFVector &channel_word, double snr) = 0;
    virtual std::string name() const = 0;
};

class HipDecoderBase : public Decoder {
public:
    // live device handles per decoder object: least recently used ones beyond this are destroyed
    static constexpr size_t kMaxHandles = 8;

    ~HipDecoderBase() override {
        for (auto &e : cache_) drop(e);
    }

    std::pair<TCodeword, bool> decode(const TMatrix &H, const TFVector &channel_word, double snr) override {
        // the handle stays checked out for the duration of the call, so a concurrent decode() with another H (the
        // reference calls one decoder object from THREADS_NUM pthreads, experiment.h:101) cannot evict it under us
        Lease l(this, H);
        const int n = (int) H[0].size();
        assert((int) channel_word.size() == n);
        std::vector<uint8_t> bits((size_t) n);
        uint8_t ok = 0;
        int rc = acg_ldpc_decode_batch(l.dec(), channel_word.data(), 1, snr, bits.data(), &ok, nullptr);
        check(rc);
        return finish(bits, ok != 0);
    }

    // batched form: Y is frames*n doubles; returns per-frame (word, flag) exactly as decode() would
    std::vector<std::pair<TCodeword, bool>> decode_batch(const TMatrix &H, const std::vector<double> &Y, double snr) {
        Lease l(this, H);
        const int n = (int) H[0].size();
        const int64_t frames = (int64_t) (Y.size() / (size_t) n);
        std::vector<uint8_t> bits((size_t) frames * n), ok((size_t) frames);
        check(acg_ldpc_decode_batch(l.dec(), Y.data(), frames, snr, bits.data(), ok.data(), nullptr));
        std::vector<std::pair<TCodeword, bool>> out;
        out.reserve((size_t) frames);
        for (int64_t f = 0; f < frames; f++)
            out.push_back(finish(std::vector<uint8_t>(bits.begin() + f * n, bits.begin() + (f + 1) * n), ok[f] != 0));
        return out;
    }

    // the C handle for Monte-Carlo runs (acg_ldpc_mc_run).  The reference hands H to every decode() and re-analyses it
    // (bp.h:136-153, qp_admm.h:15-21); here the analysed graph is cached on the CONTENT of H (hash of the packed words of
    // vector<bool> + a full compare of the packed copy on a hit), so a matrix that is modified or whose storage is recycled
    // can never meet a stale handle.  The returned pointer stays valid until kMaxHandles OTHER matrices have been used
    // through this object; decode() / decode_batch() pin theirs for the duration of the call.
    acg_ldpc_decoder *handle(const TMatrix &H) {
        std::lock_guard<std::mutex> lk(mu_);
        return lookup(H)->dec;
    }

    // acg_ldpc_mc_run_detail (the classification of experiment.h:109-120, extended): the counters of a Monte-Carlo run plus
    // the bit errors of the returned words and the first `cap` frames that are not correct, in ascending global frame order.
    // words[k] (only when want_words) = returned word XOR sent word of events[k], (n+31)/32 packed words per row.
    struct McDetail {
        acg_ldpc_mc_detail d;
        int64_t cap = 0;
        int n = 0;
        std::vector<acg_ldpc_mc_event> events;
        std::vector<uint32_t> words;
        double BER() const { return (double) d.bit_errors / ((double) d.base.total * n); }  // over returned words, see acg_ldpc.h
    };
    McDetail run_detail(const TMatrix &H, const acg_ldpc_mc_cfg &cfg, int64_t cap, bool want_words = false) {
        Lease l(this, H);
        McDetail o;
        o.cap = cap;
        o.n = (int) H[0].size();
        const size_t nwords = (size_t) (o.n + 31) / 32;
        o.events.resize((size_t) cap);
        if (want_words) o.words.resize((size_t) cap * nwords);
        check(acg_ldpc_mc_run_detail(l.dec(), &cfg, &o.d, cap ? o.events.data() : nullptr, want_words && cap ? o.words.data() : nullptr, cap));
        o.events.resize((size_t) o.d.n_stored);
        if (want_words) o.words.resize((size_t) o.d.n_stored * nwords);
        return o;
    }
    // shards: acg_ldpc_mc_detail_merge for the counters; the event lists concatenated, sorted by frame, cut to a.cap
    static void merge_details(McDetail &a, const McDetail &b) {
        acg_ldpc_mc_detail_merge(&a.d, &b.d);
        const size_t nwords = (size_t) (a.n + 31) / 32, na = a.events.size(), nb = b.events.size();
        const bool w = a.words.size() == na * nwords && b.words.size() == nb * nwords;
        std::vector<acg_ldpc_mc_event> ev(a.events);
        ev.insert(ev.end(), b.events.begin(), b.events.end());
        std::vector<size_t> order(ev.size());
        for (size_t i = 0; i < order.size(); i++) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return ev[x].frame < ev[y].frame; });
        if (order.size() > (size_t) a.cap) order.resize((size_t) a.cap);
        std::vector<uint32_t> words;
        a.events.clear();
        for (size_t i : order) {
            a.events.push_back(ev[i]);
            if (w) {
                const uint32_t *row = i < na ? a.words.data() + i * nwords : b.words.data() + (i - na) * nwords;
                words.insert(words.end(), row, row + nwords);
            }
        }
        a.words.swap(words);
        a.d.n_stored = (int64_t) a.events.size();
    }

    size_t live_handles() const {
        std::lock_guard<std::mutex> lk(mu_);
        return cache_.size();
    }

protected:
    virtual void fill(acg_ldpc_params &p) const = 0;
    virtual std::pair<TCodeword, bool> finish(const std::vector<uint8_t> &bits, bool ok) const = 0;
    // the create call of the C ABI this class's handles come from
    virtual int create(const acg_ldpc_code *code, const acg_ldpc_params &p, acg_ldpc_decoder **out) const {
        return acg_ldpc_decoder_create(code, &p, out);
    }

    static void check(int rc) {
        if (rc != 0) {  // the reference aborts through assert(); so does the adaptor, with the library's message
            std::fprintf(stderr, "acg_ldpc: error %d: %s\n", rc, acg_ldpc_last_error());
            std::abort();
        }
    }

    // f(handle for H), the handle pinned for the duration of the call as decode() pins its own
    template <class F>
    void with_handle(const TMatrix &H, F &&f) {
        Lease l(this, H);
        f(l.dec());
    }

private:
    struct Entry {
        int m = 0, n = 0;
        uint64_t h = 0;
        std::vector<uint64_t> packed;  // row-major, every row padded to whole 64-bit words
        acg_ldpc_code *code = nullptr;
        acg_ldpc_decoder *dec = nullptr;
        int pins = 0;                  // decode() calls in flight on this handle
    };
    typedef std::list<Entry>::iterator It;

    struct Lease {  // keeps one entry out of the eviction's reach while a call uses its handle
        Lease(HipDecoderBase *o, const TMatrix &H) : o_(o) {
            std::lock_guard<std::mutex> lk(o_->mu_);
            it_ = o_->lookup(H);
            it_->pins++;
        }
        ~Lease() {
            std::lock_guard<std::mutex> lk(o_->mu_);
            it_->pins--;
            o_->trim();
        }
        acg_ldpc_decoder *dec() const { return it_->dec; }
        HipDecoderBase *o_;
        It it_;
    };

    static void pack(const TMatrix &H, int m, int n, std::vector<uint64_t> &out, uint64_t &h) {
        const int wpr = (n + 63) / 64;
        out.assign((size_t) m * wpr, 0);
        h = 1469598103934665603ull;
        for (int i = 0; i < m; i++) {
            uint64_t *row = out.data() + (size_t) i * wpr;
#if defined(__GLIBCXX__)
            // whole 64-bit words of the row, then the tail bits (bits beyond size() in the last word are unspecified)
            static_assert(sizeof(unsigned long) == 8, "packed copy assumes 64-bit words");
            const unsigned long *wp = H[i].begin()._M_p;
            const int full = n / 64;
            for (int w = 0; w < full; w++) row[w] = (uint64_t) wp[w];
            for (int j = full * 64; j < n; j++) row[j >> 6] |= (uint64_t) H[i][j] << (j & 63);
#else
            for (int j = 0; j < n; j++) row[j >> 6] |= (uint64_t) H[i][j] << (j & 63);
#endif
            for (int w = 0; w < wpr; w++) h = (h ^ row[w]) * 1099511628211ull;
            h = (h ^ 0x9E3779B97F4A7C15ull) * 1099511628211ull;  // row separator
        }
    }

    // caller holds mu_.  Hit: move to the front.  Miss: analyse H, create the device handle, evict beyond kMaxHandles.
    It lookup(const TMatrix &H) {
        const int m = (int) H.size(), n = (int) H[0].size();
        pack(H, m, n, scratch_, scratch_h_);
        for (It it = cache_.begin(); it != cache_.end(); ++it)
            if (it->m == m && it->n == n && it->h == scratch_h_ && it->packed == scratch_) {
                cache_.splice(cache_.begin(), cache_, it);
                return cache_.begin();
            }
        std::vector<uint8_t> dense((size_t) m * n);
        for (int i = 0; i < m; i++)
            for (int j = 0; j < n; j++) dense[(size_t) i * n + j] = H[i][j];
        Entry e;
        e.m = m;
        e.n = n;
        e.h = scratch_h_;
        e.packed = scratch_;
        check(acg_ldpc_code_from_dense(dense.data(), m, n, &e.code));
        acg_ldpc_params p;
        acg_ldpc_params_default(&p);
        fill(p);
        check(create(e.code, p, &e.dec));
        cache_.push_front(e);
        trim();
        return cache_.begin();
    }

    void trim() {  // caller holds mu_: drop least recently used entries that no call is using
        for (It it = cache_.end(); cache_.size() > kMaxHandles && it != cache_.begin();) {
            --it;
            if (it->pins == 0 && it != cache_.begin()) {
                drop(*it);
                it = cache_.erase(it);
            }
        }
    }

    static void drop(Entry &e) {
        acg_ldpc_decoder_destroy(e.dec);
        acg_ldpc_code_destroy(e.code);
        e.dec = nullptr;
        e.code = nullptr;
    }

    std::list<Entry> cache_;
    std::vector<uint64_t> scratch_;
    uint64_t scratch_h_ = 0;
    mutable std::mutex mu_;
};

// algo/bp.h:208-222
class BeliefPropagationDecoder : public HipDecoderBase {
public:
    // layered (build-added, default off = the reference's flooding schedule, bit-exact hard decisions): the same check rule with the
    // posteriors updated per block row — the reference's FER at about half the iterations, FER-level parity only
    // lanes_per_frame: acg_ldpc_params::lanes_per_frame (with layered, 256 / 512 / 1024 = the engine with one workgroup per frame)
    explicit BeliefPropagationDecoder(int max_iter, bool layered = false, int lanes_per_frame = 0)
        : _max_iter(max_iter), _layered(layered), _lanes(lanes_per_frame) {}
    std::string name() const override { return "BP"; }  // bp.h:218

protected:
    void fill(acg_ldpc_params &p) const override {
        p.algo = ACG_LDPC_BP_SUMPRODUCT;
        p.max_iter = _max_iter;
        p.schedule = _layered ? ACG_LDPC_SCHEDULE_LAYERED : ACG_LDPC_SCHEDULE_FLOODING;
        p.lanes_per_frame = _lanes;
    }
    std::pair<TCodeword, bool> finish(const std::vector<uint8_t> &bits, bool ok) const override {
        if (!ok) return {TCodeword(), false};  // bp.h:198
        return {TCodeword(bits.begin(), bits.end()), true};
    }

private:
    int _max_iter;
    bool _layered;
    int _lanes;
};

// algo/qp_admm.h:180-194 (same defaults)
class QPADMMDecoder : public HipDecoderBase {
public:
    explicit QPADMMDecoder(double alpha, double mu, int max_iter = 2000, double eps_stop = 1e-5)
        : _alpha(alpha), _mu(mu), _eps_stop(eps_stop), _max_iter(max_iter) {}
    std::string name() const override { return "QP-ADMM"; }  // qp_admm.h:189

protected:
    void fill(acg_ldpc_params &p) const override {
        p.algo = ACG_LDPC_QPADMM;
        p.max_iter = _max_iter;
        p.alpha = _alpha;
        p.mu = _mu;
        p.eps_stop = _eps_stop;
    }
    std::pair<TCodeword, bool> finish(const std::vector<uint8_t> &bits, bool ok) const override {
        return {TCodeword(bits.begin(), bits.end()), ok};  // qp_admm.h:112-114 (zeros,false) / :177 (word,true)
    }

private:
    double _alpha, _mu, _eps_stop;
    int _max_iter;
};

// build-added (north_star); not in the reference: parity unpinned.  layered = true: ACG_LDPC_SCHEDULE_LAYERED (about half the
// iterations for the same FER; FER-level parity only)
class MinSumDecoder : public HipDecoderBase {
public:
    explicit MinSumDecoder(int max_iter, double scale = 1.0, bool layered = false, int lanes_per_frame = 0)
        : _max_iter(max_iter), _scale(scale), _layered(layered), _lanes(lanes_per_frame) {}
    std::string name() const override { return "MS"; }

protected:
    void fill(acg_ldpc_params &p) const override {
        p.algo = ACG_LDPC_BP_MINSUM;
        p.max_iter = _max_iter;
        p.ms_scale = _scale;
        p.schedule = _layered ? ACG_LDPC_SCHEDULE_LAYERED : ACG_LDPC_SCHEDULE_FLOODING;
        p.lanes_per_frame = _lanes;
    }
    std::pair<TCodeword, bool> finish(const std::vector<uint8_t> &bits, bool ok) const override {
        if (!ok) return {TCodeword(), false};
        return {TCodeword(bits.begin(), bits.end()), true};
    }

private:
    int _max_iter;
    double _scale;
    bool _layered;
    int _lanes;
};

// build-added; not in the reference.  Layered sum-product and min-sum with fp32 posteriors and messages in device memory
// (acg_ldpc_decoder_create_layered_streamed): any code size, any check degree; word and flag of every frame equal those of
// BeliefPropagationDecoder(max_iter, true, 256) / MinSumDecoder(max_iter, scale, true, 256) on every code both accept.  A code
// whose frame fits in LDS is decoded faster by those.

// what the two classes below add to their flooding-or-layered base: the create call, and the LLR entrance (acg_ldpc.h:
// acg_ldpc_decode_batch_llr*) — LLRs in, posterior LLRs out
template <class Base>
class StreamedLayeredIo : public Base {
public:
    using Base::Base;
    struct LlrResult {
        std::vector<uint8_t> bits, ok;   // frames*n bytes (zeros for a failed frame), frames flags
        std::vector<int32_t> iters;      // frames
        std::vector<float> post;         // frames*n posterior LLRs (natural-log units; the sign bit is the bit); empty when not asked for
    };
    // L: frames*n LLRs, positive = bit 0 (NaN counts as 0, every value is clamped to +-2^20; punctured = 0, shortened = +-2^20)
    LlrResult decode_llr_batch(const TMatrix &H, const std::vector<float> &L, bool posteriors = true) {
        const size_t n = H[0].size(), frames = L.size() / n;
        LlrResult r;
        r.bits.resize(frames * n);
        r.ok.resize(frames);
        r.iters.resize(frames);
        if (posteriors) r.post.resize(frames * n);
        this->with_handle(H, [&](acg_ldpc_decoder *d) {
            Base::check(acg_ldpc_decode_batch_llr(d, L.data(), (int64_t) frames, r.bits.data(), r.ok.data(), r.iters.data(),
                                                  posteriors ? r.post.data() : nullptr));
        });
        return r;
    }
    // device buffers, asynchronous on `stream` (null: the handle's own)
    void decode_llr_batch_dev(const TMatrix &H, const float *llr_dev, int64_t frames, uint32_t *bits_dev, uint8_t *ok_dev,
                              int32_t *iters_dev = nullptr, float *post_dev = nullptr, void *stream = nullptr) {
        this->with_handle(H, [&](acg_ldpc_decoder *d) {
            Base::check(acg_ldpc_decode_batch_llr_dev(d, llr_dev, frames, bits_dev, ok_dev, iters_dev, post_dev, stream));
        });
    }
    // acg_ldpc_mc_run_rm: a Monte-Carlo run of a punctured / shortened code.  pattern: n bytes of ACG_LDPC_RM_*, empty = all sent
    acg_ldpc_mc_result run_rate_matched(const TMatrix &H, const acg_ldpc_mc_cfg &cfg, const std::vector<uint8_t> &pattern = {}) {
        acg_ldpc_mc_result r{};
        this->with_handle(H, [&](acg_ldpc_decoder *d) {
            assert(pattern.empty() || pattern.size() == H[0].size());
            Base::check(acg_ldpc_mc_run_rm(d, &cfg, pattern.empty() ? nullptr : pattern.data(), &r));
        });
        return r;
    }

protected:
    int create(const acg_ldpc_code *code, const acg_ldpc_params &p, acg_ldpc_decoder **out) const override {
        return acg_ldpc_decoder_create_layered_streamed(code, &p, out);
    }
};

class StreamedLayeredBPDecoder : public StreamedLayeredIo<BeliefPropagationDecoder> {
public:
    explicit StreamedLayeredBPDecoder(int max_iter) : StreamedLayeredIo<BeliefPropagationDecoder>(max_iter, true, 0) {}
};

class StreamedLayeredMinSumDecoder : public StreamedLayeredIo<MinSumDecoder> {
public:
    explicit StreamedLayeredMinSumDecoder(int max_iter, double scale = 1.0) : StreamedLayeredIo<MinSumDecoder>(max_iter, scale, true, 0) {}
};

// build-added; not in the reference.  Fixed-point layered min-sum (acg_ldpc_decoder_create_quantized): integer channel values,
// messages and posteriors as *quant says; the default quantiser is offset-1 min-sum on a 6-bit channel.  name() == "QMS".
class QuantizedMinSumDecoder : public HipDecoderBase {
public:
    static acg_ldpc_quant default_quant() {
        acg_ldpc_quant q;
        acg_ldpc_quant_default(&q);
        return q;
    }
    explicit QuantizedMinSumDecoder(int max_iter, const acg_ldpc_quant &quant = default_quant(), int lanes_per_frame = 0)
        : _max_iter(max_iter), _lanes(lanes_per_frame), _quant(quant) {}
    std::string name() const override { return "QMS"; }

    // ---- the integer entrance (acg_ldpc.h: acg_ldpc_decode_batch_q*): channel values in, posteriors out ----
    // Y: symbols -> int16 channel values, this decoder's quantiser as the symbol entrance applies it (acg_ldpc_debug_quantize)
    std::vector<int16_t> quantize(const std::vector<double> &Y, double snr) const {
        std::vector<int16_t> c(Y.size());
        check(acg_ldpc_debug_quantize(Y.data(), 1, (int64_t) Y.size(), snr, &_quant, c.data()));
        return c;
    }
    struct LlrResult {
        std::vector<uint8_t> bits, ok;   // frames*n bytes (zeros for a failed frame), frames flags
        std::vector<int32_t> iters;      // frames
        std::vector<int16_t> post;       // frames*n posteriors; empty when not asked for
    };
    // C: frames*n channel values (clamped to +-Cmax by the decoder; punctured = 0, shortened = +-Cmax)
    LlrResult decode_llr_batch(const TMatrix &H, const std::vector<int16_t> &C, bool posteriors = true) {
        const size_t n = H[0].size(), frames = C.size() / n;
        LlrResult r;
        r.bits.resize(frames * n);
        r.ok.resize(frames);
        r.iters.resize(frames);
        if (posteriors) r.post.resize(frames * n);
        with_handle(H, [&](acg_ldpc_decoder *d) {
            check(acg_ldpc_decode_batch_q(d, C.data(), (int64_t) frames, r.bits.data(), r.ok.data(), r.iters.data(),
                                          posteriors ? r.post.data() : nullptr));
        });
        return r;
    }
    // device buffers, asynchronous on `stream` (null: the handle's own)
    void decode_llr_batch_dev(const TMatrix &H, const int16_t *c_dev, int64_t frames, uint32_t *bits_dev, uint8_t *ok_dev,
                              int32_t *iters_dev = nullptr, int16_t *post_dev = nullptr, void *stream = nullptr) {
        with_handle(H, [&](acg_ldpc_decoder *d) {
            check(acg_ldpc_decode_batch_q_dev(d, c_dev, frames, bits_dev, ok_dev, iters_dev, post_dev, stream));
        });
    }
    void quantize_dev(const TMatrix &H, const void *y_dev, bool y_is_f64, int64_t count, double snr, int16_t *c_dev,
                      void *stream = nullptr) {
        with_handle(H, [&](acg_ldpc_decoder *d) { check(acg_ldpc_quantize_dev(d, y_dev, y_is_f64 ? 1 : 0, count, snr, c_dev, stream)); });
    }
    // acg_ldpc_mc_run_rm: a Monte-Carlo run of a punctured / shortened code.  pattern: n bytes of ACG_LDPC_RM_*, empty = all sent
    acg_ldpc_mc_result run_rate_matched(const TMatrix &H, const acg_ldpc_mc_cfg &cfg, const std::vector<uint8_t> &pattern = {}) {
        acg_ldpc_mc_result r{};
        with_handle(H, [&](acg_ldpc_decoder *d) {
            assert(pattern.empty() || pattern.size() == H[0].size());
            check(acg_ldpc_mc_run_rm(d, &cfg, pattern.empty() ? nullptr : pattern.data(), &r));
        });
        return r;
    }

protected:
    void fill(acg_ldpc_params &p) const override {
        p.algo = ACG_LDPC_BP_MINSUM;
        p.max_iter = _max_iter;
        p.schedule = ACG_LDPC_SCHEDULE_LAYERED;
        p.lanes_per_frame = _lanes;
    }
    int create(const acg_ldpc_code *code, const acg_ldpc_params &p, acg_ldpc_decoder **out) const override {
        return acg_ldpc_decoder_create_quantized(code, &p, &_quant, out);
    }
    std::pair<TCodeword, bool> finish(const std::vector<uint8_t> &bits, bool ok) const override {
        if (!ok) return {TCodeword(), false};
        return {TCodeword(bits.begin(), bits.end()), true};
    }

    const acg_ldpc_quant &quant() const { return _quant; }

private:
    int _max_iter, _lanes;
    acg_ldpc_quant _quant;
};

// build-added; not in the reference.  The same decoder with a frame's state in device memory
// (acg_ldpc_decoder_create_quantized_streamed): any code size, any check degree, the same results on every code both accept.
// A code whose frame fits in LDS is decoded faster by QuantizedMinSumDecoder.
class StreamedQuantizedMinSumDecoder : public QuantizedMinSumDecoder {
public:
    explicit StreamedQuantizedMinSumDecoder(int max_iter, const acg_ldpc_quant &quant = default_quant()) : QuantizedMinSumDecoder(max_iter, quant, 0) {}

protected:
    int create(const acg_ldpc_code *code, const acg_ldpc_params &p, acg_ldpc_decoder **out) const override {
        return acg_ldpc_decoder_create_quantized_streamed(code, &p, &quant(), out);
    }
};

// build-added; not in the reference.  Ordered-statistics decoding of order 0 or 1 (acg_ldpc.h, "OSD"): one GF(2) elimination per
// frame on int16 soft values, always a codeword.  decode() quantises the symbols (snr is ignored); name() == "OSD".
class OSDDecoder : public HipDecoderBase {
public:
    explicit OSDDecoder(int order = 1, int lanes_per_frame = 0) : _order(order), _lanes(lanes_per_frame) {}
    std::string name() const override { return "OSD"; }

    // Y: symbols -> the int16 soft values the symbol entrance forms (acg_ldpc_debug_osd_soft)
    static std::vector<int16_t> soft_values(const std::vector<double> &Y) {
        std::vector<int16_t> s(Y.size());
        check(acg_ldpc_debug_osd_soft(Y.data(), 1, (int64_t) Y.size(), s.data()));
        return s;
    }
    struct SoftResult {
        std::vector<uint8_t> bits, ok;   // frames*n bytes, frames flags (all 1)
        std::vector<int32_t> iters;      // frames: positions of the information set flipped, 0 or 1
    };
    // S: frames*n soft values (sign = hard decision, magnitude = reliability)
    SoftResult decode_soft_batch(const TMatrix &H, const std::vector<int16_t> &S) {
        const size_t n = H[0].size(), frames = S.size() / n;
        SoftResult r;
        r.bits.resize(frames * n);
        r.ok.resize(frames);
        r.iters.resize(frames);
        with_handle(H, [&](acg_ldpc_decoder *d) {
            check(acg_ldpc_osd_decode_batch(d, S.data(), (int64_t) frames, r.bits.data(), r.ok.data(), r.iters.data()));
        });
        return r;
    }
    // device buffers, asynchronous on `stream` (null: the handle's own)
    void decode_soft_batch_dev(const TMatrix &H, const int16_t *s_dev, int64_t frames, uint32_t *bits_dev, uint8_t *ok_dev,
                               int32_t *iters_dev = nullptr, void *stream = nullptr) {
        with_handle(H, [&](acg_ldpc_decoder *d) { check(acg_ldpc_osd_decode_batch_dev(d, s_dev, frames, bits_dev, ok_dev, iters_dev, stream)); });
    }

protected:
    void fill(acg_ldpc_params &p) const override {
        p.algo = ACG_LDPC_OSD;
        p.max_iter = _order;
        p.lanes_per_frame = _lanes;
    }
    std::pair<TCodeword, bool> finish(const std::vector<uint8_t> &bits, bool ok) const override {
        if (!ok) return {TCodeword(), false};
        return {TCodeword(bits.begin(), bits.end()), true};
    }

private:
    int _order, _lanes;
};

// Scores a batch of parity-check matrices of one m x n under one set of QP-ADMM parameters (acg_ldpc_mc_run_codes): the
// scoring step of optimize_H.cpp:16-25 for many proposals at once.  Thin: one evaluator handle, results as the C ABI's.
class QPADMMEvaluator {
public:
    explicit QPADMMEvaluator(double alpha, double mu, int max_iter = 2000, double eps_stop = 1e-5) {
        acg_ldpc_params p;
        acg_ldpc_params_default(&p);
        p.algo = ACG_LDPC_QPADMM;
        p.alpha = alpha;
        p.mu = mu;
        p.max_iter = max_iter;
        p.eps_stop = eps_stop;
        check(acg_ldpc_evaluator_create(&p, &ev_));
    }
    ~QPADMMEvaluator() { acg_ldpc_evaluator_destroy(ev_); }
    QPADMMEvaluator(const QPADMMEvaluator &) = delete;
    QPADMMEvaluator &operator=(const QPADMMEvaluator &) = delete;

    // res[k] for codes[k] / cfgs[k]; frames, first_frame, snr, seed and noise must be equal in every cfg
    std::vector<acg_ldpc_mc_result> run(const std::vector<const acg_ldpc_code *> &codes, const std::vector<acg_ldpc_mc_cfg> &cfgs) {
        assert(codes.size() == cfgs.size());
        std::vector<acg_ldpc_mc_result> res(codes.size());
        check(acg_ldpc_mc_run_codes(ev_, codes.data(), (int32_t) codes.size(), cfgs.data(), res.data()));
        return res;
    }

    std::string describe() const {
        char b[512];
        acg_ldpc_evaluator_describe(ev_, b, (int32_t) sizeof b);
        return b;
    }

private:
    static void check(int rc) {
        if (rc != 0) {
            std::fprintf(stderr, "acg_ldpc: error %d: %s\n", rc, acg_ldpc_last_error());
            std::abort();
        }
    }
    acg_ldpc_evaluator *ev_ = nullptr;
};

}  // namespace acg_ldpc
