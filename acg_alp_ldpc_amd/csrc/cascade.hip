// C ABI of libacg_ldpc_hip.so (include/acg_ldpc.h), part 5: two-stage decoding.  A cascade owns two decoder handles for one
// code; a frame the first gives up on (ok = 0) is decoded again by the second, from the same symbols — or, where the first is
// a quantized handle and the second OSD, from the first's posteriors (post_handover).  The engines are the
// handles' own (launch_decode): what is new is the hand-over, which stays on the device — select, gather, scatter
// (cascade_kernels.hip) — with one host wait per chunk, for the number of failed frames.  The Monte-Carlo run is in mc.hip.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "handle.hpp"

using namespace acg;

// ACG_CASCADE_CHUNK=<frames>: developer / test switch that lowers the chunk of a cascade call (README, developer variables)
int64_t acg::cascade_chunk_frames(int64_t frames, size_t row_bytes) {
    const int64_t chunk = host_chunk_frames(std::max<int64_t>(frames, 1), row_bytes);
    const int64_t v = env_frames("ACG_CASCADE_CHUNK");
    return v ? std::min(chunk, v) : chunk;
}

// the hand-over buffers for chunks of up to `frames` frames whose symbol rows have row_bytes
int acg::cascade_ensure(acg_ldpc_cascade *c, int64_t frames, size_t row_bytes) {
    if (frames <= c->cap_frames && row_bytes <= c->cap_row) return 0;
    const size_t f = (size_t) std::max(frames, c->cap_frames), row = std::max(row_bytes, c->cap_row);
    const size_t nwords = (size_t) (c->stage[0]->c.n + 31) / 32;
    // (reserve() frees a buffer that has to grow, and hipFree waits for the device: no launch of an earlier call still uses it)
    if (int rc = c->idx.reserve(f * sizeof(int32_t))) return rc;
    if (int rc = c->count.reserve(sizeof(int32_t))) return rc;
    if (int rc = c->count_h.reserve(sizeof(int32_t))) return rc;
    if (int rc = c->c_y.reserve(f * row)) return rc;
    if (int rc = c->c_bits.reserve(f * nwords * sizeof(uint32_t))) return rc;
    if (int rc = c->c_ok.reserve(f)) return rc;
    if (int rc = c->c_iters.reserve(f * sizeof(int32_t))) return rc;
    if (c->post_handover) {
        const size_t vals = f * (size_t) c->stage[0]->c.n * sizeof(int16_t);
        if (int rc = c->q_c.reserve(vals)) return rc;
        if (int rc = c->q_post.reserve(vals)) return rc;
    }
    c->cap_frames = (int64_t) f;
    c->cap_row = row;
    return 0;
}

// device time of a finished decode launch of handle d
static float slot_ms(const acg_ldpc_decoder *d, int slot) {
    float ms = 0;
    return slot >= 0 && hipEventElapsedTime(&ms, d->ring_ev0[slot], d->ring_ev[slot]) == hipSuccess ? ms : 0;
}

// the second stage's launch of the last chunk, which the call left running: wait for it and book its time
int acg::cascade_settle(acg_ldpc_cascade *c) {
    if (c->pending_slot < 0) return 0;
    const acg_ldpc_decoder *d1 = c->stage[1].get();
    HIP_OK(hipEventSynchronize(d1->ring_ev[c->pending_slot]));
    c->last_ms[1] += slot_ms(d1, c->pending_slot);
    c->pending_slot = -1;
    return 0;
}

int acg::cascade_chunk_dev(acg_ldpc_cascade *c, const void *y, int y_is_f64, int64_t fc, double snr, uint32_t *bits, uint8_t *ok,
                           int32_t *iters, uint8_t *stage, hipStream_t s, const CascadeHooks *hooks) {
    acg_ldpc_decoder *d0 = c->stage[0].get(), *d1 = c->stage[1].get();
    const int n = d0->c.n, nwords = (n + 31) / 32;
    if (fc <= 0 || fc > c->cap_frames || (size_t) n * (y_is_f64 ? 8 : 4) > c->cap_row) {
        set_error("internal: a cascade chunk its buffers were not sized for");
        return 11;
    }
    // the hand-over buffers are the cascade's: a chunk on another stream than the previous one waits for that one's tail
    if (c->tail_used) HIP_OK(hipStreamWaitEvent(s, c->tail_ev, 0));
    // 1. stage 0, straight into the caller's outputs
    DecodeArgs a = decode_args(y, y_is_f64, fc, snr);
    a.out_bits = bits;
    a.out_ok = ok;
    a.out_iters = iters;
    if (c->post_handover) {
        // stage 0 through its quantiser and its integer entrance — equal to its symbol entrance (include/acg_ldpc.h) — so that
        // its posteriors stand in q_post
        HIP_OK(quantize_debug_launch(decode_args(y, y_is_f64, fc * n, snr), d0->qargs, fc * n, c->q_c.as<int16_t>(), s));
        a.y = nullptr;
        const QuantIo io{c->q_c.as<int16_t>(), c->q_post.as<int16_t>()};
        if (int rc = launch_decode(d0, a, s, &io)) return rc;
    } else if (int rc = launch_decode(d0, a, s)) {
        return rc;
    }
    const int slot0 = d0->last_slot;
    if (hooks && hooks->first_done)
        if (int rc = hooks->first_done()) return rc;
    // 2. select; K comes to the host: the one wait of the chunk
    int32_t *idx = c->idx.as<int32_t>(), *count_h = c->count_h.as<int32_t>();
    HIP_OK(cascade_select_launch(ok, (int32_t) fc, idx, c->count.as<int32_t>(), stage, s));
    HIP_OK(hipMemcpyAsync(count_h, c->count.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    // (the stream is idle: stage 0 of this chunk and stage 1 of the previous one have finished, their events can be read)
    c->last_ms[0] += slot_ms(d0, slot0);
    if (int rc = cascade_settle(c)) return rc;
    const int64_t K = *count_h;
    if (K < 0 || K > fc) {
        set_error("acg_ldpc_cascade: the select kernel reported " + std::to_string(K) + " failed frames in a chunk of " + std::to_string(fc));
        return 11;
    }
    c->last_second += K;
    if (K == 0) return 0;
    // 3. gather, stage 1 over the compact batch, scatter
    // (posterior hand-over: the failed frames' int16 posterior rows instead of their symbol rows, into OSD's integer entrance)
    if (c->post_handover) HIP_OK(cascade_gather_launch(c->q_post.p, 2, n, idx, (int32_t) K, c->c_y.p, s));
    else HIP_OK(cascade_gather_launch(y, y_is_f64 ? 8 : 4, n, idx, (int32_t) K, c->c_y.p, s));
    DecodeArgs b = decode_args(c->post_handover ? nullptr : c->c_y.p, y_is_f64, K, snr);
    b.out_bits = c->c_bits.as<uint32_t>();
    b.out_ok = c->c_ok.as<uint8_t>();
    b.out_iters = c->c_iters.as<int32_t>();
    const QuantIo io1{c->c_y.as<int16_t>(), nullptr};
    if (int rc = launch_decode(d1, b, s, c->post_handover ? DecodeIo(&io1) : DecodeIo())) return rc;
    c->pending_slot = d1->last_slot;
    if (hooks && hooks->second_done)
        if (int rc = hooks->second_done(K)) return rc;
    HIP_OK(cascade_scatter_launch(b.out_bits, b.out_ok, b.out_iters, idx, (int32_t) K, nwords, bits, ok, iters, stage, s));
    HIP_OK(hipEventRecord(c->tail_ev, s));
    c->tail_used = true;
    return 0;
}

// a new call: what acg_ldpc_cascade_last_call reports starts from zero
void acg::cascade_begin(acg_ldpc_cascade *c, int64_t chunk) {
    c->last_chunk = chunk;
    c->last_second = 0;
    c->last_ms[0] = c->last_ms[1] = 0;
    c->pending_slot = -1;
}

static int cascade_create_impl(const acg_ldpc_code *code, const acg_ldpc_params *first, const acg_ldpc_quant *q_first,
                               const acg_ldpc_params *second, const acg_ldpc_quant *q_second, acg_ldpc_cascade **out) {
    if (!code || !first || !second || !out) {
        set_error("null argument");
        return 1;
    }
    auto resolved = [](int dev) {
        if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
        return dev;
    };
    const int dev0 = resolved(first->device), dev1 = resolved(second->device);
    if (dev0 != dev1) {
        set_error("acg_ldpc_cascade_create: the two decoders resolve to different devices (" + std::to_string(dev0) + " and " +
                  std::to_string(dev1) + ")");
        return 1;
    }
    struct Drop { void operator()(acg_ldpc_cascade *x) const { acg_ldpc_cascade_destroy(x); } };
    std::unique_ptr<acg_ldpc_cascade, Drop> own(new acg_ldpc_cascade());
    acg_ldpc_cascade *c = own.get();
    const acg_ldpc_params *p[2] = {first, second};
    const acg_ldpc_quant *q[2] = {q_first, q_second};
    for (int k = 0; k < 2; k++) {
        acg_ldpc_decoder *d = nullptr;
        if (int rc = acg_ldpc_decoder_create_impl(code, p[k], &d, nullptr, q[k])) {
            set_error(std::string(k ? "second: " : "first: ") + last_error());
            return rc;
        }
        c->stage[k].reset(d);
    }
    c->post_handover = q[0] && !q[1] && c->stage[1]->osd;
    c->device = c->stage[0]->device;
    c->name = c->stage[0]->name + "+" + c->stage[1]->name;
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(hipEventCreateWithFlags(&c->tail_ev, hipEventDisableTiming));
    *out = own.release();
    return 0;
}

static int cascade_decode_dev_impl(acg_ldpc_cascade *c, const void *y_dev, int32_t y_is_f64, int64_t frames, double snr,
                                   uint32_t *bits_dev, uint8_t *ok_dev, int32_t *iters_dev, uint8_t *stage_dev, void *stream) {
    if (!c) {
        set_error("null cascade");
        return 1;
    }
    if (frames < 0) {
        set_error("acg_ldpc_cascade_decode_batch_dev: frames < 0");
        return 1;
    }
    if (frames > 0 && !y_dev) {
        set_error("acg_ldpc_cascade_decode_batch_dev: null y with frames > 0");
        return 1;
    }
    if (!bits_dev || !ok_dev) {
        set_error("acg_ldpc_cascade_decode_batch_dev: null bits or ok");
        return 1;
    }
    acg_ldpc_decoder *d0 = c->stage[0].get(), *d1 = c->stage[1].get();
    std::lock_guard<std::mutex> lk(c->mu);
    std::lock_guard<std::recursive_mutex> lk0(d0->mu);
    std::lock_guard<std::recursive_mutex> lk1(d1->mu);
    const int n = d0->c.n, nwords = (n + 31) / 32, f64 = y_is_f64 ? 1 : 0;
    const size_t row = (size_t) n * (f64 ? 8 : 4);
    const int64_t chunk = cascade_chunk_frames(frames, row);
    cascade_begin(c, chunk);
    if (frames == 0) return 0;
    HIP_OK(hipSetDevice(c->device));
    if (int rc = cascade_ensure(c, chunk, row)) return rc;
    hipStream_t s = stream ? (hipStream_t) stream : d0->stream;
    for (int64_t f0 = 0; f0 < frames; f0 += chunk) {
        const int64_t fc = std::min(chunk, frames - f0);
        if (int rc = cascade_chunk_dev(c, (const unsigned char *) y_dev + (size_t) f0 * row, f64, fc, snr, bits_dev + (size_t) f0 * nwords,
                                       ok_dev + f0, iters_dev ? iters_dev + f0 : nullptr, stage_dev ? stage_dev + f0 : nullptr, s))
            return rc;
    }
    return 0;
}

// The host entry points compose the host paths the two handles already have: first's pipelined decode over all frames, the
// failed rows gathered on the host, second's decode over them, the results scattered on the host.  Nothing new runs on the device.
static int cascade_decode_host_impl(acg_ldpc_cascade *c, const void *y, int elem, int64_t frames, double snr, uint8_t *bits, uint8_t *ok,
                                    int32_t *iters, uint8_t *stage) {
    if (!c) {
        set_error("null cascade");
        return 1;
    }
    if (frames < 0) {
        set_error("acg_ldpc_cascade_decode_batch: frames < 0");
        return 1;
    }
    if (frames > 0 && !y) {
        set_error("acg_ldpc_cascade_decode_batch: null y with frames > 0");
        return 1;
    }
    if (!bits || !ok) {
        set_error("acg_ldpc_cascade_decode_batch: null bits or ok");
        return 1;
    }
    acg_ldpc_decoder *d0 = c->stage[0].get(), *d1 = c->stage[1].get();
    std::lock_guard<std::mutex> lk(c->mu);
    std::lock_guard<std::recursive_mutex> lk0(d0->mu);
    std::lock_guard<std::recursive_mutex> lk1(d1->mu);
    const size_t n = (size_t) d0->c.n, row = n * elem;
    if (c->post_handover) {
        // the posteriors exist on the device only: the chunks of the device path, symbols copied in and outputs copied out
        const int nwords = (int) (n + 31) / 32;
        const int64_t chunk = cascade_chunk_frames(frames, row);
        cascade_begin(c, chunk);
        if (frames == 0) return 0;
        HIP_OK(hipSetDevice(c->device));
        if (int rc = cascade_ensure(c, chunk, row)) return rc;
        DeviceBuf dy, dbits, dok, dit, dst;
        if (int rc = dy.reserve((size_t) chunk * row)) return rc;
        if (int rc = dbits.reserve((size_t) chunk * nwords * sizeof(uint32_t))) return rc;
        if (int rc = dok.reserve((size_t) chunk)) return rc;
        if (int rc = dit.reserve((size_t) chunk * sizeof(int32_t))) return rc;
        if (int rc = dst.reserve((size_t) chunk)) return rc;
        std::vector<uint32_t> hbits((size_t) chunk * nwords);
        hipStream_t s = d0->stream;
        for (int64_t f0 = 0; f0 < frames; f0 += chunk) {
            const int64_t fc = std::min(chunk, frames - f0);
            HIP_OK(hipMemcpyAsync(dy.p, (const unsigned char *) y + (size_t) f0 * row, (size_t) fc * row, hipMemcpyHostToDevice, s));
            if (int rc = cascade_chunk_dev(c, dy.p, elem == 8 ? 1 : 0, fc, snr, dbits.as<uint32_t>(), dok.as<uint8_t>(), dit.as<int32_t>(), dst.as<uint8_t>(), s))
                return rc;
            HIP_OK(hipStreamSynchronize(s));
            HIP_OK(hipMemcpy(hbits.data(), dbits.p, (size_t) fc * nwords * sizeof(uint32_t), hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(ok + f0, dok.p, (size_t) fc, hipMemcpyDeviceToHost));
            if (iters) HIP_OK(hipMemcpy(iters + f0, dit.p, (size_t) fc * sizeof(int32_t), hipMemcpyDeviceToHost));
            if (stage) HIP_OK(hipMemcpy(stage + f0, dst.p, (size_t) fc, hipMemcpyDeviceToHost));
            for (int64_t f = 0; f < fc; f++)
                for (size_t v = 0; v < n; v++) bits[(size_t) (f0 + f) * n + v] = (hbits[(size_t) f * nwords + (v >> 5)] >> (v & 31)) & 1u;
        }
        return cascade_settle(c);
    }
    cascade_begin(c, host_chunk_frames(std::max<int64_t>(frames, 1), row));
    if (frames == 0) return 0;
    auto decode = [&](acg_ldpc_decoder *d, const void *sym, int64_t f, uint8_t *b, uint8_t *o, int32_t *it) {
        return elem == 8 ? acg_ldpc_decode_batch(d, (const double *) sym, f, snr, b, o, it) : acg_ldpc_decode_batch_f32(d, (const float *) sym, f, snr, b, o, it);
    };
    if (int rc = decode(d0, y, frames, bits, ok, iters)) return rc;
    c->last_ms[0] = std::max(0.0f, acg_ldpc_decoder_last_kernel_ms(d0));
    if (stage) std::memset(stage, 1, (size_t) frames);
    std::vector<int64_t> idx;
    for (int64_t f = 0; f < frames; f++)
        if (!ok[f]) idx.push_back(f);
    const size_t K = idx.size();
    c->last_second = (int64_t) K;
    if (K == 0) return 0;
    std::vector<unsigned char> cy(K * row), cbits(K * n), cok(K);
    std::vector<int32_t> cit(K);
    for (size_t k = 0; k < K; k++) std::memcpy(&cy[k * row], (const unsigned char *) y + (size_t) idx[k] * row, row);
    if (int rc = decode(d1, cy.data(), (int64_t) K, cbits.data(), cok.data(), cit.data())) return rc;
    c->last_ms[1] = std::max(0.0f, acg_ldpc_decoder_last_kernel_ms(d1));
    for (size_t k = 0; k < K; k++) {
        const size_t f = (size_t) idx[k];
        std::memcpy(bits + f * n, &cbits[k * n], n);
        ok[f] = cok[k];
        if (iters) iters[f] = cit[k];
        if (stage) stage[f] = 2;
    }
    return 0;
}

extern "C" {

int acg_ldpc_cascade_create(const acg_ldpc_code *code, const acg_ldpc_params *first, const acg_ldpc_quant *q_first,
                            const acg_ldpc_params *second, const acg_ldpc_quant *q_second, acg_ldpc_cascade **out) {
    return guarded([&] { return cascade_create_impl(code, first, q_first, second, q_second, out); });
}

void acg_ldpc_cascade_destroy(acg_ldpc_cascade *c) {
    if (!c) return;
    (void) hipSetDevice(c->device);
    // the tail of the last call may still run on a caller's stream; the stages wait for their own launches when they go
    if (c->tail_ev) {
        if (c->tail_used) (void) hipEventSynchronize(c->tail_ev);
        (void) hipEventDestroy(c->tail_ev);
    }
    c->stage[1].reset();
    c->stage[0].reset();
    delete c;
}

acg_ldpc_decoder *acg_ldpc_cascade_stage(acg_ldpc_cascade *c, int32_t stage) {
    if (!c || stage < 0 || stage > 1) {
        set_error("acg_ldpc_cascade_stage: null cascade, or a stage that is not 0 or 1");
        return nullptr;
    }
    return c->stage[stage].get();
}

const char *acg_ldpc_cascade_name(const acg_ldpc_cascade *c) { return c ? c->name.c_str() : ""; }

int32_t acg_ldpc_cascade_describe(const acg_ldpc_cascade *c, char *buf, int32_t cap) {
    if (!c) return 0;
    return guarded([&] {
        std::string t = "cascade " + c->name;
        for (int k = 0; k < 2; k++) {
            std::vector<char> b((size_t) std::max(1, acg_ldpc_decoder_describe(c->stage[k].get(), nullptr, 0)));
            (void) acg_ldpc_decoder_describe(c->stage[k].get(), b.data(), (int32_t) b.size());
            t += std::string(k ? " | second: " : " | first: ") + b.data();
        }
        // (the two figures of the last call are read without the mutex: describe is a diagnostic, as the decoder's is)
        t += " | chunk=" + std::to_string(c->last_chunk ? c->last_chunk : cascade_chunk_frames(1 << 16, (size_t) c->stage[0]->c.n * 4)) +
             " last_second_frames=" + std::to_string(c->last_second) + (c->post_handover ? " handover=posteriors" : " handover=symbols");
        return (int) copy_text(t, buf, cap);
    });
}

int acg_ldpc_cascade_decode_batch_dev(acg_ldpc_cascade *c, const void *y_dev, int32_t y_is_f64, int64_t frames, double snr,
                                      uint32_t *bits_dev, uint8_t *ok_dev, int32_t *iters_dev, uint8_t *stage_dev, void *stream) {
    return guarded([&] { return cascade_decode_dev_impl(c, y_dev, y_is_f64, frames, snr, bits_dev, ok_dev, iters_dev, stage_dev, stream); });
}

int acg_ldpc_cascade_decode_batch(acg_ldpc_cascade *c, const double *y, int64_t frames, double snr, uint8_t *bits, uint8_t *ok,
                                  int32_t *iters, uint8_t *stage) {
    return guarded([&] { return cascade_decode_host_impl(c, y, 8, frames, snr, bits, ok, iters, stage); });
}

int acg_ldpc_cascade_decode_batch_f32(acg_ldpc_cascade *c, const float *y, int64_t frames, double snr, uint8_t *bits, uint8_t *ok,
                                      int32_t *iters, uint8_t *stage) {
    return guarded([&] { return cascade_decode_host_impl(c, y, 4, frames, snr, bits, ok, iters, stage); });
}

int acg_ldpc_cascade_last_call(acg_ldpc_cascade *c, int64_t *second_frames, float *first_ms, float *second_ms) {
    if (!c) {
        set_error("null cascade");
        return 1;
    }
    return guarded([&] {
        std::lock_guard<std::mutex> lk(c->mu);
        HIP_OK(hipSetDevice(c->device));
        if (int rc = cascade_settle(c)) return rc;
        if (second_frames) *second_frames = c->last_second;
        if (first_ms) *first_ms = c->last_ms[0];
        if (second_ms) *second_ms = c->last_ms[1];
        return 0;
    });
}

}  // extern "C"
