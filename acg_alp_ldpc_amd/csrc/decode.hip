// C ABI of libacg_ldpc_hip.so (include/acg_ldpc.h), part 2: decoding.  The one launch path of every engine (launch_decode),
// the device-buffer entry point, and the pipelined host-buffer entry points with their staging and host threads.
#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>

#include "handle.hpp"

namespace acg {

// A few persistent host threads for the byte shuffling of the host-buffer entry points (pageable user memory -> pinned
// staging, packed words -> one byte per bit): at 25 M frames/s that is ~30-60 GB/s of memcpy, more than one core moves.
class HostPool {
public:
    explicit HostPool(int n) {
        for (int i = 0; i < n; i++) th_.emplace_back([this, i] { run(i); });
    }
    ~HostPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    int size() const { return (int) th_.size(); }
    // fn(part, parts) on every worker thread; returns when all are done
    void run_all(const std::function<void(int, int)> &fn) {
        std::lock_guard<std::mutex> one(call_mu_);   // the pool is shared by every handle of the process: one job at a time
        std::unique_lock<std::mutex> lk(mu_);
        fn_ = &fn;
        pending_ = (int) th_.size();
        gen_++;
        cv_.notify_all();
        done_.wait(lk, [this] { return pending_ == 0; });
        fn_ = nullptr;
    }

private:
    void run(int id) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(int, int)> *fn;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                fn = fn_;
            }
            (*fn)(id, (int) th_.size());
            {
                std::lock_guard<std::mutex> lk(mu_);
                if (--pending_ == 0) done_.notify_all();
            }
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_, call_mu_;
    std::condition_variable cv_, done_;
    const std::function<void(int, int)> *fn_ = nullptr;
    uint64_t gen_ = 0;
    int pending_ = 0;
    bool stop_ = false;
};

// ONE pool per process, created the first time a batch is large enough to use it (>= 4096 frames): a caller that hands a new
// H to every decode — the reference's optimize_H loop, one decoder handle per proposal — must not collect threads per handle.
static HostPool *host_pool() {
    static std::mutex mu;
    static HostPool *pool = nullptr;   // intentionally never destroyed (worker threads must not be joined from a static destructor)
    std::lock_guard<std::mutex> lk(mu);
    if (!pool) {
        const unsigned hc = std::thread::hardware_concurrency();
        pool = new HostPool((int) std::max(2u, std::min(16u, hc ? hc / 2 : 2u)));
    }
    return pool;
}

}  // namespace acg

using namespace acg;

double acg::channel_sigma(double snr) { return std::sqrt(acg_ldpc_llr_variance(snr)); }  // channel.h:20

void acg::fill_channel(DecodeArgs &a, double snr) {
    const double var = acg_ldpc_llr_variance(snr);
    a.var = var;
    a.inv_var2 = 2.0 / var;
    a.sigma = (float) std::sqrt(var);
}

// one launch of a streamed layered engine (q: the integer engine's quantiser, or null; lio: the float engine's LLR entrance and
// its IO instance, or null): a wavefront per tile of the frames, no more than the handle has slabs
static hipError_t launch_streamed_layered(acg_ldpc_decoder *d, const DecodeArgs &a, const QuantArgs *q, hipStream_t s, const StreamLayIo *lio = nullptr) {
    const int T = d->frames_per_block;
    const int grid = (int) std::min<int64_t>((a.frames + T - 1) / T, d->sl_tiles);
    const void *kernel = lio ? d->kernel_lio[d->p.algo == ACG_LDPC_BP_SUMPRODUCT ? 0 : 1] : d->kernel[0];
    return bp_streamed_layered_launch(kernel, d->sltab, a, q, d->sl_ws.as<unsigned char>(), grid, s, lio);
}

// launch on stream s (events recorded around the kernel on that stream).  Caller holds d->mu.
int acg::launch_decode(acg_ldpc_decoder *d, DecodeArgs &a, hipStream_t s, const DecodeIo &io) {
    const QuantIo *qio = io.q;
    const QuantGridArgs *qgrid = io.grid;
    const StreamLayIo *lio = io.llr;
    if (lio && (qio || qgrid || !d->streaml || !lio->llr_in)) {
        set_error("internal: LLRs handed to a launch that cannot take them");
        return 11;
    }
    if (qio && d->osd ? qio->post_out != nullptr : qio && (d->layered_wg != acg_ldpc_decoder::LayeredWg::q || (!d->kernel_qio && !d->streamq))) {
        set_error("internal: channel values handed to a decoder that is not quantized");
        return 11;
    }
    if (qgrid && (qio || d->layered_wg != acg_ldpc_decoder::LayeredWg::q || !d->kernel_qgrid || !qgrid->tab || qgrid->fc == 0 || a.frames >= ((int64_t) 1 << 30))) {
        set_error("internal: a quantiser grid handed to a launch that cannot take it");
        return 11;
    }
    a.max_iter = d->p.max_iter;
    a.early_exit = d->p.early_exit;
    a.ms_scale = (float) d->p.ms_scale;
    a.phi_memo = d->phi_memo ? 1 : 0;
    if (a.frames <= 0) return 0;
    // this launch's own work counter (see acg_ldpc_decoder::work_ring)
    const int slot = (int) (d->launch_seq++ % acg_ldpc_decoder::WORK_RING);
    if (d->ring_used[slot]) HIP_OK(hipStreamWaitEvent(s, d->ring_ev[slot], 0));
    // engines whose HBM workspace belongs to the handle (streamed BP, streamed QP-ADMM): a launch on another stream waits
    // (and the snapshot slots of the fused kernels' freeze path)
    const bool owns_ws = d->streamed || d->streamq || d->streaml || d->freeze || (d->admm && admm_device_streamed(d->admm.get(), nullptr, nullptr, nullptr));
    if (owns_ws && d->last_slot >= 0 && d->last_stream != s) HIP_OK(hipStreamWaitEvent(s, d->ring_ev[d->last_slot], 0));
    a.work_counter = d->work_counter(slot);
    HIP_OK(hipMemsetAsync(a.work_counter, 0, sizeof(unsigned long long), s));
#ifdef ACG_BLOCK_STAMPS
    static unsigned long long *stamp_buf = nullptr;  // developer build only (tools/ab_variant.sh ... -DACG_BLOCK_STAMPS)
    if (!stamp_buf) HIP_OK(hipMalloc((void **) &stamp_buf, 16 * 5 * sizeof(unsigned long long)));
    HIP_OK(hipMemsetAsync(stamp_buf, 0, 16 * 5 * sizeof(unsigned long long), s));
    a.dbg_post = stamp_buf;
#endif
    HIP_OK(hipEventRecord(d->ring_ev0[slot], s));
    if (d->admm) {
        std::string err;
        hipError_t e = admm_launch(d->admm.get(), a, s, err);
        if (e != hipSuccess) {
            set_error(err.empty() ? std::string("admm launch: ") + hipGetErrorString(e) : err);
            return 10;
        }
    } else if (d->streamed) {
        if (a.mc) {
            set_error("internal: streamed engine has no in-kernel generator");
            return 11;
        }
        // W wavefronts cooperate on a tile: 4 when there are enough tiles to fill the chip, more for small batches
        const int64_t tiles = (a.frames + 63) / 64;
        int W = 4;
        while (W < 8 && tiles * W < 8 * (int64_t) d->cu_count) W <<= 1;
        const int per_cu = (W <= 4) ? 2 : 1;
        int grid = (int) std::min<int64_t>(tiles, (int64_t) per_cu * d->cu_count);
        if (d->sring) {
            // traces (acg_ldpc_debug_bp_trace) run the debug instance of the SAME kernel: its sweeps, its counted waits
            const void *kp = d->sring;
            if (a.dbg_c2v || a.dbg_v2c) {
                kp = bp_streamed_ring_ptr_dbg();
                HIP_OK(hipFuncSetAttribute(kp, hipFuncAttributeMaxDynamicSharedMemorySize, RING_LDS_BYTES));
            }
            grid = (int) std::min<int64_t>(tiles, (int64_t) d->sring_per_cu * d->cu_count);
            HIP_OK(bp_streamed_ring_launch(kp, d->stab, a, (uint32_t *) d->sws.va, grid, s));
        } else {
            HIP_OK(bp_streamed_launch(d->skernel, d->stab, a, (uint32_t *) d->sws.va, grid, W * 64, s));
        }
    } else if (d->streamq) {
        if (a.mc) {
            set_error("internal: the streamed quantized engine has no in-kernel generator");
            return 11;
        }
        const int T = d->frames_per_block;
        QuantArgs q = d->qargs;
        if (qio) {
            q.c_in = qio->c_in;
            q.post_out = qio->post_out;
            HIP_OK(launch_streamed_layered(d, a, &q, s));
        } else {
            // the symbol entrance: the handle's quantiser into its staging buffer, then the integer path, a residency of tiles at a time
            const int64_t chunk = std::min<int64_t>(a.frames, (int64_t) d->sl_tiles * T);
            const size_t n = (size_t) d->c.n, nwords = (n + 31) / 32;
            if (int rc = d->sq_stage.reserve((size_t) chunk * n * sizeof(int16_t))) return rc;
            q.c_in = d->sq_stage.as<int16_t>();
            q.post_out = nullptr;
            for (int64_t f0 = 0; f0 < a.frames; f0 += chunk) {
                DecodeArgs ac = a;
                ac.frames = std::min(chunk, a.frames - f0);
                ac.y = static_cast<const unsigned char *>(a.y) + (size_t) f0 * n * (a.y_is_f64 ? 8 : 4);
                if (a.out_bits) ac.out_bits = a.out_bits + (size_t) f0 * nwords;
                if (a.out_ok) ac.out_ok = a.out_ok + f0;
                if (a.out_iters) ac.out_iters = a.out_iters + f0;
                if (f0 > 0) HIP_OK(hipMemsetAsync(a.work_counter, 0, sizeof(unsigned long long), s));   // (the chunks share the launch's counter)
                HIP_OK(quantize_debug_launch(ac, q, ac.frames * (int64_t) n, d->sq_stage.as<int16_t>(), s));
                HIP_OK(launch_streamed_layered(d, ac, &q, s));
            }
        }
    } else if (d->streaml) {
        if (a.mc) {
            set_error("internal: the streamed layered engine has no in-kernel generator");
            return 11;
        }
        HIP_OK(launch_streamed_layered(d, a, nullptr, s, lio));
    } else if (d->osd) {
        if (a.mc) {
            set_error("internal: the OSD engine has no in-kernel generator");
            return 11;
        }
        OsdArgs o = d->oargs;
        o.s_in = qio ? qio->c_in : nullptr;
        HIP_OK(osd_launch(d->kernel[0], o, a, (int) std::min<int64_t>(a.frames, d->grid_cap[0]), d->block, d->lds_block, s));
    } else if (d->layered_wg != acg_ldpc_decoder::LayeredWg::none) {
        if (a.mc) {
            set_error("internal: the workgroup-per-frame layered engine has no in-kernel generator");
            return 11;
        }
        if (qio) {
            // the same launch with the integer entrance's instance and the two pointers behind the quantiser
            QuantArgs q = d->qargs;
            q.c_in = qio->c_in;
            q.post_out = qio->post_out;
            const int grid = (int) std::min<int64_t>(a.frames, d->grid_cap_qio);
            HIP_OK(bp_layered_wg_launch(d->kernel_qio, d->lbtab, a, &q, grid, d->block, d->lds_block, s));
        } else if (qgrid) {
            // the same launch with the grid form's instance: the quantiser block travels but is not read
            const int grid = (int) std::min<int64_t>(a.frames, d->grid_cap_qgrid);
            HIP_OK(bp_layered_wg_launch(d->kernel_qgrid, d->lbtab, a, &d->qargs, grid, d->block, d->lds_block, s, qgrid));
        } else {
            const int grid = (int) std::min<int64_t>(a.frames, d->grid_cap[0]);
            const QuantArgs *q = d->layered_wg == acg_ldpc_decoder::LayeredWg::q ? &d->qargs : nullptr;
            HIP_OK(bp_layered_wg_launch(d->kernel[0], d->lbtab, a, q, grid, d->block, d->lds_block, s));
        }
    } else if (d->layered) {
        const int mc = a.mc ? 1 : 0;
        const int64_t blocks = (a.frames + d->frames_per_block - 1) / d->frames_per_block;
        const int grid = (int) std::min<int64_t>(blocks, d->grid_cap[mc]);
        HIP_OK(bp_layered_launch(d->kernel[mc], d->ltab, a, grid, d->block, d->lds_block, s));
    } else {
        int64_t blocks = (a.frames + d->frames_per_block - 1) / d->frames_per_block;
        const int mc = a.mc ? 1 : 0;
        int grid = (int) std::min<int64_t>(blocks, d->grid_cap[mc]);
        if (d->freeze && !a.dbg_c2v && !a.dbg_v2c) {
            // one slot per frame group of the largest grid this handle launches: sized once, so no launch in flight loses it
            // (the kernel forms 32-bit word offsets: a workspace beyond 2^31 words, far from any code these kernels take, goes without)
            const size_t words = FREEZE_WS_HEAD + (size_t) std::max(d->grid_cap[0], d->grid_cap[1]) * d->frames_per_block * d->freeze_slot_words;
            if (words < ((size_t) 1 << 31)) {
                if (!d->freeze_ws.p) {
                    if (d->freeze_ws.reserve(words * sizeof(uint32_t))) return 10;
                    HIP_OK(hipMemsetAsync(d->freeze_ws.p, 0, FREEZE_WS_HEAD * sizeof(uint32_t), s));
                }
                a.freeze_ws = d->freeze_ws.as<uint32_t>();
                a.freeze_cfg = (uint32_t) d->freeze_first | ((uint32_t) d->freeze_period << 12) | (d->freeze_gate ? 0u : FREEZE_CFG_NO_GATE) |
                               (d->freeze_count ? 0x80000000u : 0u);
            }
        }
        HIP_OK(bp_launch(d->kernel[mc], d->tab, a, grid, d->block, d->lds_block, s));
    }
    HIP_OK(hipEventRecord(d->ring_ev[slot], s));   // stop event of this launch = the event later users of the slot wait on
#ifdef ACG_BLOCK_STAMPS
    if (!d->admm && !d->streamed && getenv("ACG_STAMPS")) {
        unsigned long long h[16 * 5];
        HIP_OK(hipStreamSynchronize(s));
        HIP_OK(hipMemcpy(h, stamp_buf, sizeof(h), hipMemcpyDeviceToHost));
        for (int w = 0; w < 16; w++)
            if (h[w * 5 + 4])
                fprintf(stderr, "[stamps] wave %2d: per sweep: check %6.0f  barrier %6.0f  var %6.0f  barrier %6.0f cycles (%llu sweeps)\n", w,
                        (double) h[w * 5] / h[w * 5 + 4], (double) h[w * 5 + 1] / h[w * 5 + 4], (double) h[w * 5 + 2] / h[w * 5 + 4],
                        (double) h[w * 5 + 3] / h[w * 5 + 4], h[w * 5 + 4]);
    }
#endif
    d->ring_used[slot] = true;
    d->last_slot = slot;
    d->last_stream = s;
    d->ev_valid = true;
    return 0;
}

// the staged outputs (stage_outputs) of `frames` frames
int acg::reserve_outputs(acg_ldpc_decoder *d, int64_t frames) {
    const size_t f = (size_t) frames, nwords = (size_t) (d->c.n + 31) / 32;
    if (int rc = d->st_bits.reserve(f * nwords * sizeof(uint32_t))) return rc;
    if (int rc = d->st_ok.reserve(f)) return rc;
    return d->st_iters.reserve(f * sizeof(int32_t));
}

// outputs of `frames` frames, and room for their symbols as doubles
int acg::ensure_staging(acg_ldpc_decoder *d, int64_t frames) {
    if (int rc = d->st_y.reserve((size_t) frames * d->c.n * sizeof(double))) return rc;
    return reserve_outputs(d, frames);
}

// the decode outputs of a launch into the staging buffers
void acg::stage_outputs(const acg_ldpc_decoder *d, DecodeArgs &a) {
    a.out_bits = d->st_bits.as<uint32_t>();
    a.out_ok = d->st_ok.as<uint8_t>();
    a.out_iters = d->st_iters.as<int32_t>();
}

// the arguments of a plain decode of `frames` frames whose symbols lie at y on the device
DecodeArgs acg::decode_args(const void *y, int y_is_f64, int64_t frames, double snr) {
    DecodeArgs a{};
    a.y = y;
    a.y_is_f64 = y_is_f64;
    a.frames = frames;
    fill_channel(a, snr);
    return a;
}

// One decode chunk on the handle's stream: symbols already on the device in, outputs in the staging buffers (which the
// caller reserved).  io: the entrance (launch_decode) — with io.grid, `frames` virtual frames of a quantiser grid over the
// io.grid->fc frames at y; with io.q or io.llr, channel values in place of y and snr (null and 0: neither is read).
// Caller holds d->mu, so c.slot is this launch's own event pair.
int acg::decode_chunk(acg_ldpc_decoder *d, const void *y, int y_is_f64, int64_t frames, double snr, Chunk &c, const DecodeIo &io) {
    c.a = decode_args(y, y_is_f64, frames, snr);
    stage_outputs(d, c.a);
    const int rc = launch_decode(d, c.a, d->stream, io);
    c.slot = d->last_slot;
    return rc;
}

// the chunk's kernel time, once the caller has synchronised with the stream (0 where the events cannot be read)
float acg::chunk_ms(const acg_ldpc_decoder *d, const Chunk &c) {
    float ms = 0;
    return hipEventElapsedTime(&ms, d->ring_ev0[c.slot], d->ring_ev[c.slot]) == hipSuccess ? ms : 0;
}

// frames per chunk of the pipelined host path: bounded by BYTES (256 MiB of symbols per staging buffer), not by a frame
// count — 65536 frames of the 10 000-symbol code in doubles would pin 2 x 5.2 GB of host memory and as much HBM per handle
int64_t acg::host_chunk_frames(int64_t frames, size_t y_bytes) {
    const int64_t by_bytes = (int64_t) (((size_t) 256 << 20) / std::max<size_t>(y_bytes, 1));
    const int64_t cap = std::max<int64_t>(1024, std::min<int64_t>(1 << 16, by_bytes));
    return std::min<int64_t>(frames, cap);
}

extern "C" {

double acg_ldpc_llr_variance(double snr) { return std::pow(10, -(snr / 10)) / 2; }  // llr_variance, channel.h:12

static int acg_ldpc_decode_batch_dev_impl(acg_ldpc_decoder *d, const void *y_dev, int32_t y_is_f64, int64_t frames, double snr,
                              uint32_t *bits_dev, uint8_t *ok_dev, int32_t *iters_dev, void *stream) {
    if (!d) {
        set_error("null decoder");
        return 1;
    }
    if (frames < 0 || (frames > 0 && !y_dev)) {
        set_error("bad frames / y");
        return 1;
    }
    std::lock_guard<std::recursive_mutex> lk(d->mu);
    HIP_OK(hipSetDevice(d->device));
    DecodeArgs a = decode_args(y_dev, y_is_f64, frames, snr);
    a.out_bits = bits_dev;
    a.out_ok = ok_dev;
    a.out_iters = iters_dev;
    return launch_decode(d, a, stream ? (hipStream_t) stream : d->stream);
}

int acg_ldpc_decode_batch_dev(acg_ldpc_decoder *d, const void *y_dev, int32_t y_is_f64, int64_t frames, double snr,
                              uint32_t *bits_dev, uint8_t *ok_dev, int32_t *iters_dev, void *stream) {
    return guarded([&] { return acg_ldpc_decode_batch_dev_impl(d, y_dev, y_is_f64, frames, snr, bits_dev, ok_dev, iters_dev, stream); });
}

// y_bytes, out_bytes: per frame
static int ensure_pipe(acg_ldpc_decoder *d, int64_t chunk, size_t y_bytes, size_t out_bytes) {
    if (!d->pipe) {
        // built completely before it is published in the handle: a half-made pipe must never be seen by a later call
        std::unique_ptr<HostPipe> np(new HostPipe());
        for (int b = 0; b < HostPipe::NBUF; b++) {
            HIP_OK(hipStreamCreateWithFlags(&np->stream[b], hipStreamNonBlocking));
            HIP_OK(hipEventCreateWithFlags(&np->done[b], hipEventDisableTiming));
        }
        d->pipe = std::move(np);
    }
    HostPipe &P = *d->pipe;
    // keep the buffers while they fit and are not grossly oversized for what is asked now (a 1M-frame batch followed by
    // single-frame decode() calls must not pin hundreds of MB for good)
    const size_t want = (size_t) chunk * y_bytes, have = (size_t) P.chunk * P.y_bytes;
    if (chunk <= P.chunk && y_bytes <= P.y_bytes && out_bytes <= P.out_bytes && (have <= ((size_t) 32 << 20) || have <= 16 * want)) return 0;
    P.release();
    for (int b = 0; b < HostPipe::NBUF; b++) {
        if (int rc = P.pin_y[b].reserve((size_t) chunk * y_bytes)) return rc;
        if (int rc = P.pin_out[b].reserve((size_t) chunk * out_bytes + 16)) return rc;
        if (int rc = P.dev_y[b].reserve((size_t) chunk * y_bytes)) return rc;
        if (int rc = P.dev_out[b].reserve((size_t) chunk * out_bytes + 16)) return rc;
    }
    P.chunk = chunk;
    P.y_bytes = y_bytes;
    P.out_bytes = out_bytes;
    return 0;
}

// packed words -> one byte per bit, 8 bits at a time through a 256-entry table
static void unpack_bits(const uint32_t *words, int nwords, int n, int64_t frames, uint8_t *bits) {
    static const std::vector<uint64_t> lut = [] {
        std::vector<uint64_t> t(256);
        for (int x = 0; x < 256; x++) {
            uint64_t v = 0;
            for (int k = 0; k < 8; k++) v |= (uint64_t) ((x >> k) & 1) << (8 * k);
            t[x] = v;
        }
        return t;
    }();
    for (int64_t f = 0; f < frames; f++) {
        uint8_t *b = bits + (size_t) f * n;
        const uint8_t *w = reinterpret_cast<const uint8_t *>(words + (size_t) f * nwords);
        int v = 0;
        for (; v + 8 <= n; v += 8) std::memcpy(b + v, &lut[w[v >> 3]], 8);
        for (; v < n; v++) b[v] = (w[v >> 3] >> (v & 7)) & 1u;
    }
}

// Host buffers in, host buffers out: chunks of the batch travel through two pinned staging sets.  Per chunk c (set c % 2):
// host threads copy the symbols into pinned memory -> H2D, decode, D2H of words / flags / sweep counts on the set's
// stream -> host threads expand the words into one byte per bit.  Chunk c + 1 is packed and chunk c - 1 unpacked while
// the GPU works on chunk c.  elem = 8 (double symbols: exact LLRs, channel.h:14-16) or 4 (float symbols); elem = 2: int16
// channel values of a quantized handle (acg_ldpc_decode_batch_q; snr unused), whose int16 posteriors come back behind the
// flags of the chunk where post is given, or int16 soft values of an OSD handle (acg_ldpc_osd_decode_batch).  llr (elem = 4):
// fp32 LLRs of a streamed float layered handle (acg_ldpc_decode_batch_llr; snr unused), whose fp32 posteriors come back the same way.
static int decode_batch_host(acg_ldpc_decoder *d, const void *y, int elem, int64_t frames, double snr, uint8_t *bits, uint8_t *ok,
                             int32_t *iters, void *post = nullptr, bool llr = false) {
    const int n = d->c.n, nwords = (n + 31) / 32;
    const size_t y_bytes = (size_t) n * elem;
    const size_t post_bytes = (size_t) n * (llr ? 4 : 2);   // of a frame's posteriors
    const size_t row = (size_t) nwords * 4 + 5;   // words, sweep count and flag of a frame
    auto post_off = [&](int64_t fc) { return ((size_t) fc * row + 15) & ~(size_t) 15; };
    // small batches (single frames: the reference's decode()) take one chunk; large ones <= 64k frames / 256 MiB per chunk
    const int64_t chunk = host_chunk_frames(frames, y_bytes);
    if (int rc = ensure_pipe(d, chunk, y_bytes, row + (post ? post_bytes : 0))) return rc;
    HostPipe &P = *d->pipe;
    const int64_t nchunks = (frames + chunk - 1) / chunk;
    const bool threads = frames >= 4096;  // tiny batches: the hand-off to the pool costs more than the copy
    HostPool *pool = threads ? host_pool() : nullptr;   // process-wide, created on first use
    auto chunk_frames = [&](int64_t c) { return std::min(chunk, frames - c * chunk); };
    auto pack = [&](int64_t c) {
        const int b = (int) (c % HostPipe::NBUF);
        const int64_t fc = chunk_frames(c);
        const unsigned char *src = reinterpret_cast<const unsigned char *>(y) + (size_t) c * chunk * y_bytes;
        unsigned char *dst = P.pin_y[b].as<unsigned char>();
        const size_t total = (size_t) fc * y_bytes;
        if (!threads) {
            std::memcpy(dst, src, total);
            return;
        }
        pool->run_all([&](int part, int parts) {
            const size_t lo = total * part / parts / 64 * 64, hi = (part + 1 == parts) ? total : total * (part + 1) / parts / 64 * 64;
            std::memcpy(dst + lo, src + lo, hi - lo);
        });
    };
    auto submit = [&](int64_t c) -> int {
        const int b = (int) (c % HostPipe::NBUF);
        const int64_t fc = chunk_frames(c);
        hipStream_t s = P.stream[b];
        unsigned char *dev_out = P.dev_out[b].as<unsigned char>();
        HIP_OK(hipMemcpyAsync(P.dev_y[b].p, P.pin_y[b].p, (size_t) fc * y_bytes, hipMemcpyHostToDevice, s));
        DecodeArgs a = decode_args(elem == 2 || llr ? nullptr : P.dev_y[b].p, (elem == 8) ? 1 : 0, fc, snr);
        const QuantIo io{P.dev_y[b].as<int16_t>(), post ? reinterpret_cast<int16_t *>(dev_out + post_off(fc)) : nullptr};
        const StreamLayIo lio{P.dev_y[b].as<float>(), post ? reinterpret_cast<float *>(dev_out + post_off(fc)) : nullptr};
        a.out_bits = reinterpret_cast<uint32_t *>(dev_out);
        a.out_iters = reinterpret_cast<int32_t *>(dev_out + (size_t) fc * nwords * 4);
        a.out_ok = dev_out + (size_t) fc * (nwords * 4 + 4);
        if (int rc = launch_decode(d, a, s, llr ? DecodeIo(&lio) : elem == 2 ? DecodeIo(&io) : DecodeIo())) return rc;
        HIP_OK(hipMemcpyAsync(P.pin_out[b].p, dev_out, post ? post_off(fc) + (size_t) fc * post_bytes : (size_t) fc * row, hipMemcpyDeviceToHost, s));
        HIP_OK(hipEventRecord(P.done[b], s));
        return 0;
    };
    auto collect = [&](int64_t c) -> int {
        const int b = (int) (c % HostPipe::NBUF);
        const int64_t fc = chunk_frames(c), f0 = c * chunk;
        HIP_OK(hipEventSynchronize(P.done[b]));
        const unsigned char *out = P.pin_out[b].as<unsigned char>();
        const uint32_t *pbits = reinterpret_cast<const uint32_t *>(out);
        std::memcpy(ok + f0, out + (size_t) fc * (nwords * 4 + 4), (size_t) fc);
        if (iters) std::memcpy(iters + f0, out + (size_t) fc * nwords * 4, (size_t) fc * 4);
        const unsigned char *ppost = out + post_off(fc);
        unsigned char *const upost = static_cast<unsigned char *>(post);
        if (!threads) {
            unpack_bits(pbits, nwords, n, fc, bits + (size_t) f0 * n);
            if (post) std::memcpy(upost + (size_t) f0 * post_bytes, ppost, (size_t) fc * post_bytes);
            return 0;
        }
        pool->run_all([&](int part, int parts) {
            const int64_t lo = fc * part / parts, hi = fc * (part + 1) / parts;
            unpack_bits(pbits + (size_t) lo * nwords, nwords, n, hi - lo, bits + (size_t) (f0 + lo) * n);
            if (post) std::memcpy(upost + (size_t) (f0 + lo) * post_bytes, ppost + (size_t) lo * post_bytes, (size_t) (hi - lo) * post_bytes);
        });
        return 0;
    };
    pack(0);
    for (int64_t c = 0; c < nchunks; c++) {
        if (int rc = submit(c)) return rc;
        if (c + 1 < nchunks) {
            // set (c + 1) % 2 was last used by chunk c - 1: its results must be out before its buffers are refilled
            if (c >= 1)
                if (int rc = collect(c - 1)) return rc;
            pack(c + 1);
        } else if (c >= 1) {
            if (int rc = collect(c - 1)) return rc;
        }
    }
    return collect(nchunks - 1);
}

// elem = 8: double symbols (acg_ldpc_decode_batch), 4: float symbols (acg_ldpc_decode_batch_f32)
static int decode_batch_impl(acg_ldpc_decoder *d, const void *y, int elem, int64_t frames, double snr, uint8_t *bits, uint8_t *ok,
                             int32_t *iters) {
    if (!d) {
        set_error("null decoder");
        return 1;
    }
    if (frames < 0 || (frames > 0 && (!y || !bits || !ok))) {
        set_error("null buffer");
        return 1;
    }
    if (frames == 0) return 0;
    std::lock_guard<std::recursive_mutex> lk(d->mu);
    HIP_OK(hipSetDevice(d->device));
    return decode_batch_host(d, y, elem, frames, snr, bits, ok, iters);
}

int acg_ldpc_decode_batch(acg_ldpc_decoder *d, const double *y, int64_t frames, double snr, uint8_t *bits, uint8_t *ok,
                          int32_t *iters) {
    return guarded([&] { return decode_batch_impl(d, y, 8, frames, snr, bits, ok, iters); });
}

int acg_ldpc_decode_batch_f32(acg_ldpc_decoder *d, const float *y, int64_t frames, double snr, uint8_t *bits, uint8_t *ok,
                              int32_t *iters) {
    return guarded([&] { return decode_batch_impl(d, y, 4, frames, snr, bits, ok, iters); });
}

// ---- the integer entrance of the fixed-point layered min-sum engine: channel values in, posteriors out ----

// what the three entry points refuse before they look at their buffers
static int quantized_handle(const acg_ldpc_decoder *d) {
    if (!d) {
        set_error("null decoder");
        return 1;
    }
    if (d->layered_wg != acg_ldpc_decoder::LayeredWg::q) {
        set_error("channel values need a decoder of acg_ldpc_decoder_create_quantized");
        return 3;
    }
    return 0;
}

static int quantize_dev_impl(acg_ldpc_decoder *d, const void *y_dev, int32_t y_is_f64, int64_t count, double snr, int16_t *c_dev,
                             void *stream) {
    if (int rc = quantized_handle(d)) return rc;
    if (count < 0 || (count > 0 && (!y_dev || !c_dev))) {
        set_error("bad count / y / c");
        return 1;
    }
    if (count == 0) return 0;
    std::lock_guard<std::recursive_mutex> lk(d->mu);
    HIP_OK(hipSetDevice(d->device));
    const DecodeArgs a = decode_args(y_dev, y_is_f64 ? 1 : 0, count, snr);
    HIP_OK(quantize_debug_launch(a, d->qargs, count, c_dev, stream ? (hipStream_t) stream : d->stream));
    return 0;
}

static int decode_batch_q_dev_impl(acg_ldpc_decoder *d, const int16_t *c_dev, int64_t frames, uint32_t *bits_dev, uint8_t *ok_dev,
                                   int32_t *iters_dev, int16_t *post_dev, void *stream) {
    if (int rc = quantized_handle(d)) return rc;
    if (frames < 0 || (frames > 0 && !c_dev)) {
        set_error("bad frames / c");
        return 1;
    }
    if (frames == 0) return 0;
    std::lock_guard<std::recursive_mutex> lk(d->mu);
    HIP_OK(hipSetDevice(d->device));
    DecodeArgs a = decode_args(nullptr, 0, frames, 0.0);   // (no symbols, no channel: the kernel reads neither)
    a.out_bits = bits_dev;
    a.out_ok = ok_dev;
    a.out_iters = iters_dev;
    const QuantIo io{c_dev, post_dev};
    return launch_decode(d, a, stream ? (hipStream_t) stream : d->stream, &io);
}

static int decode_batch_q_impl(acg_ldpc_decoder *d, const int16_t *c, int64_t frames, uint8_t *bits, uint8_t *ok, int32_t *iters,
                               int16_t *post) {
    if (int rc = quantized_handle(d)) return rc;
    if (frames < 0 || (frames > 0 && (!c || !bits || !ok))) {
        set_error("null buffer");
        return 1;
    }
    if (frames == 0) return 0;
    std::lock_guard<std::recursive_mutex> lk(d->mu);
    HIP_OK(hipSetDevice(d->device));
    return decode_batch_host(d, c, 2, frames, 0.0, bits, ok, iters, post);
}

int acg_ldpc_quantize_dev(acg_ldpc_decoder *d, const void *y_dev, int32_t y_is_f64, int64_t count, double snr, int16_t *c_dev,
                          void *stream) {
    return guarded([&] { return quantize_dev_impl(d, y_dev, y_is_f64, count, snr, c_dev, stream); });
}

int acg_ldpc_decode_batch_q_dev(acg_ldpc_decoder *d, const int16_t *c_dev, int64_t frames, uint32_t *bits_dev, uint8_t *ok_dev,
                                int32_t *iters_dev, int16_t *post_dev, void *stream) {
    return guarded([&] { return decode_batch_q_dev_impl(d, c_dev, frames, bits_dev, ok_dev, iters_dev, post_dev, stream); });
}

int acg_ldpc_decode_batch_q(acg_ldpc_decoder *d, const int16_t *c, int64_t frames, uint8_t *bits, uint8_t *ok, int32_t *iters,
                            int16_t *post) {
    return guarded([&] { return decode_batch_q_impl(d, c, frames, bits, ok, iters, post); });
}

// ---- the LLR entrance of the streamed float layered engine: fp32 LLRs in, fp32 posterior LLRs out ----

// what the two entry points refuse that is not a null or a negative argument
static int streaml_handle(const acg_ldpc_decoder *d) {
    if (!d->streaml) {
        set_error("LLRs need a decoder of acg_ldpc_decoder_create_layered_streamed");
        return 3;
    }
    return 0;
}

static int decode_batch_llr_dev_impl(acg_ldpc_decoder *d, const float *llr_dev, int64_t frames, uint32_t *bits_dev, uint8_t *ok_dev,
                                     int32_t *iters_dev, float *post_dev, void *stream) {
    if (!d) {
        set_error("null decoder");
        return 1;
    }
    if (frames < 0 || (frames > 0 && !llr_dev)) {
        set_error("bad frames / llr");
        return 1;
    }
    if (int rc = streaml_handle(d)) return rc;
    if (frames == 0) return 0;
    std::lock_guard<std::recursive_mutex> lk(d->mu);
    HIP_OK(hipSetDevice(d->device));
    DecodeArgs a = decode_args(nullptr, 0, frames, 0.0);   // (no symbols, no channel: the IO instances read neither)
    a.out_bits = bits_dev;
    a.out_ok = ok_dev;
    a.out_iters = iters_dev;
    const StreamLayIo io{llr_dev, post_dev};
    return launch_decode(d, a, stream ? (hipStream_t) stream : d->stream, &io);
}

static int decode_batch_llr_impl(acg_ldpc_decoder *d, const float *llr, int64_t frames, uint8_t *bits, uint8_t *ok, int32_t *iters, float *post) {
    if (!d) {
        set_error("null decoder");
        return 1;
    }
    if (frames < 0 || (frames > 0 && (!llr || !bits || !ok))) {
        set_error("null buffer");
        return 1;
    }
    if (int rc = streaml_handle(d)) return rc;
    if (frames == 0) return 0;
    std::lock_guard<std::recursive_mutex> lk(d->mu);
    HIP_OK(hipSetDevice(d->device));
    return decode_batch_host(d, llr, 4, frames, 0.0, bits, ok, iters, post, true);
}

int acg_ldpc_decode_batch_llr_dev(acg_ldpc_decoder *d, const float *llr_dev, int64_t frames, uint32_t *bits_dev, uint8_t *ok_dev,
                                  int32_t *iters_dev, float *post_dev, void *stream) {
    return guarded([&] { return decode_batch_llr_dev_impl(d, llr_dev, frames, bits_dev, ok_dev, iters_dev, post_dev, stream); });
}

int acg_ldpc_decode_batch_llr(acg_ldpc_decoder *d, const float *llr, int64_t frames, uint8_t *bits, uint8_t *ok, int32_t *iters,
                              float *post) {
    return guarded([&] { return decode_batch_llr_impl(d, llr, frames, bits, ok, iters, post); });
}

// ---- the integer entrance of the OSD engine: soft values in ----

static int osd_handle(const acg_ldpc_decoder *d) {
    if (!d) {
        set_error("null decoder");
        return 1;
    }
    if (!d->osd) {
        set_error("soft values need a decoder with algo = ACG_LDPC_OSD");
        return 3;
    }
    return 0;
}

static int osd_decode_batch_dev_impl(acg_ldpc_decoder *d, const int16_t *s_dev, int64_t frames, uint32_t *bits_dev, uint8_t *ok_dev,
                                     int32_t *iters_dev, void *stream) {
    if (int rc = osd_handle(d)) return rc;
    if (frames < 0 || (frames > 0 && !s_dev)) {
        set_error("bad frames / s");
        return 1;
    }
    if (frames == 0) return 0;
    std::lock_guard<std::recursive_mutex> lk(d->mu);
    HIP_OK(hipSetDevice(d->device));
    DecodeArgs a = decode_args(nullptr, 0, frames, 0.0);   // (no symbols, no channel: the kernel reads neither)
    a.out_bits = bits_dev;
    a.out_ok = ok_dev;
    a.out_iters = iters_dev;
    const QuantIo io{s_dev, nullptr};
    return launch_decode(d, a, stream ? (hipStream_t) stream : d->stream, &io);
}

static int osd_decode_batch_impl(acg_ldpc_decoder *d, const int16_t *s, int64_t frames, uint8_t *bits, uint8_t *ok, int32_t *iters) {
    if (int rc = osd_handle(d)) return rc;
    if (frames < 0 || (frames > 0 && (!s || !bits || !ok))) {
        set_error("null buffer");
        return 1;
    }
    if (frames == 0) return 0;
    std::lock_guard<std::recursive_mutex> lk(d->mu);
    HIP_OK(hipSetDevice(d->device));
    return decode_batch_host(d, s, 2, frames, 0.0, bits, ok, iters);
}

int acg_ldpc_osd_decode_batch_dev(acg_ldpc_decoder *d, const int16_t *s_dev, int64_t frames, uint32_t *bits_dev, uint8_t *ok_dev,
                                  int32_t *iters_dev, void *stream) {
    return guarded([&] { return osd_decode_batch_dev_impl(d, s_dev, frames, bits_dev, ok_dev, iters_dev, stream); });
}

int acg_ldpc_osd_decode_batch(acg_ldpc_decoder *d, const int16_t *s, int64_t frames, uint8_t *bits, uint8_t *ok, int32_t *iters) {
    return guarded([&] { return osd_decode_batch_impl(d, s, frames, bits, ok, iters); });
}

int acg_ldpc_decoder_sync(acg_ldpc_decoder *d) {
    if (!d) return 1;
    HIP_OK(hipSetDevice(d->device));
    HIP_OK(hipStreamSynchronize(d->stream));
    return 0;
}

float acg_ldpc_decoder_last_kernel_ms(acg_ldpc_decoder *d) {
    if (!d) return -1.0f;
    int slot;
    {
        std::lock_guard<std::recursive_mutex> lk(d->mu);
        if (!d->ev_valid || d->last_slot < 0) return -1.0f;
        slot = d->last_slot;
    }
    (void) hipSetDevice(d->device);
    if (hipEventSynchronize(d->ring_ev[slot]) != hipSuccess) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, d->ring_ev0[slot], d->ring_ev[slot]) != hipSuccess) return -1.0f;
    return ms;
}

}  // extern "C"
