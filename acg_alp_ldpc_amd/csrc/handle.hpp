// The handles behind include/acg_ldpc.h and what the host files of the library share: the types a decoder handle holds, the
// guard of the extern "C" boundary, and one declaration of every host function that one of api.hip / decode.hip / mc.hip /
// mc_codes.hip / cascade.hip / debug.hip defines and another calls.  As with launchers.hpp, the defining file includes it too, so a definition that
// drifts from its declaration does not compile.  Not part of the ABI.
#pragma once

#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <new>

#include "device_mem.hpp"
#include "launchers.hpp"

namespace acg {

const std::string &last_error();  // the calling thread's error text (acg_ldpc_last_error)

// a describe string into the caller's buffer (cut to cap - 1 characters) -> the size a complete copy needs
inline int32_t copy_text(const std::string &s, char *buf, int32_t cap) {
    if (buf && cap > 0) {
        const size_t k = std::min<size_t>(s.size(), (size_t) cap - 1);
        std::memcpy(buf, s.data(), k);
        buf[k] = 0;
    }
    return (int32_t) s.size() + 1;
}

// No C++ exception may cross the extern "C" boundary (std::bad_alloc from a vector, std::system_error from std::thread, ...):
// every entry point that can throw runs its body through guarded() and reports an error code + message instead.
template <class F>
int guarded(F &&body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        set_error("out of host memory");
        return 12;
    } catch (const std::exception &e) {
        set_error(std::string("internal exception: ") + e.what());
        return 13;
    } catch (...) {
        set_error("internal exception");
        return 13;
    }
}

// Double-buffered staging of acg_ldpc_decode_batch / _f32: while the GPU works on chunk c (H2D, kernel, D2H on stream c % 2)
// the host threads fill the pinned buffer of chunk c + 1 and unpack chunk c - 1.
struct HostPipe {
    static constexpr int NBUF = 2;
    int64_t chunk = 0;       // frames per chunk the buffers are sized for
    size_t y_bytes = 0;      // bytes per frame of the symbol buffers
    size_t out_bytes = 0;    // bytes per frame of the output buffers (+ 16 per buffer for the alignment of the posteriors)
    PinnedBuf pin_y[NBUF], pin_out[NBUF];  // out: [frames][nwords] words | [frames] sweep counts | [frames] flags of the chunk in
    DeviceBuf dev_y[NBUF], dev_out[NBUF];  // flight (| [frames][n] posteriors from a 16-byte boundary, int16 where
                                           // acg_ldpc_decode_batch_q, fp32 where acg_ldpc_decode_batch_llr is asked for them):
                                           // one region, so the results come back in ONE device-to-host copy
    hipStream_t stream[NBUF] = {};
    hipEvent_t done[NBUF] = {};
    void release() {
        for (int b = 0; b < NBUF; b++) pin_y[b].reset(), pin_out[b].reset(), dev_y[b].reset(), dev_out[b].reset();
        chunk = 0;
    }
    ~HostPipe() {
        for (int b = 0; b < NBUF; b++) {
            if (done[b]) (void) hipEventDestroy(done[b]);
            if (stream[b]) (void) hipStreamDestroy(stream[b]);
        }
    }
};

// Workspace of the streamed engine as separately created physical chunks mapped into one virtual range in a shuffled order
// (HIP virtual-memory-management API).  Why: see decoder_setup_streamed — a physically CONTIGUOUS backing of the slabs is the
// slow mode of bp_streamed_ring_kernel on slabs beyond the Infinity Cache (181 ms against 158 ms per launch on configs[4]),
// and plain hipMalloc hands out either kind depending on the allocation history of the process.
// Move-only owner; adopt() makes it the owner of one plain allocation instead (the small-workspace and fallback path).
struct ScatteredAlloc {
    void *va = nullptr;
    size_t bytes = 0, chunk = 0;
    std::vector<hipMemGenericAllocationHandle_t> handles;
    std::vector<char> mapped;
    bool plain = false;  // va is ONE allocation (adopt), released by hipFree
    ScatteredAlloc() = default;
    ScatteredAlloc(ScatteredAlloc &&o) noexcept { *this = std::move(o); }
    ScatteredAlloc &operator=(ScatteredAlloc &&o) noexcept {
        release();
        va = o.va, bytes = o.bytes, chunk = o.chunk;
        handles = std::move(o.handles), mapped = std::move(o.mapped), plain = o.plain;
        o.va = nullptr;
        return *this;
    }
    ~ScatteredAlloc() { release(); }
    void adopt(void *p, size_t n) {
        release();
        va = p, bytes = n, plain = true;
    }
    void release() {
        if (!va) return;
        if (plain) {
            (void) hipFree(va);
            va = nullptr, plain = false;
            return;
        }
        for (size_t i = 0; i < handles.size(); i++) {
            if (mapped[i]) (void) hipMemUnmap((char *) va + i * chunk, chunk);
        }
        for (auto &h : handles) (void) hipMemRelease(h);
        (void) hipMemAddressFree(va, bytes);
        va = nullptr;
        handles.clear();
        mapped.clear();
    }
    // -> true on success (va usable, read/write from `dev`)
    // spread > 1: `spread` times as many physical chunks are created and only every spread-th is kept (the others are released
    // again at once), so the kept ones are spaced out over a `spread` times larger part of the device memory
    bool create(size_t want, size_t chunk_bytes, int dev, bool shuffle, int spread = 1);  // api.hip
};

}  // namespace acg

struct acg_ldpc_code {
    acg::Code c;
};

struct acg_ldpc_decoder {
    acg::Code c;  // private copy: the handle outlives the code object safely
    acg_ldpc_params p;
    int device = 0;
    int cu_count = 256;
    hipStream_t stream = nullptr;
    bool own_stream = true;  // false: the stream is an evaluator's (acg_ldpc_mc_run_codes, per-code path) and outlives the handle
    bool ev_valid = false;
    std::recursive_mutex mu;  // (recursive: acg_ldpc_mc_run_grid holds it across the per-point runs of its sequential path)
    std::string name;
    // BP
    acg::BpLayout lay;
    acg::BpTables tab{};
    std::vector<acg::DeviceBuf> dev_allocs;  // the device copies of the tables below
    int maxd = 0, f64 = 0, L = 64;
    int block = 256, frames_per_block = 0;
    int grid_cap[2] = {0, 0};          // [mc] resident blocks: occupancy x CUs
    const void *kernel[2] = {nullptr, nullptr};
    size_t lds_block = 0;
    int variant = -1;       // wave-group kernels: 0 / 1 / 2 (see bp_inst_*.hip); -1 = workgroup-per-frame
    bool phi_memo = false;  // DecodeArgs::phi_memo (the SAT instances read it)
    // the SAT instances' freeze of latched frames whose state recurs (bp_fused_body): one snapshot slot per resident frame
    // group behind a small head with the debug counter (DecodeArgs::freeze_ws), allocated at the first launch
    bool freeze = false;
    bool freeze_count = false;  // acg_ldpc_debug_freeze_stats asked for the counters
    bool freeze_gate = true;    // a per-lane checksum decides whether a detection loads and compares (ACG_BP_FREEZE_NO_GATE=1: always)
    bool phi_split = false;     // the handle runs the instances with the one-series phi (split::; ACG_BP_NO_PHISPLIT=1: those without)
    int freeze_first = 0, freeze_period = 0;
    size_t freeze_slot_words = 0;
    acg::DeviceBuf freeze_ws;
    // name of the build-time instance with this code's pass structure constant that the handle runs (bp_inst_spec.hip); null: the generic one
    const char *spec = nullptr;
    const char *spec_split_rows = nullptr;  // its rows with the one-series phi (BpSpecSig::split_rows), for describe()
    const char *spec_sat_rows = nullptr;  // that instance's fast-path row masks (BpSpecSig::sat_rows), for describe()
    bool pair = false;      // ACG_LDPC_PREC_F16: two frames per workgroup, packed half-precision messages (bp_pair.hip)
    bool blk_idxlds = false, blk_idxreg = false;
    // layered min-sum (bp_layered.hip)
    bool layered = false;
    acg::LayeredLayout llay;
    acg::LayerTables ltab{};
    // layered BP, one workgroup per frame (bp_layered_block.hip): the step and position tables stay in device memory.  Which kernel:
    // bp_layered_block_kernel (check degree <= 8), bp_layered_wide_kernel (<= 32, same tables) or bp_layered_q_kernel (fixed-point
    // min-sum, handles of acg_ldpc_decoder_create_quantized only).  Decode only: Monte-Carlo runs take the unfused route.
    enum class LayeredWg { none, block, wide, q };
    LayeredWg layered_wg = LayeredWg::none;
    acg_ldpc_quant quant{};
    acg::QuantArgs qargs{};
    const void *kernel_qio = nullptr;   // q: the instance of the integer entrance (acg_ldpc_decode_batch_q*) and its resident
    int grid_cap_qio = 0;               // workgroups; kernel[0] stays the symbol entrance's
    const void *kernel_qgrid = nullptr; // q: the grid form of the symbol entrance (acg_ldpc_mc_run_quants: a quantiser per virtual
    int grid_cap_qgrid = 0;             // frame) and its resident workgroups
    acg::LayeredBlockLayout lblay;
    acg::LayerBlockTables lbtab{};
    acg::DeviceBuf lb_step, lb_pos;
    // streamed fixed-point layered min-sum (bp_streamed_q.hip; handles of acg_ldpc_decoder_create_quantized_streamed only): a
    // quantized handle (layered_wg == q, quant, qargs, the sets in lblay) whose frames live in the slabs of sl_ws, one per resident
    // tile of 64 frames.  sq_stage: the symbol entrance's int16 channel values of the frames in flight.
    bool streamq = false;
    acg::DeviceBuf sq_stage;
    // streamed float layered BP (bp_streamed_layered.hip; handles of acg_ldpc_decoder_create_layered_streamed only): sum-product
    // or min-sum with fp32 posteriors and messages, a frame in the slabs of sl_ws, one per resident tile of 64 frames; the sets in
    // lblay.  NOT a quantized handle (layered_wg stays none): the integer entrances refuse it.  Decode only: Monte-Carlo runs take
    // the unfused route.
    bool streaml = false;
    // its IO instances (the LLR entrance, acg_ldpc_decode_batch_llr*): sum-product's and min-sum's, of which launch_decode takes
    // the one of the handle's algorithm; kernel[0] stays the symbol entrance's.  The same slabs and tiles: a grid of the IO
    // instance is bounded by sl_tiles too
    const void *kernel_lio[2] = {nullptr, nullptr};
    // what either of the two has (a handle is at most one of them): the CSR and slab size, the resident tiles, their slabs
    acg::StreamLayTables sltab{};
    int sl_tiles = 0;
    acg::DeviceBuf sl_ws;
    // ordered-statistics decoding (osd.hip; algo = ACG_LDPC_OSD): the packed column table, and what the kernel reads.  One kernel
    // for both entrances (OsdArgs::s_in set per launch); decode only: Monte-Carlo runs take the unfused route.
    bool osd = false;
    acg::OsdArgs oargs{};
    acg::DeviceBuf osd_cols;
    // streamed BP engine
    bool streamed = false;
    acg::StreamTables stab{};
    const void *skernel = nullptr;
    const void *sring = nullptr;  // LDS-DMA ring variant (fp32), null = not available for this code
    int sring_per_cu = 2;
    bool sring_nt = false;  // ring instance with non-temporal slab accesses (slabs beyond the Infinity Cache)
    acg::ScatteredAlloc sws;  // the slabs: shuffled physical chunks, or one plain allocation
    std::vector<float> sws_probe_ms;  // probe time of every workspace candidate that was tried (the fastest was kept)
    int sws_spread = 1;               // the kept physical chunks are every sws_spread-th of those created
    int sgrid = 0;
    // ADMM
    struct AdmmDrop { void operator()(acg::AdmmDevice *a) const { acg::admm_device_destroy(a); } };
    std::unique_ptr<acg::AdmmDevice, AdmmDrop> admm;
    // staging for the host API (ensure_staging)
    acg::DeviceBuf st_y, st_bits, st_ok, st_iters;
    std::unique_ptr<acg::HostPipe> pipe;  // pipelined staging of the host-buffer entry points (created on first use)
    // MC through engines without an in-kernel generator (streamed): chunk buffers
    acg::DeviceBuf mc_y;
    // rate-matched runs (acg_ldpc_mc_run_rm): the pattern of the call, the raw-error counts of a chunk (its channel values: mc_y)
    acg::DeviceBuf rm_pattern, rm_raw;
    // MC
    acg::DeviceBuf cw_dev;
    int64_t cw_count = 0;
    uint64_t cw_hash = 0;
    acg::DeviceBuf counters;
    // detail run (acg_ldpc_mc_run_detail), allocated by its first call: DET_NCOUNTERS counters, one kind byte per frame of a
    // chunk with its pinned copy, the chunk-relative frames selected as events, their records and XOR rows
    acg::DeviceBuf det_counters, det_kind, det_sel, det_events, det_words;
    acg::PinnedBuf det_kind_h, det_sel_h, det_counters_h;
    // parameter grid (acg_ldpc_mc_run_grid; quantiser grid, acg_ldpc_mc_run_quants): counters[point][MC_NCOUNTERS] and the
    // per-point tables of the chunk in flight (q: 32 bytes per point, the head of its QuantArgs)
    acg::DeviceBuf grid_counters, grid_tab;
    // Per-launch work counters: every launch takes the next slot of a small ring of device words (the dynamic frame /
    // tile hand-out of the kernels), so launches of one handle that overlap on different streams never share one.
    // ring_ev[k] is recorded behind the launch that used slot k; the next user of the slot — and, for the streamed
    // engine, whose HBM slabs belong to the handle, every launch on a different stream — waits on it on the device.
    // Timing: every launch also owns the (start, stop) event pair of its slot, so two launches of one handle in flight on
    // two streams never pair each other's events; ring_ev[k] IS the stop event of slot k.
    static constexpr int WORK_RING = 32;
    acg::DeviceBuf work_ring;
    hipEvent_t ring_ev0[WORK_RING] = {};
    hipEvent_t ring_ev[WORK_RING] = {};
    bool ring_used[WORK_RING] = {};
    uint64_t launch_seq = 0;
    int last_slot = -1;
    hipStream_t last_stream = nullptr;

    unsigned long long *counters_dev() const { return counters.as<unsigned long long>(); }
    unsigned long long *work_counter(int slot) const { return work_ring.as<unsigned long long>() + slot; }
};

namespace acg {

// owned until handed out: an exception or an error releases the streams, events and device memory made so far
struct DecoderDrop { void operator()(acg_ldpc_decoder *x) const { acg_ldpc_decoder_destroy(x); } };
using DecoderPtr = std::unique_ptr<acg_ldpc_decoder, DecoderDrop>;

}  // namespace acg

// Two decoders for one code on one device and the buffers of the hand-over between them (cascade.hip; the Monte-Carlo run in
// mc.hip).  A call holds mu, then stage[0]->mu, then stage[1]->mu.
struct acg_ldpc_cascade {
    acg::DecoderPtr stage[2];
    std::mutex mu;
    std::string name;  // "<first>+<second>"
    int device = 0;
    // the chunk in flight: the failed frames' indices and their count (with its pinned copy), their symbols, and the second
    // decoder's outputs for them; sized by ensure() for the largest chunk so far, released by release()
    int64_t cap_frames = 0;
    size_t cap_row = 0;  // bytes of a symbol row the compact buffer was sized for
    acg::DeviceBuf idx, count, c_y, c_bits, c_ok, c_iters;
    // posterior hand-over (stage 0 quantized, stage 1 OSD): the chunk's channel values and posteriors; c_y holds the failed
    // frames' posterior rows
    bool post_handover = false;
    acg::DeviceBuf q_c, q_post;
    acg::PinnedBuf count_h;
    // recorded behind every chunk that handed frames on: the next chunk waits for it on ITS stream before it reuses the buffers
    hipEvent_t tail_ev = nullptr;
    bool tail_used = false;
    // of the most recent decode call (acg_ldpc_cascade_last_call): the second stage's launch of the last chunk may still run,
    // so its event slot is kept instead of its time
    int64_t last_chunk = 0;  // frames per chunk that call used
    int64_t last_second = 0;
    float last_ms[2] = {0, 0};
    int pending_slot = -1;
    // Monte-Carlo run: symbols and outputs of a chunk; counters rows `first`, `total`, then the second stage's sweeps
    acg::DeviceBuf mc_y, mc_bits, mc_ok, mc_iters, mc_counters;
    void release() {
        idx.reset(), count.reset(), c_y.reset(), c_bits.reset(), c_ok.reset(), c_iters.reset(), count_h.reset(), q_c.reset(), q_post.reset();
        cap_frames = 0, cap_row = 0;
    }
};

namespace acg {

// ---- api.hip (on_stream != null: the handle works on that stream of the caller's instead of one of its own;
// quant != null: the fixed-point layered min-sum engine of acg_ldpc_decoder_create_quantized, or with q_streamed the one of
// acg_ldpc_decoder_create_quantized_streamed; l_streamed (quant null): the streamed float layered engine of
// acg_ldpc_decoder_create_layered_streamed) ----
int acg_ldpc_decoder_create_impl(const acg_ldpc_code *code, const acg_ldpc_params *params, acg_ldpc_decoder **out,
                                 hipStream_t on_stream = nullptr, const acg_ldpc_quant *quant = nullptr, bool q_streamed = false,
                                 bool l_streamed = false);
QuantArgs quant_args(const acg_ldpc_quant &q);

// ---- decode.hip ----
double channel_sigma(double snr);
void fill_channel(DecodeArgs &a, double snr);
// What a launch takes besides the symbols at a.y; none set: the symbol entrance.  A pointer of one of the three types converts,
// so a call site passes &io of the entrance it means.
// q: the integer entrance of a quantized handle — channel values instead of a.y, posteriors where asked for; of an OSD handle —
//    soft values instead of a.y (post_out null)
// grid: the grid form of a quantized handle — a.frames virtual frames, a quantiser per point instead of the handle's
// llr: the LLR entrance of a streamed float layered handle — LLRs instead of a.y, posteriors where asked for
struct DecodeIo {
    const QuantIo *q = nullptr;
    const QuantGridArgs *grid = nullptr;
    const StreamLayIo *llr = nullptr;
    DecodeIo() = default;
    DecodeIo(const QuantIo *q_) : q(q_) {}
    DecodeIo(const QuantGridArgs *grid_) : grid(grid_) {}
    DecodeIo(const StreamLayIo *llr_) : llr(llr_) {}
};
int launch_decode(acg_ldpc_decoder *d, DecodeArgs &a, hipStream_t s, const DecodeIo &io = {});
int reserve_outputs(acg_ldpc_decoder *d, int64_t frames);
int ensure_staging(acg_ldpc_decoder *d, int64_t frames);
void stage_outputs(const acg_ldpc_decoder *d, DecodeArgs &a);
DecodeArgs decode_args(const void *y, int y_is_f64, int64_t frames, double snr);
struct Chunk {  // one decode on the handle's stream: its arguments and its event slot
    DecodeArgs a;
    int slot;
};
int decode_chunk(acg_ldpc_decoder *d, const void *y, int y_is_f64, int64_t frames, double snr, Chunk &c, const DecodeIo &io = {});
float chunk_ms(const acg_ldpc_decoder *d, const Chunk &c);
// frames per chunk of the pipelined host path for symbol rows of y_bytes: at most 65536 frames / 256 MiB of symbols
int64_t host_chunk_frames(int64_t frames, size_t y_bytes);

// ---- mc.hip (what mc_codes.hip and cascade.hip call) ----
int check_mc_cfg(const acg_ldpc_mc_cfg *cfg);
void pack_codewords(const uint8_t *codewords, int64_t n_codewords, int n, uint32_t *out);
void noise_host(int n, int64_t first, int64_t fc, double snr, double *out);
void counters_to_result(const unsigned long long *c, acg_ldpc_mc_result *r);
int acg_ldpc_mc_run_impl(acg_ldpc_decoder *d, const acg_ldpc_mc_cfg *cfg, acg_ldpc_mc_result *res);
// the frames a developer / test variable holds (README, developer variables); 0: not set, or not a positive count
int64_t env_frames(const char *name);
int64_t mc_grid_budget();
// `points` points over `frames` > 0 frames in launches of at most `budget` virtual frames: frames in blocks of fb, points in
// chunks of npc >= 1, npc * fb <= budget (or one point's fb frames)
struct PointChunks {
    int64_t fb, npc;
};
PointChunks point_chunks(int64_t budget, int64_t frames, int64_t points);

// ---- cascade.hip ----
// frames per chunk of a cascade call over `frames` frames of symbol rows of row_bytes (host_chunk_frames; ACG_CASCADE_CHUNK lowers it)
int64_t cascade_chunk_frames(int64_t frames, size_t row_bytes);
// the Monte-Carlo run's two looks into a chunk, both on the chunk's stream: first_done when stage 0's outputs stand in the
// caller's buffers (before the select), second_done(K) when stage 1's stand in the compact ones (before the scatter)
struct CascadeHooks {
    std::function<int()> first_done;
    std::function<int(int64_t)> second_done;
};
// One chunk of fc <= the frames ensure()d: stage 0 -> select -> wait for K -> gather, stage 1, scatter (asynchronous behind the
// wait); K and the launches' times are added to c->last_second / c->last_ms.  Caller holds the three mutexes, has set the
// device and called cascade_begin and cascade_ensure for fc.
int cascade_ensure(acg_ldpc_cascade *c, int64_t frames, size_t row_bytes);
// a new call in chunks of `chunk` frames: what acg_ldpc_cascade_last_call reports starts from zero
void cascade_begin(acg_ldpc_cascade *c, int64_t chunk);
// waits for the second stage's launch of the last chunk, which a call leaves running, and books its time in c->last_ms[1]
int cascade_settle(acg_ldpc_cascade *c);
int cascade_chunk_dev(acg_ldpc_cascade *c, const void *y, int y_is_f64, int64_t fc, double snr, uint32_t *bits, uint8_t *ok, int32_t *iters,
                      uint8_t *stage, hipStream_t s, const CascadeHooks *hooks = nullptr);

}  // namespace acg
