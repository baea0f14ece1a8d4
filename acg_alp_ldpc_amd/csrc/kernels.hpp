// Device-facing argument blocks shared by the .hip kernels and the host API.  Not part of the ABI.
#pragma once

#include <cstdint>

namespace acg {

// Device copies of BpLayout (see ldpc_internal.hpp for the meaning of each table).
struct BpTables {
    const int32_t *c_pass;     // [n_cpass][2] = {max degree in pass, A offset of pass}
    const int32_t *c_cnt_ge;   // [34] number of checks with degree >= d (zero padded)
    const int32_t *v_pass;     // [n_vpass][2] = {max degree in pass, index-table offset of pass}
    const int32_t *v_cnt_ge;   // [34]
    const int32_t *v_var;      // [n_vpass*L] variable id per slot (-1 none)
    const uint16_t *v_apos;    // [v_apos_len] A word of (pass, k, lane)
    int32_t v_apos_len;
    int32_t idx_lds_bytes;     // bytes of the block-shared LDS copy of v_apos (0 = read it from global)
    int32_t n_cpass, n_vpass;
    int32_t a_words, zero_pos;
    int32_t m, n, nwords;      // nwords = (n+31)/32 packed output words per frame
    int32_t llr_words;         // n_vpass * L
    int32_t lds_bytes_per_frame;
    // absorbed degree-1 variables (BpLayout::n_apass): the last n_apass check passes; 0 = none
    const int32_t *a_var;      // [n_apass*L] variable id per (absorbed pass, lane), -1 none
    int32_t n_apass;
};

// most absorbed check passes a fused kernel keeps in registers (two VGPRs per pass and lane)
constexpr int BP_MAX_APASS = 2;

// per-launch MC statistics (one row per launch; experiment.h:25-68)
enum { MC_CORRECT = 0, MC_PSEUDO, MC_TOTAL, MC_HAM, MC_HAM_OK, MC_HAM_WRONG, MC_ITERS, MC_NCOUNTERS };
// the counters of a detail run (acg_ldpc_mc_run_detail): the row above, then acg_ldpc_mc_detail's own sums and, per chunk,
// the packed (weight << 32 | chunk-relative frame) minimum over the pseudo frames (all ones: none)
enum { DET_WORD_FRAMES = MC_NCOUNTERS, DET_BIT_ERRORS, DET_NONCODEWORD, DET_SYNDROME, DET_MIN_PSEUDO, DET_NCOUNTERS };

struct DecodeArgs {
    // input
    const void *y;      // frames*n float or double (null in MC/device-noise mode)
    int32_t y_is_f64;
    int64_t frames;
    double inv_var2;    // 2 / sigma^2  (llr = y * inv_var2; fp64 path divides exactly like channel.h:14-16)
    double var;         // sigma^2
    // output (any may be null in MC mode)
    uint32_t *out_bits;
    uint8_t *out_ok;
    int32_t *out_iters;
    // params
    int32_t max_iter;
    int32_t early_exit;
    float ms_scale;
    int32_t phi_memo;   // fused fixed-work sum-product sweeps: the phi memo of the absorbed check passes (BpPass::phi_c); 0 = off
    // Monte-Carlo mode
    int32_t mc;          // 0 = decode y; 1 = generate y on device + classify
    uint64_t seed;
    int64_t first_frame;
    const uint32_t *cw_packed;  // n_cw * nwords, null = all-zero codeword
    int64_t n_cw;
    float sigma;
    unsigned long long *counters;  // MC_NCOUNTERS
    unsigned long long *work_counter;  // fused BP: next unassigned frame (zeroed before every launch)
    // diagnostics (streamed engine, first 64-frame tile only): raw message words after the LAST executed
    // check sweep / variable sweep, [E][64], and posteriors [n][64]; null = off
    void *dbg_c2v;
    void *dbg_v2c;
    void *dbg_post;
    // fused fixed-work sum-product (the SAT instances of bp_fused_body): a latched frame whose state recurs stops sweeping.
    // (Last in the block: the kernels that do not read them keep every argument offset.)
    // freeze_ws: FREEZE_WS_HEAD words (three 64-bit debug counters: += frames frozen << FREEZE_STATS_SHIFT | sweeps not run, then
    // at FREEZE_WS_STORES / FREEZE_WS_COMPARES the detections that only wrote a snapshot / that loaded and compared one),
    // then one snapshot slot of a_words + BP_MAX_APASS * L words per resident frame group [grid * groups per block]; null = off.
    // freeze_cfg: bits 0-11 sweeps between the latch and the first snapshot (>= 1), bits 12-23 sweeps between a snapshot and
    // the compare against it (>= 1), bit 30 no checksum gate in front of the compare (FREEZE_CFG_NO_GATE), bit 31 count.  (Three scalar registers in all: the kernel has none to spare.)
    uint32_t *freeze_ws;
    uint32_t freeze_cfg;
};
constexpr int FREEZE_WS_HEAD = 8;       // 32-bit words
constexpr int FREEZE_WS_STORES = 1;     // 64-bit words from the head's start
constexpr int FREEZE_WS_COMPARES = 2;
constexpr uint32_t FREEZE_CFG_NO_GATE = 0x40000000u;
constexpr int FREEZE_STATS_SHIFT = 40;

// One code of a batch (acg_ldpc_mc_run_codes) as the classification and symbol kernels of mc_kernels.hip see it
struct CodeRef {
    const uint32_t *cw_packed;     // n_cw * nwords sent words of THIS code, null = the all-zero word
    int64_t n_cw;
    const int32_t *row_ptr;        // its CSR (IsCodeword, experiment.h:111); unused by guard codes
    const int32_t *edge_var;
    unsigned long long *counters;  // its row of MC_NCOUNTERS
};

// ---- QP-ADMM constraint rows (qp_admm.h:34-83), shared by the streamed engine (admm_streamed.hip) and host checks ----
// A constraint group of type 3 (three variables, qp_admm.h:34-57) owns 4 consecutive rows, type 2 (:75-83) 2 rows, type 1
// (:70-74) 1 row.  Member `wpos` (its position in the group's construction, 0..2) has coefficient +1 in row `wpos` and in
// row 3, -1 in the other rows; b is 2 in row 3 of a type-3 group, 0 everywhere else.
#ifdef __HIP__
#define ACG_HD __host__ __device__
#else
#define ACG_HD
#endif
ACG_HD inline int admm_group_rows(int type) { return type == 3 ? 4 : type; }
ACG_HD inline bool admm_row_plus(int type, int row, int wpos) { return (type == 3 && row == 3) || row == wpos; }
ACG_HD inline double admm_row_b(int type, int row) { return (type == 3 && row == 3) ? 2.0 : 0.0; }

// Layered min-sum (bp_layered.hip; LayeredLayout in ldpc_internal.hpp)
struct LayerTables {
    const int32_t *layer;    // [n_layers][4] = {degree, message offset (words), checks, first proto entry | first row << 16}
    const int32_t *proto;    // quasi-cyclic H: {block column, shift} pairs per block row; null = use pos
    const int32_t *proto_packed;  // the same, one word per pair: block column * Z * 4 << 16 | shift * 4 (byte units, for the hot loop)
    const uint16_t *pos;     // any other H: [e_pad] variable of (layer, edge, lane), n = neutral cell; null when proto is set
    int32_t n_layers, Z, n, nwords;
    int32_t e_pad;           // message words per frame
    int32_t p_words;         // posterior words per frame (n + the neutral cell, rounded up)
    int32_t r_words;         // 32-bit words the e_pad messages of a frame occupy (e_pad, or half of it rounded up for fp16 storage)
    int32_t tab_lds_bytes;   // bytes of the workgroup's position table
    int32_t lds_bytes_per_frame;
};

// Workgroup-per-frame layered BP (bp_layered_block.hip, bp_layered_wide.hip, bp_layered_q.hip; LayeredBlockLayout in
// ldpc_internal.hpp).  Both tables live in device memory.  degree is 1 ... 8 for bp_layered_block_kernel, 1 ... 32 for the other two.
struct LayerBlockTables {
    // [n_steps][8]: the (set, pass) pairs of one iteration in processing order =
    //   {degree, 1 = barrier behind the step (the last pass of a set; 0 behind the last set: the round's OR is its barrier),
    //    message cell of (edge 0, thread 0), position entry of (edge 0, thread 0), checks in the pass (<= L),
    //    checks in the whole set (the distance between the position entries of consecutive edges), 0, 0}
    const int32_t *step;
    const int32_t *pos;      // [e] byte offset of the posterior cell (fp32; q: int16) of (set, edge j, slot) at set offset + j * cnt + slot
    int32_t n_steps, n_sets;
    int32_t n, nwords;
    int32_t e;               // message cells per frame = edges of the graph
    int32_t p_words;         // 32-bit words of the posterior cells: n + the neutral cell, padded to 16 bytes
    int32_t r_words;         // 32-bit words of the e message cells (fp32, fp16; q: one byte), rounded up
};

// Fixed-point layered min-sum (bp_layered_q.hip): acg_ldpc_quant as the kernel reads it
struct QuantArgs {
    float inv_step;   // (float) (1 / llr_step)
    int32_t cmax, rmax, pmax;
    int32_t scale_num, scale_shift, rnd, offset;   // rnd = 2^(scale_shift - 1), 0 for scale_shift = 0
    // the integer entrance (acg_ldpc_decode_batch_q*), read by the IO instances only.  (Last in the block, and in the one block
    // that only this kernel reads: no other argument moves.)
    const int16_t *c_in;   // frames * n channel values, clamped to +-cmax by the kernel
    int16_t *post_out;     // frames * n posteriors, written with the frame's word; null = off
};
// The grid form of the kernel (bp_layered_q_grid_kernel, acg_ldpc_mc_run_quants): an argument block of its own behind
// QuantArgs, so no argument of the other instances moves.
struct QuantGridArgs {
    const int32_t *tab;   // [points][8]: the first 32 bytes of each point's QuantArgs (inv_step ... offset)
    uint32_t fc;          // frames per point: virtual frame vf = point * fc + frame
};
// the two pointers as launch_decode takes them
struct QuantIo {
    const int16_t *c_in;
    int16_t *post_out;
};

// The streamed layered engines (bp_streamed_q.hip: fixed-point min-sum; bp_streamed_layered.hip: float sum-product and min-sum):
// the checks in processing order as a plain CSR, read through scalar loads, and the slab of a tile
struct StreamLayTables {
    const int32_t *row_ptr;    // [m + 1] first edge of the i-th check processed (the sets of bp_layered_block_build, set by set)
    const int32_t *edge_var;   // [E] variables of those edges, ascending inside a check
    int32_t m, n, E, nwords;   // m: checks with at least one variable
    int32_t max_deg;           // largest check degree: rows of the float engine's wide-check scratch
    int64_t slab_bytes;        // bytes of a tile's slab, rounded up to 256: P[n][T] int16 | R[E][T] int8, or P[n][T] | R[E][T] | scratch in fp32
};

// The LLR entrance of the streamed float layered engine (acg_ldpc_decode_batch_llr*): what the IO instances of
// bp_streamed_layered_kernel read, an argument block of their own behind ws, so no argument of the other instances moves
struct StreamLayIo {
    const float *llr_in;   // frames * n LLRs, positive = bit 0; the kernel takes NaN as +0 and clamps to +-2^20
    float *post_out;       // frames * n posterior LLRs in natural-log units, written with the frame's word; null = off
};

// Ordered-statistics decoding (osd.hip): what the kernel reads next to DecodeArgs
struct OsdArgs {
    const uint32_t *cols;   // [n][stride] H column-major, bit r % 32 of word r / 32 of column v = H[r][v]
    const int16_t *s_in;    // frames * n soft values (the integer entrance); null: the symbol entrance quantises a.y
    int32_t n, m, nwords;
    int32_t wm, stride;     // words of a column = ceil(m / 32), and their distance = wm made odd
    int32_t rank;           // rank of H over GF(2): the pivots of a frame
    int32_t order;          // 0 or 1
};

// Streamed ("HBM") BP engine: plain CSR of the Tanner graph, read through scalar loads.
struct StreamTables {
    const int32_t *row_ptr;   // [m+1] edges in check-major order (variables ascending)
    const int32_t *col_ptr;   // [n+1]
    const int32_t *col_edge;  // [E] edge ids per variable (checks ascending)
    int32_t m, n, E, nwords;
    int64_t ws_words_per_wave;  // workspace words (of 4 bytes) per wavefront
    // LDS-DMA ring engine (bp_streamed_ring_kernel, fp32): the sweeps cut into tasks of at most RING_SLOT_LINES message
    // lines; task i of a sweep belongs to wavefront i mod RING_WAVES.  int4 per task:
    //   check task {first check, checks, first line, lines | wait << 8 | wait_nostore << 16}
    //   variable task {first variable, variables, first col_ptr entry, edge lines | wait << 8 | wait_nostore << 16}
    // wait = vector-memory operations GUARANTEED to be issued behind the task's loads when its data is needed (see the kernel)
    const int32_t *ctask;
    const int32_t *vtask;
    const int32_t *vtask_of_word;  // [nwords] first variable task holding a variable >= 32 * word
    int32_t n_ctask, n_vtask;
};
#ifndef ACG_RING_SLOTS
#define ACG_RING_SLOTS 3
#endif
#ifndef ACG_RING_SLOT_LINES
#define ACG_RING_SLOT_LINES 16
#endif
#ifndef ACG_RING_MAX_PER_CU
#define ACG_RING_MAX_PER_CU 4
#endif
constexpr int RING_WAVES = 4;        // wavefronts per workgroup of the ring engine
constexpr int RING_SLOTS = ACG_RING_SLOTS;            // ring slots per wavefront (tasks in flight: RING_SLOTS - 1 ahead of the one computed)
constexpr int RING_SLOT_LINES = ACG_RING_SLOT_LINES;  // 256-byte lines per slot
constexpr int RING_VAR_EDGE_LINES = RING_SLOT_LINES - 4;  // variable task: edge lines + up to 4 LLR lines
constexpr int RING_MAX_CDEG = RING_SLOT_LINES < 16 ? RING_SLOT_LINES : 16;          // a node must fit in one slot
constexpr int RING_MAX_VDEG = RING_VAR_EDGE_LINES < 12 ? RING_VAR_EDGE_LINES : 12;  // (and in the kernels' degree switches)
constexpr int RING_LDS_BYTES = RING_WAVES * RING_SLOTS * RING_SLOT_LINES * 256;
// the counted waits must stay within the 6-bit vmcnt field: (slots - 1) tasks of loads + stores behind a task's loads
static_assert((RING_SLOTS - 1) * (RING_SLOT_LINES + RING_SLOT_LINES / 4 + 1) <= 63, "ring too deep for vmcnt");

}  // namespace acg
