// Every function that one .hip file defines and another calls, declared once.  Both the caller and the defining file
// include this header, so a definition that drifts from its declaration does not compile.  Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/acg_ldpc.h"
#include "kernels.hpp"

namespace acg {

struct Code;  // ldpc_internal.hpp

// ---- bp_inst_{spa,ms}_{f32,f64}.hip: the instances of bp_fused_kernel (bp_core.inc) ----
const void *bp_kernel_ptr_spa_f32(int maxd, int L, bool mc, int variant, bool sat, bool split = false);
const void *bp_kernel_ptr_spa_f64(int maxd, int L, bool mc, int variant);
const void *bp_kernel_ptr_ms_f32(int maxd, int L, bool mc, int variant);
const void *bp_kernel_ptr_ms_f64(int maxd, int L, bool mc, int variant);
const void *bp_kernel_ptr_spa_f32_dbg(int L, int sat = 0);
const void *bp_kernel_ptr_spa_f64_dbg(int L);

// ---- bp_inst_spec.hip: build-time instances with a code's pass structure constant (bp_spec.hpp) ----
struct BpLayout;  // ldpc_internal.hpp
const void *bp_spec_kernel_ptr(const BpLayout &lay, bool mc, const char **name, const char **sat_rows = nullptr, bool split = false,
                               const char **split_rows = nullptr);

// ---- bp_kernels.hip ----
const void *bp_kernel_ptr(int algo, int f64, int maxd, int L, bool mc, int variant, bool sat, bool split = false);
const void *bp_kernel_ptr_dbg(int f64, int L, int sat = 0);
hipError_t bp_launch(const void *kernel, const BpTables &t, const DecodeArgs &a, int grid, int block, size_t lds,
                     hipStream_t s);
hipError_t phi_debug_launch(const void *x, void *out, int n, int f64, hipStream_t s);
hipError_t phi_sat_debug_launch(const float *x, uint32_t *out, int n, hipStream_t s);
constexpr int PHI_SPLIT_NOUT = 6;  // words of phi_split_debug_launch's result (bp_kernels.hip: phi_split_debug_kernel)
hipError_t phi_split_debug_launch(uint32_t *out, hipStream_t s);

// ---- mc_kernels.hip ----
hipError_t awgn_launch(float *y, int64_t frames, int n, int nwords, int64_t first_frame, uint64_t seed,
                       const uint32_t *cw_packed, int64_t n_cw, float sigma, hipStream_t s);
// detail run (acg_ldpc_mc_run_detail): counters = DET_NCOUNTERS words, kind = one byte per frame of the chunk
hipError_t classify_detail_launch(const float *y, const uint32_t *bits, const uint8_t *ok, const int32_t *iters, int64_t frames,
                                  int n, int nwords, int64_t first_frame, const uint32_t *cw_packed, int64_t n_cw,
                                  unsigned long long *counters, uint8_t *kind, const int32_t *row_ptr, const int32_t *edge_var, int m,
                                  hipStream_t s);
hipError_t gather_events_launch(const int32_t *sel, int n_sel, const float *y, const uint32_t *bits, const uint8_t *ok,
                                const int32_t *iters, const uint8_t *kind, int n, int nwords, int64_t first_frame,
                                const uint32_t *cw_packed, int64_t n_cw, const int32_t *row_ptr, const int32_t *edge_var, int m,
                                acg_ldpc_mc_event *events, uint32_t *words, hipStream_t s);
// classification of units x frames virtual frames: the codes of a batch; the points of a grid (one point: acg_ldpc_mc_run)
hipError_t classify_codes_launch(const void *y, int y_is_f64, const uint32_t *bits, const uint8_t *ok, const int32_t *iters,
                                 int64_t frames, int64_t codes, int n, int nwords, int64_t first_frame, const CodeRef *refs, int m,
                                 hipStream_t s);
hipError_t codes_symbols_launch(const double *noise, double *y, int64_t frames, int64_t codes, int n, int nwords, int64_t first_frame,
                                const CodeRef *refs, hipStream_t s);
hipError_t classify_grid_launch(const void *y, int y_is_f64, const uint32_t *bits, const uint8_t *ok, const int32_t *iters,
                                int64_t frames, int64_t points, int n, int nwords, int64_t first_frame, const uint32_t *cw_packed,
                                int64_t n_cw, unsigned long long *counters, const int32_t *row_ptr, const int32_t *edge_var, int m,
                                hipStream_t s);

// ---- mc_rm_kernels.hip: Monte-Carlo for punctured / shortened codes (acg_ldpc_mc_run_rm) ----
// noise -> symbol -> channel value of frames x n positions in one pass: fp32 LLRs (q == null; inv_var2 = 2 / sigma^2) or q's
// int16 channel values into out; pattern: n bytes of ACG_LDPC_RM_*, null = all sent; raw (may be null): frames raw-error
// counts, zeroed here on s
hipError_t rm_channel_launch(void *out, const QuantArgs *q, int32_t *raw, int64_t frames, int n, int nwords, int64_t first_frame,
                             uint64_t seed, const uint32_t *cw_packed, int64_t n_cw, float sigma, double inv_var2, const uint8_t *pattern,
                             hipStream_t s);
// classify_grid_launch for one decoder, with raw[f] in place of the Hamming count over the symbols
hipError_t classify_rm_launch(const int32_t *raw, const uint32_t *bits, const uint8_t *ok, const int32_t *iters, int64_t frames, int n,
                              int nwords, int64_t first_frame, const uint32_t *cw_packed, int64_t n_cw, unsigned long long *counters,
                              hipStream_t s);

// ---- cascade_kernels.hip: the glue of a two-stage decode, per chunk of frames (an int32 count: at most 65536) ----
// idx[0 .. *count) = the frames with ok == 0, ascending; stage (may be null) = 1 for every frame.  idx: `frames` entries
hipError_t cascade_select_launch(const uint8_t *ok, int32_t frames, int32_t *idx, int32_t *count, uint8_t *stage, hipStream_t s);
// row k of out = row idx[k] of y, rows of n symbols of elem = 4 or 8 bytes (2: the int16 posteriors of a quantized stage)
hipError_t cascade_gather_launch(const void *y, int elem, int32_t n, const int32_t *idx, int32_t K, void *out, hipStream_t s);
// rows idx[k] of bits / ok / iters (may be null) / stage (may be null, = 2) from row k of the compact outputs
hipError_t cascade_scatter_launch(const uint32_t *cbits, const uint8_t *cok, const int32_t *citers, const int32_t *idx, int32_t K,
                                  int32_t nwords, uint32_t *bits, uint8_t *ok, int32_t *iters, uint8_t *stage, hipStream_t s);
// *sum += iters[0 .. K)
hipError_t cascade_sum_iters_launch(const int32_t *iters, int32_t K, unsigned long long *sum, hipStream_t s);

// ---- bp_block.hip, bp_pair.hip, bp_layered.hip ----
const void *bp_block_kernel_ptr(int algo, int f64, int L, bool mc, bool idxlds, bool idxreg, bool regular);
const void *bp_block_kernel_ptr_dbg(int f64);
const void *bp_pair_kernel_ptr(int L, bool regular);
const void *bp_layered_kernel_ptr(int G, int waves, bool qc_arith, bool f16, int algo, bool mc);
hipError_t bp_layered_launch(const void *kernel, const LayerTables &t, const DecodeArgs &a, int grid, int block, size_t lds, hipStream_t s);

// ---- the workgroup-per-frame layered kernels: bp_layered_block.hip (check degree <= 8; L = 256, 512, 1024), bp_layered_wide.hip
// (<= 32, the same tables) and bp_layered_q.hip (fixed-point min-sum, <= 32; L = 64, 128, 256, 512, 1024) ----
const void *bp_layered_block_kernel_ptr(int L, bool f16, int algo);
const void *bp_layered_wide_kernel_ptr(int L, bool f16, int algo);
// io: the instance of the integer entrance (QuantArgs::c_in in, QuantArgs::post_out out) instead of the symbol entrance's
const void *bp_layered_q_kernel_ptr(int L, bool io);
// the grid form of the symbol entrance: a quantiser per virtual frame (QuantGridArgs, acg_ldpc_mc_run_quants)
const void *bp_layered_q_grid_kernel_ptr(int L);
// q: the quantiser of bp_layered_q_kernel, null for the float kernels; g: the fourth argument of bp_layered_q_grid_kernel
hipError_t bp_layered_wg_launch(const void *kernel, const LayerBlockTables &t, const DecodeArgs &a, const QuantArgs *q, int grid, int block,
                                size_t lds, hipStream_t s, const QuantGridArgs *g = nullptr);
// the kernel's quantiser on `count` symbols (a: y, y_is_f64 and the channel terms) -> count int16
hipError_t quantize_debug_launch(const DecodeArgs &a, const QuantArgs &q, int64_t count, int16_t *out, hipStream_t s);

// ---- bp_streamed_q.hip: streamed fixed-point layered min-sum, a wavefront per tile of 64 frames ----
const void *bp_streamed_q_kernel_ptr();

// ---- bp_streamed_layered.hip: streamed float layered BP, a wavefront per tile of 64 frames ----
// algo: 0 sum-product, 1 min-sum; io: the instance of the LLR entrance (StreamLayIo: LLRs in, posteriors out) instead of the symbol entrance's
const void *bp_streamed_layered_kernel_ptr(int algo, bool io = false);
// fp32 words per frame behind P and R: the scratch of a wide sum-product check (0: max_deg <= 8, or min-sum)
size_t bp_streamed_layered_scratch_words(int algo, int max_deg);
bool bp_streamed_layered_stores_mag();   // pass 2 of a wide sum-product check reads mag back (or forms it again)
// either engine.  q: the quantiser of bp_streamed_q_kernel with c_in set (and post_out, or null), null for the float kernels; ws:
// grid slabs of t.slab_bytes; io: the last argument of the float kernels' IO instances, null for every other kernel
hipError_t bp_streamed_layered_launch(const void *kernel, const StreamLayTables &t, const DecodeArgs &a, const QuantArgs *q, unsigned char *ws,
                                      int grid, hipStream_t s, const StreamLayIo *io = nullptr);

// ---- osd.hip: ordered-statistics decoding, one workgroup of L = 64, 128 or 256 threads per frame ----
const void *osd_kernel_ptr(int L);
size_t osd_lds_bytes(int n, int m);   // dynamic LDS of a workgroup
hipError_t osd_launch(const void *kernel, const OsdArgs &o, const DecodeArgs &a, int grid, int block, size_t lds, hipStream_t s);
// the symbol entrance's quantiser on `count` symbols -> count int16
hipError_t osd_soft_debug_launch(const void *y, int y_is_f64, int64_t count, int16_t *out, hipStream_t s);

// ---- bp_streamed.hip ----
const void *bp_streamed_ptr(int algo, int f64);
const void *bp_streamed_ring_ptr(int algo, bool nt);
const void *bp_streamed_ring_ptr_dbg();
hipError_t bp_streamed_ring_launch(const void *kernel, const StreamTables &t, const DecodeArgs &a, uint32_t *ws, int grid, hipStream_t s);
hipError_t bp_streamed_launch(const void *kernel, const StreamTables &t, const DecodeArgs &a, uint32_t *ws, int grid,
                              int block, hipStream_t s);

// ---- admm_kernels.hip (AdmmDevice stays opaque to its callers) ----
struct AdmmDevice;
AdmmDevice *admm_device_create(const Code &c, const acg_ldpc_params &p, int cu_count, std::string &err);
void admm_device_destroy(AdmmDevice *d);
hipError_t admm_launch(AdmmDevice *d, const DecodeArgs &a, hipStream_t s, std::string &err);
void admm_device_layout(const AdmmDevice *d, int *lds_per_frame, int *lanes, int *frames_per_block, int *grid);
bool admm_device_unfused_mc(const AdmmDevice *d, const int32_t **row_ptr, const int32_t **edge_var);
bool admm_device_streamed(const AdmmDevice *d, int *slabs, int64_t *slab_bytes, int *f32);
// parameter grid (acg_ldpc_mc_run_grid)
double admm_device_e_min(const AdmmDevice *d);
bool admm_device_has_grid_kernel(const AdmmDevice *d);
void admm_grid_tables(const AdmmDevice *d, const double *alpha, const double *mu, int np, std::vector<unsigned char> &pt,
                      std::vector<unsigned char> &inv);
void admm_grid_bind(AdmmDevice *d, const void *pt_dev, const void *inv_dev, uint32_t frames_per_point);
bool admm_device_set_point(AdmmDevice *d, double alpha, double mu, std::string &err);
// batch of codes (acg_ldpc_mc_run_codes): a plan is an AdmmDevice whose tables lie in a host blob (see admm_kernels.hip)
AdmmDevice *admm_codes_plan(const Code &c, const acg_ldpc_params &p, std::vector<unsigned char> &blob, std::string &err);
int admm_codes_shape(const AdmmDevice *d);
size_t admm_codes_lds(const AdmmDevice *d);
size_t admm_codes_tables_bytes();
void admm_codes_csr(const AdmmDevice *d, size_t *row_ptr_off, size_t *edge_var_off);
void admm_codes_tables(const AdmmDevice *d, uintptr_t base, void *out);
int admm_codes_grid_cap(const AdmmDevice *d, size_t lds, int cu_count, std::string &err);
hipError_t admm_codes_launch(const AdmmDevice *d, const void *tabs_dev, uint32_t frames_per_code, size_t lds, int grid_cap,
                             const DecodeArgs &a, hipStream_t s);

// ---- admm_streamed.hip (called by admm_kernels.hip) ----
struct AdmmStream;
AdmmStream *admm_stream_create(const Code &c, const acg_ldpc_params &p, int cu_count, std::string &err);
void admm_stream_destroy(AdmmStream *s);
void admm_stream_info(const AdmmStream *s, int *slabs, int64_t *slab_bytes, int *f32);
bool admm_stream_set_point(AdmmStream *s, double alpha, double mu);
hipError_t admm_stream_launch(AdmmStream *s, const DecodeArgs &a, hipStream_t st);

}  // namespace acg
