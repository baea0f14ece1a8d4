/*
 * acg_ldpc.h — C ABI of the MI355X-native batched LDPC decoder (libacg_ldpc_hip.so).
 *
 * Drop-in boundary for ONE path of GreatDrake/acg-alp-ldpc: the per-frame call
 *     pair<TCodeword,bool> Decoder::decode(const TMatrix &H, const TFVector &y, double snr)
 * (reference algo/algo.h:8) as implemented by BeliefPropagationDecoder (algo/bp.h:208-222) and
 * QPADMMDecoder (algo/qp_admm.h:180-194), plus the Monte-Carlo loop that drives it
 * (experiment.h:80-139) with its AWGN generator (utils/channel.h:18-26).
 *
 * Plain C: opaque handles, caller-owned buffers, int return codes (0 = ok), no exceptions,
 * no torch / STL types.  Every entry point cites the reference interface it replaces.
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Threading: a decoder handle owns one HIP stream + workspace on one device; host calls on the same
 * handle are serialised by an internal mutex (the reference calls one decoder object from
 * THREADS_NUM pthreads, experiment.h:101,127-130 — that keeps working, one handle per thread
 * is faster).  Code handles are immutable after creation and may be shared.
 * Streams: acg_ldpc_decode_batch_dev is asynchronous on the caller's stream.  Launches of ONE handle on
 * DIFFERENT streams may overlap on the device: each launch owns its work counter (a ring of 32 per handle,
 * a slot is reused only behind the launch that held it).  The streamed BP engine keeps its message slabs
 * in the handle, so its launches are ordered on the device (a launch on another stream waits for the
 * previous one through an event) — correct, not concurrent; use one handle per stream to overlap those.  The same holds
 * for the streamed QP-ADMM engine.
 */
#ifndef ACG_LDPC_H
#define ACG_LDPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct acg_ldpc_code acg_ldpc_code;       /* parity-check matrix + analysed Tanner graph (host) */
typedef struct acg_ldpc_decoder acg_ldpc_decoder; /* device-resident graph, workspace, stream, params */

/* algorithm selector */
enum {
    ACG_LDPC_BP_SUMPRODUCT = 0, /* algo/bp.h — the reference's BP (phi-domain sum-product) */
    ACG_LDPC_BP_MINSUM = 1,     /* build-added (north_star); NOT in the reference: parity unpinned */
    ACG_LDPC_QPADMM = 2,        /* algo/qp_admm.h */
    ACG_LDPC_OSD = 3            /* build-added: ordered-statistics decoding, order max_iter = 0 or 1 (see "OSD" below) */
};

/* arithmetic selector */
enum {
    ACG_LDPC_PREC_DEFAULT = 0, /* BP: fp32 messages; QP-ADMM: fp64 */
    ACG_LDPC_PREC_F64 = 1,     /* everything fp64 */
    ACG_LDPC_PREC_F32 = 2,     /* everything fp32 (QP-ADMM then matches FER only) */
    ACG_LDPC_PREC_F16 = 3      /* min-sum only (build-added variant, parity unpinned): half-precision messages, two frames
                                  per workgroup sharing every LDS word, index and barrier — for codes whose messages fill
                                  the LDS of a CU (check degree <= 8, variable degree <= 4, n <= 12288) */
};

/* engine selector (BP and QP-ADMM) */
enum {
    ACG_LDPC_ENGINE_AUTO = 0,     /* fused when a frame's state fits in LDS, else streamed.  QP-ADMM: the LDS kernels for every
                                     code they accept (lanes_per_frame 0); the streamed engine only where they refuse the code
                                     because its frame state does not fit in LDS */
    ACG_LDPC_ENGINE_FUSED = 1,    /* state resident in LDS for the whole decode (HBM: symbols in, bits out); a code too
                                     large for it is refused */
    ACG_LDPC_ENGINE_STREAMED = 2  /* state [row][frame] in HBM, one lane per frame, coalesced sweeps (any code size).
                                     BP: messages per edge.  QP-ADMM: w per constraint row, v, and the channel term; needs
                                     lanes_per_frame = 0.  Workspace: one slab of (C + n_var + n) x 64 words (8 bytes fp64, 4
                                     fp32; C constraint rows and n_var variables of acg_ldpc_code_admm_shape) per
                                     workgroup, min(2 x CU count, slabs fitting in a quarter of the free device memory,
                                     at least one) slabs, hipMalloc'ed when the decoder is created (configs[4], 5000 x 10000
                                     (3,6)-regular, fp64: 58.9 MB per slab, 512 slabs = 30.1 GB on an MI355X).  Creation
                                     fails when not even one slab fits. */
};

/* BP message schedule */
enum {
    ACG_LDPC_SCHEDULE_FLOODING = 0, /* the reference's schedule (bp.h:183-199): all checks, then all variables */
    ACG_LDPC_SCHEDULE_LAYERED = 1   /* build-added: the block rows of a quasi-cyclic H (or, for any other H, groups
                                       of checks that share no variable) are processed in sequence and the posteriors are
                                       updated in place after every layer, so one iteration does the work of about two
                                       flooding sweeps.  A DIFFERENT algorithm from the reference's BeliefPropagationDecoder:
                                       parity is FER-level only.  With ACG_LDPC_BP_MINSUM: normalised min-sum (parity unpinned
                                       anyway); with ACG_LDPC_BP_SUMPRODUCT: the reference's check rule (bp.h:49-57) in the
                                       layered message order — the reference's FER at about half its iterations.  fp32
                                       posteriors; messages fp32, or fp16 with ACG_LDPC_PREC_F16.
                                       Three engines.  Check degree <= 8, lanes_per_frame 0: 16, 20, 32 or 64 lanes of a
                                       wavefront per frame (bp_layered_kernel; n < 16000, a few thousand edges).
                                       Check degree <= 8, lanes_per_frame 256, 512 or 1024: one workgroup per frame
                                       (bp_layered_block_kernel) — posteriors + messages + output word of ONE frame within the
                                       160 KiB of LDS, i.e. (n + 4) * 4 + E * 4 (E * 2 with fp16 messages) + n / 8 bytes for E
                                       edges; a Monte-Carlo run on it goes noise kernel -> decode -> classification kernel.
                                       Pass 1024 for codes of tens of thousands of edges: 0 selects the workgroup engine by
                                       itself only where the wavefront-group kernel refuses the code for its size.
                                       Largest check degree 9 ... 32 (high-rate codes): one workgroup per frame with wide
                                       checks worked off in chunks of 8 edges (bp_layered_wide_kernel), for every
                                       lanes_per_frame it takes — 256, 512, 1024, or 0 = the smallest of the three that holds
                                       the largest set of checks, else 1024; the same LDS rule and Monte-Carlo path as the
                                       other workgroup engine.  A check of more than 32 variables is refused. */
};

/* noise source for acg_ldpc_mc_run */
enum {
    ACG_LDPC_NOISE_DEVICE_PHILOX = 0, /* counter-based, keyed on (seed, global frame, symbol): same
                                         frames for any GPU count; statistically validated only */
    ACG_LDPC_NOISE_HOST_MT19937 = 1   /* bit-exact experiment.h:97-99: frame i <- mt19937(i+1) +
                                         libstdc++ normal_distribution, generated on the host */
};

typedef struct acg_ldpc_params {
    int32_t algo;       /* ACG_LDPC_* */
    int32_t max_iter;   /* BeliefPropagationDecoder(max_iter) bp.h:210 / QPADMMDecoder max_iter qp_admm.h:182 */
    double alpha;       /* QP-ADMM (qp_admm.h:182) */
    double mu;          /* QP-ADMM */
    double eps_stop;    /* QP-ADMM residual threshold (qp_admm.h:161) */
    double ms_scale;    /* min-sum normalisation factor (1.0 = plain) */
    int32_t early_exit; /* 1 = reference semantics: stop a frame at its first zero syndrome (bp.h:195-196)
                           / residual < eps (qp_admm.h:161).  0 = fixed work: run max_iter sweeps for every
                           frame, output LATCHED at the first zero syndrome (identical results). */
    int32_t precision;  /* ACG_LDPC_PREC_* */
    int32_t device;     /* HIP device ordinal; -1 = current device */
    int32_t lanes_per_frame; /* 0 = auto; 16/32/64: that many lanes of a wavefront cooperate on one frame; 256 (BP also
                                1024): one workgroup per frame (QP-ADMM then picks 128, 192 or 256 threads itself).
                                ACG_LDPC_SCHEDULE_LAYERED: 0 (check degree <= 8: the layering picks the lanes of a wavefront
                                group; 9 ... 32: the smallest workgroup that holds the largest set), or 256, 512, 1024 = one
                                workgroup of that many threads per frame (check degree <= 32) */
    int32_t engine;     /* ACG_LDPC_ENGINE_* (BP and QP-ADMM) */
    int32_t fast_setup; /* 0 = default: spend up to ~1 s per decoder on the static LDS placement of the QP-ADMM kernel
                           (bank-conflict search; cached per parity-check matrix inside the process);
                           1 = skip that search (throw-away decoders, e.g. one per proposal of the check-matrix local
                           search, optimize_H.cpp:89-104).  Results are identical either way. */
    int32_t schedule;   /* ACG_LDPC_SCHEDULE_* (BP only; default flooding) */
} acg_ldpc_params;

void acg_ldpc_params_default(acg_ldpc_params *p);

/* last error message of the calling thread ("" if none).  The reference aborts via assert();
 * here every failure is an error code + message and nothing is silently computed on the CPU. */
const char *acg_ldpc_last_error(void);

/* 1 if a HIP device is usable from this process, 0 otherwise (never falls back to a CPU decode). */
int acg_ldpc_device_available(void);

/* ---- parity-check matrix --------------------------------------------------------------- */

/* replaces: TMatrix (utils/codeword.h:18) handed to decode() on every call; analysed once here
 * (the reference re-scans H per frame: bp.h:136-153, qp_admm.h:15-21,60-66). H: m*n bytes, !=0 -> 1. */
int acg_ldpc_code_from_dense(const uint8_t *H, int32_t m, int32_t n, acg_ldpc_code **out);
/* replaces read_pcm (utils/parse_data.h:6-25), same quirks */
int acg_ldpc_code_load_txt(const char *path, acg_ldpc_code **out);
/* replaces save_matrix (utils/parse_data.h:44-54) */
int acg_ldpc_code_save_txt(const acg_ldpc_code *code, const char *path);
void acg_ldpc_code_destroy(acg_ldpc_code *code);
/* m checks, n variables, E edges (ones of H) */
void acg_ldpc_code_dims(const acg_ldpc_code *code, int32_t *m, int32_t *n, int32_t *E);
/* dense copy back (m*n bytes) */
void acg_ldpc_code_dense(const acg_ldpc_code *code, uint8_t *H);
/* QP-ADMM problem shape of ConstructADMMProblem (qp_admm.h:13-102) */
void acg_ldpc_code_admm_shape(const acg_ldpc_code *code, int32_t *n_var, int32_t *n_con, int32_t *nnz,
                              double *e_min, double *e_max);
/* replaces GetOrtogonal (utils/codeword.h:97-128): G must hold (n-m)*n bytes; returns 0 ok,
 * 1 if a row of H vanishes during elimination (the reference's {TMatrix(), false}). */
int acg_ldpc_code_generator(const acg_ldpc_code *code, uint8_t *G);
/* replaces IsCodeword (utils/codeword.h:90-95): 1 / 0 */
int acg_ldpc_code_is_codeword(const acg_ldpc_code *code, const uint8_t *bits);

/* ---- decoder --------------------------------------------------------------------------- */

/* replaces make_shared<BeliefPropagationDecoder>(it) / make_shared<QPADMMDecoder>(a,mu,it,eps)
 * (main.cpp:28-40).  Fails (non-zero) when no HIP device is present. */
int acg_ldpc_decoder_create(const acg_ldpc_code *code, const acg_ldpc_params *params, acg_ldpc_decoder **out);
void acg_ldpc_decoder_destroy(acg_ldpc_decoder *dec);
/* replaces Decoder::name() (algo/algo.h:10): "BP" (bp.h:218), "QP-ADMM" (qp_admm.h:189), "MS"; "QMS" for a handle of
 * acg_ldpc_decoder_create_quantized or acg_ldpc_decoder_create_quantized_streamed */
const char *acg_ldpc_decoder_name(const acg_ldpc_decoder *dec);

/* ---- fixed-point layered min-sum (build-added; not in the reference) ------------------------ */

/* The quantiser of the integer layered min-sum engine (bp_layered_q_kernel): every value of the decoder is an integer, so a
 * restatement (tests/layered_q_ref.py) matches word, flag and exit iteration of every frame.
 *   channel     c = clamp(round-half-even(llr32 * (float) (1 / llr_step)), -Cmax, +Cmax), llr32 the fp32 channel LLR the float
 *               layered engines form ((float) (2 y / sigma^2) for double symbols, (float) ((double) y * (2 / sigma^2)) for float
 *               symbols), the product ONE fp32 multiply; NaN -> 0, +-inf -> +-Cmax.  Posterior P = c, every message R = 0.
 *   one check   q_j = P_j - R_j; a_j = min(|q_j|, Rmax); m1 <= m2 the two smallest a_j (a check of ONE variable: m2 = Rmax);
 *               mu_j = (a_j == m1) ? m2 : m1; mu'_j = max(((mu_j * scale_num + rnd) >> scale_shift) - offset, 0) with
 *               rnd = 2^(scale_shift - 1) (0 for scale_shift = 0); R'_j = +-mu'_j, negative where the XOR of the signs (q < 0)
 *               of the OTHER edges is 1; P'_j = clamp(q_j + R'_j, -Pmax, +Pmax).
 *   decision    P < 0 decides 1; P = 0 decides 0.
 * Schedule, stopping rule, latching, the final syndrome pass and the iteration count are those of the layered workgroup engines
 * (ACG_LDPC_SCHEDULE_LAYERED above) over the sets acg_ldpc_debug_layers_wide reports. */
typedef struct acg_ldpc_quant {      /* 32 bytes */
    double  llr_step;     /* LLR per integer unit, finite, > 0 */
    int32_t ch_bits;      /* channel value clipped to +-(2^(ch_bits-1) - 1)   = +-Cmax; 2 <= ch_bits <= post_bits */
    int32_t msg_bits;     /* check->variable messages, +-(2^(msg_bits-1) - 1) = +-Rmax; 2 <= msg_bits <= 8, msg_bits <= post_bits */
    int32_t post_bits;    /* posteriors, +-(2^(post_bits-1) - 1)              = +-Pmax; post_bits <= 16 */
    int32_t scale_num;    /* normalisation scale_num / 2^scale_shift, rounded half up; 1 <= scale_num <= 2^scale_shift */
    int32_t scale_shift;  /* 0 <= scale_shift <= 8 */
    int32_t offset;       /* subtracted after scaling, floor at 0; 0 <= offset <= Rmax */
} acg_ldpc_quant;
/* llr_step 0.5, ch_bits 6, msg_bits 6, post_bits 8, scale 1 / 2^0, offset 1: offset-1 min-sum */
void acg_ldpc_quant_default(acg_ldpc_quant *q);
/* host only, no device needed: 0 if *q obeys every rule written next to the fields above, else non-zero with the rule in
 * acg_ldpc_last_error */
int acg_ldpc_quant_check(const acg_ldpc_quant *q);
/* A decoder on the integer engine: one workgroup per frame, LDS = int16 posteriors + one byte per edge + the output word
 * (acg_ldpc_decoder_layout reports the bytes).  The only way to it; acg_ldpc_decoder_create never selects it.  Required of
 * *params, anything else is refused with a message and nothing is launched:
 *   algo = ACG_LDPC_BP_MINSUM, schedule = ACG_LDPC_SCHEDULE_LAYERED, precision = ACG_LDPC_PREC_DEFAULT,
 *   engine = ACG_LDPC_ENGINE_AUTO or ACG_LDPC_ENGINE_FUSED,
 *   lanes_per_frame 0, 64, 128, 256, 512 or 1024 = threads of the workgroup that owns a frame (0: the smallest of the five that
 *   holds the largest set of checks, else 1024).
 * ms_scale is IGNORED: the normalisation is scale_num / 2^scale_shift and offset of *q.  max_iter, early_exit and device apply
 * as everywhere.  Also refused: an invalid *q (acg_ldpc_quant_check), a check of more than 32 variables, a frame whose state
 * does not fit in LDS.
 * The handle is an ordinary decoder: acg_ldpc_decode_batch, _f32 and _dev take symbols + snr; acg_ldpc_mc_run and
 * acg_ldpc_mc_run_detail go noise kernel -> decode -> classification kernel; acg_ldpc_mc_run_grid refuses it as it refuses every
 * decoder that is not QP-ADMM; acg_ldpc_decoder_name returns "QMS"; acg_ldpc_decoder_describe names the kernel, the workgroup,
 * sets and steps and the seven values of *q.
 * What a number format costs: acg_ldpc_mc_run_quants (declared with the Monte-Carlo calls below) runs acg_ldpc_mc_run for a
 * whole list of quantisers on ONE such handle, frames of different quantisers sharing a launch. */
int acg_ldpc_decoder_create_quantized(const acg_ldpc_code *code, const acg_ldpc_params *params, const acg_ldpc_quant *q,
                                      acg_ldpc_decoder **out);
/* diagnostics: the engine's quantiser, run on the device, on `count` host symbols (doubles if y_is_f64, else floats) at `snr`;
 * out_host receives count int16 channel values */
int acg_ldpc_debug_quantize(const void *y_host, int32_t y_is_f64, int64_t count, double snr, const acg_ldpc_quant *q,
                            int16_t *out_host);

/* The integer entrance of the engine: channel values in, posteriors out.  For bit-true work against another implementation of
 * the rules above, for channel values from one's own demapper or quantiser, and for channels that symbols + snr cannot express.
 *   channel value in   a frame is n int16_t values c_v; the decoder starts from P_v = clamp(c_v, -Cmax, +Cmax) (so -32768
 *                      becomes -Cmax) and every message from 0: exactly the state the symbol entrance reaches when its
 *                      quantiser yields the same P.  llr_step plays no part and there is no snr.
 *                      A punctured position is c = 0; a shortened one c = +Cmax (known 0) or -Cmax (known 1).  Nothing special
 *                      is done for them: they are channel values like any other.
 *   posterior out      a frame's posterior is n int16_t values P_v, |P_v| <= Pmax, read at the moment the frame's word, flag
 *                      and iteration are written: for a frame that latches, the posteriors of the round boundary at which its
 *                      word is formed — with early_exit = 0 the frame is swept on, the posterior written is still the latched
 *                      one; for a frame that fails, the posteriors after max_iter iterations (its word is zeros as everywhere);
 *                      for max_iter = 0 the clamped channel value.  So (post < 0) is the word of every frame with ok = 1.
 * All three take a handle of acg_ldpc_decoder_create_quantized or acg_ldpc_decoder_create_quantized_streamed only.  Each returns non-zero, leaves a message in
 * acg_ldpc_last_error and launches nothing for a null handle, a handle of acg_ldpc_decoder_create, frames (count) < 0, or
 * frames (count) > 0 with a null input (the host call: also null bits or ok).  frames == 0 is a no-op that returns 0. */

/* the handle's quantiser on the device: count symbols -> count channel values (what acg_ldpc_debug_quantize computes,
 * asynchronous on `stream`; NULL = the handle's own stream) */
int acg_ldpc_quantize_dev(acg_ldpc_decoder *dec, const void *y_dev, int32_t y_is_f64, int64_t count, double snr, int16_t *c_dev,
                          void *stream);
/* acg_ldpc_decode_batch_dev with channel values in and, if post_dev != NULL, frames*n int16 posteriors out: the same launch
 * path, so the work-counter ring, the event pair and the stream rules at the top of this header hold for it */
int acg_ldpc_decode_batch_q_dev(acg_ldpc_decoder *dec, const int16_t *c_dev, int64_t frames, uint32_t *bits_dev, uint8_t *ok_dev,
                                int32_t *iters_dev, int16_t *post_dev, void *stream);
/* host buffers, through the pipelined two-set staging path of acg_ldpc_decode_batch (2 bytes in per value; 2 more out per value
 * when post is given); post may be NULL */
int acg_ldpc_decode_batch_q(acg_ldpc_decoder *dec, const int16_t *c, int64_t frames, uint8_t *bits, uint8_t *ok, int32_t *iters,
                            int16_t *post);

/* ---- streamed fixed-point layered min-sum: any code size, any check degree (build-added) ---- */

/* The arithmetic, schedule, stopping rule, latching, final syndrome pass and iteration count of acg_ldpc_decoder_create_quantized
 * — word, flag, iteration and posterior of every frame are equal on every code both accept — with a frame's state in device
 * memory instead of LDS (bp_streamed_q_kernel): one lane is one frame, a wavefront owns a tile of T frames and walks the edges
 * of a check in a loop, so neither the size of a frame nor the degree of a check is bounded.  State of a frame: 2 n + E bytes
 * (int16 posteriors, one byte per edge).  The checks are taken in the order of the sets acg_ldpc_debug_layers_any reports,
 * set by set.  tests/streamed_q_ref.py restates it.
 * Required of *params, anything else is refused with a message before a device is looked for:
 *   algo = ACG_LDPC_BP_MINSUM, schedule = ACG_LDPC_SCHEDULE_LAYERED, precision = ACG_LDPC_PREC_DEFAULT,
 *   engine = ACG_LDPC_ENGINE_AUTO or ACG_LDPC_ENGINE_STREAMED (ACG_LDPC_ENGINE_FUSED is refused), lanes_per_frame = 0,
 *   and a *q that acg_ldpc_quant_check accepts.  ms_scale is ignored as above.
 * Workspace: one allocation of tiles x (T (2 n + E) bytes, rounded up to 256), T = 64, tiles = min(12 per compute unit, what fits
 * in a quarter of the device's free memory); creation fails with a message when not one tile fits.  ACG_STREAMQ_TILES=<count>
 * (developer switch, read at creation) lowers the tile count.  The symbol entrances quantise into a staging buffer of the handle
 * (2 n bytes per frame, at most tiles x T frames at a time) and run the integer path.
 * The handle is an ordinary quantized handle: acg_ldpc_decode_batch, _f32, _dev, acg_ldpc_decode_batch_q, _q_dev and
 * acg_ldpc_quantize_dev take it; acg_ldpc_mc_run and _detail go noise kernel -> decode -> classification kernel;
 * acg_ldpc_mc_run_quants and acg_ldpc_mc_run_grid refuse it with a message.  The workspace belongs to the handle, so launches
 * of one handle on different streams are ordered on the device.  acg_ldpc_decoder_name returns "QMS"; acg_ldpc_decoder_layout
 * reports as for the streamed engines (no LDS bytes, one lane per frame, T frames per block, tiles); acg_ldpc_decoder_describe
 * names the kernel, T, the tiles, the bytes of state per frame, the sets and the seven values of *q.
 * A code whose frame fits in LDS is decoded faster by acg_ldpc_decoder_create_quantized: use this call for the codes that one
 * refuses.
 * Not provided: a cascade stage of this engine (acg_ldpc_cascade_create builds its own stages with the two create calls
 * above), a grid form for acg_ldpc_mc_run_quants.  (Float messages: acg_ldpc_decoder_create_layered_streamed below.) */
int acg_ldpc_decoder_create_quantized_streamed(const acg_ldpc_code *code, const acg_ldpc_params *params, const acg_ldpc_quant *q,
                                               acg_ldpc_decoder **out);

/* ---- streamed float layered BP: sum-product and min-sum at any code size and check degree (build-added) ---- */

/* Layered sum-product (the reference's check rule, bp.h:49-57) and normalised min-sum with fp32 posteriors and fp32 messages, a
 * frame's state in device memory instead of LDS (bp_streamed_layered_kernel): one lane is one frame, a wavefront owns a tile of
 * T frames and walks the edges of a check in a loop, so neither the size of a frame nor the degree of a check is bounded.
 * The arithmetic, stopping rule, latching, final syndrome pass and iteration count are those of acg_ldpc_decoder_create with
 * schedule = ACG_LDPC_SCHEDULE_LAYERED and lanes_per_frame = 256 / 512 / 1024 (the workgroup-per-frame engines) — word, flag
 * and iteration of every frame are equal on every code both accept.  The checks are taken in the order of the sets
 * acg_ldpc_debug_layers_any reports, set by set.  tests/layered_ref.py restates it.  State of a frame: 4 n + 4 E bytes.
 * Required of *params, anything else is refused with a message before a device is looked for:
 *   algo = ACG_LDPC_BP_SUMPRODUCT or ACG_LDPC_BP_MINSUM, schedule = ACG_LDPC_SCHEDULE_LAYERED,
 *   precision = ACG_LDPC_PREC_DEFAULT, engine = ACG_LDPC_ENGINE_AUTO or ACG_LDPC_ENGINE_STREAMED (ACG_LDPC_ENGINE_FUSED is
 *   refused), lanes_per_frame = 0.  ms_scale, max_iter, early_exit and device apply as everywhere.
 * Workspace: one allocation of tiles x (the state of T frames plus, for sum-product on a code with a check of more than 8
 * variables, 4 ceil(Dmax / 8) bytes per frame of scratch; rounded up to 256), T = 64, tiles = min(12 per compute unit,
 * what fits in a quarter of the device's free memory); creation fails with a message when not one tile fits.
 * ACG_STREAML_TILES=<count> (developer switch, read at creation) lowers the tile count.
 * The handle is an ordinary decoder: acg_ldpc_decode_batch, _f32 and _dev take it; acg_ldpc_mc_run and _detail go noise kernel
 * -> decode -> classification kernel; acg_ldpc_mc_run_grid refuses it as it refuses every handle that is not QP-ADMM; the integer
 * entrances (acg_ldpc_decode_batch_q, _q_dev, acg_ldpc_quantize_dev, acg_ldpc_mc_run_quants) refuse it as a handle that is not
 * quantized.  The workspace belongs to the handle, so launches of one handle on different streams are ordered on the device.
 * acg_ldpc_decoder_name returns "BP" or "MS"; acg_ldpc_decoder_layout reports as for the streamed engines (no LDS bytes, one
 * lane per frame, T frames per block, tiles); acg_ldpc_decoder_describe names the kernel, the algorithm, T, the tiles, the bytes
 * of state per frame and the sets, and ends in io=llr,post (the LLR entrance below).
 * A code whose frame fits in LDS is decoded faster by acg_ldpc_decoder_create: use this call for the codes that one refuses
 * (check degree above 32, a frame beyond 160 KiB).
 * Not provided: a cascade stage of this engine (acg_ldpc_cascade_create keeps building its stages with the create calls it uses
 * today), fp16 messages, fp64, a fused Monte-Carlo kernel. */
int acg_ldpc_decoder_create_layered_streamed(const acg_ldpc_code *code, const acg_ldpc_params *params, acg_ldpc_decoder **out);

/* The LLR entrance of the engine: LLRs in, posterior LLRs out.  For punctured and shortened codes, for LLRs from one's own
 * demapper, for channels that symbols + snr cannot express, and for whatever wants soft output behind the decoder.
 *   LLR in          a frame is n float values L_v in natural-log units with the sign convention of the symbol entrance
 *                   (positive = bit 0).  Per value, in this order: NaN becomes +0; the value is clamped to +-1048576 (2^20: far
 *                   beyond any useful LLR, and +-inf never meets the arithmetic); min-sum starts from that, sum-product from
 *                   that times (float) log2(e) in one fp32 multiply — the multiply the symbol entrance applies to the LLR it
 *                   forms.  Every message starts from 0.  So for LLRs of at most 2^20 that the symbol entrance would have formed
 *                   itself (float symbols: (float) ((double) y * (2 / sigma^2))) word, flag and iteration are those of the symbol
 *                   entrance.  There is no snr.
 *                   A punctured position is L = 0; a shortened one +1048576 (known 0) or -1048576 (known 1) — or +-inf, which
 *                   is clamped to that.  Nothing special is done for them: they are LLRs like any other.
 *   posterior out   a frame's posterior is n float values in natural-log units, read at the moment the frame's word, flag and
 *                   iteration are written: min-sum hands out its posterior P_v as it is, sum-product P_v times (float) ln 2 in
 *                   one fp32 multiply.  For a frame that latches, the posteriors of the round boundary at which its word is
 *                   formed — with early_exit = 0 the frame is swept on, the posterior written is still the latched one; for a
 *                   frame that fails, the posteriors after max_iter iterations (its word is zeros as everywhere); for
 *                   max_iter = 0 the clamped input (sum-product: scaled and scaled back, two roundings, so not always the
 *                   input's bits).  The sign bit is the hard decision, -0 included: signbit(post) is the word of every frame
 *                   with ok = 1.
 * Both take a handle of acg_ldpc_decoder_create_layered_streamed only.  Each returns non-zero, leaves a message in
 * acg_ldpc_last_error and launches nothing for a null handle, frames < 0, frames > 0 with a null input (the host call: also null
 * bits or ok) — all three before a device is looked for — and for any other handle (the message names the create call).
 * frames == 0 is a no-op that returns 0.  iters* and post* may be NULL. */

/* acg_ldpc_decode_batch_dev with LLRs in and, if post_dev != NULL, frames*n float posteriors out: the same launch path, so the
 * work-counter ring, the event pair and the stream rules at the top of this header hold for it */
int acg_ldpc_decode_batch_llr_dev(acg_ldpc_decoder *dec, const float *llr_dev, int64_t frames, uint32_t *bits_dev, uint8_t *ok_dev,
                                  int32_t *iters_dev, float *post_dev, void *stream);
/* host buffers, through the pipelined two-set staging path of acg_ldpc_decode_batch_f32 (4 bytes in per value; 4 more out per
 * value when post is given) */
int acg_ldpc_decode_batch_llr(acg_ldpc_decoder *dec, const float *llr, int64_t frames, uint8_t *bits, uint8_t *ok, int32_t *iters,
                              float *post);

/* ---- OSD: ordered-statistics decoding (Fossorier-Lin) of order 0 and 1 (build-added) ------ */

/* acg_ldpc_decoder_create with algo = ACG_LDPC_OSD; max_iter is the ORDER, 0 or 1.  One GF(2) elimination per frame, no
 * iterations, no transcendental, every value an integer; it always returns a codeword.  The algorithm:
 *   A frame is n soft values s_v of type int16_t.  Hard decision z_v = (s_v < 0); reliability r_v = min(|s_v|, 32767) (so
 *   -32768 counts as 32767).
 *   Order        key_v = (r_v << 16) | v, ascending: least reliable first, ties broken by the lower v (hence n <= 65535).
 *   Pivot set B  scan the variables in ascending key; v joins B iff column v of H is linearly independent over GF(2) of the
 *                columns already in B.  |B| = rank(H).  The information set I is the complement of B: the n - rank most reliable
 *                independent positions (the dual statement of the most-reliable-basis construction on a generator matrix).
 *   Candidates   for T a subset of I, x_T is the unique codeword with x_v = z_v ^ [v in T] on I.
 *   Metric       M(x) = sum_v r_v [x_v != z_v], an integer <= n * 32767.
 *   Order 0      x_{}.   Order 1: the minimiser of M over x_{} and x_{j}, j in I; on a tie x_{} wins, then the lowest j.
 *   Outputs      the word; ok = 1 for every frame; iters = |T| of the winner, 0 or 1.
 * Symbol entrance (acg_ldpc_decode_batch, _f32, _dev, acg_ldpc_mc_run, _detail): y32 = the symbol as float (a double is rounded
 * to nearest), s = clamp(truncf(y32 * 4096.0f), -32767, 32767), NaN -> 0, +-inf -> +-32767; snr is accepted and ignored.  So
 * the symbol entrance equals acg_ldpc_debug_osd_soft followed by the integer entrance.  OSD on channel symbols alone is weak on
 * the short codes here (H05: FER 0.63 at -2 dB); it is meant as the second stage of a cascade, on posteriors (below).
 * Refused by acg_ldpc_decoder_create with a message naming the rule: max_iter other than 0 or 1; precision other than DEFAULT;
 * engine other than AUTO or FUSED; schedule other than FLOODING; lanes_per_frame other than 0, 64, 128 or 256 (workgroup threads;
 * 0 = the smallest that covers the n columns in at most two passes, else 256); n > 65535; a frame whose working matrix
 * (n columns of ceil(m / 32) words), keys, permutation, pivot bookkeeping and word do not fit in the 160 KiB of LDS of a CU.
 * alpha, mu, eps_stop, ms_scale and early_exit are ignored.  acg_ldpc_mc_run_grid and _quants refuse the handle. */

/* the integer entrance: frames * n int16 soft values in (device; the same launch path as acg_ldpc_decode_batch_dev: work-counter
 * ring, event pair, stream rules).  Null, negative and zero-frame rules are those of acg_ldpc_decode_batch_q*; both refuse a
 * handle that is not OSD. */
int acg_ldpc_osd_decode_batch_dev(acg_ldpc_decoder *dec, const int16_t *s_dev, int64_t frames, uint32_t *bits_dev, uint8_t *ok_dev,
                                  int32_t *iters_dev, void *stream);
/* host buffers, through the pipelined two-set staging path of acg_ldpc_decode_batch (2 bytes in per value) */
int acg_ldpc_osd_decode_batch(acg_ldpc_decoder *dec, const int16_t *s, int64_t frames, uint8_t *bits, uint8_t *ok, int32_t *iters);
/* the symbol entrance's quantiser on the device (test helper, the counterpart of acg_ldpc_debug_quantize): count symbols of
 * float / double on the host -> count int16 */
int acg_ldpc_debug_osd_soft(const void *y_host, int32_t y_is_f64, int64_t count, int16_t *out_host);

/* replaces Decoder::decode(H, y, snr) (algo/algo.h:8) for `frames` frames at once.
 *   y      host, frames*n doubles, raw channel symbols (NOT LLRs; llr = 2y/sigma^2 is formed inside,
 *          channel.h:12-16, bp.h:66, qp_admm.h:27)
 *   bits   host, frames*n bytes (0/1).  BP failure -> zeros (the reference returns an empty vector, bp.h:198)
 *   ok     host, frames bytes: the reference's bool (BP: zero syndrome reached; QP-ADMM: always 1 unless the
 *          e_min*mu<=alpha guard fires, qp_admm.h:112-114,177)
 *   iters  host, frames int32 or NULL: sweeps executed until exit (BP: iteration of the first zero syndrome)
 * Large batches are pipelined in chunks of at most 65536 frames / 256 MiB of symbols through two pinned staging sets
 * (a process-wide pool of host threads, created on the first batch of >= 4096 frames, copies / unpacks while the GPU
 * decodes the previous chunk); the rate is PCIe-bound: 8 bytes in + 1 byte out per symbol. */
int acg_ldpc_decode_batch(acg_ldpc_decoder *dec, const double *y, int64_t frames, double snr, uint8_t *bits,
                          uint8_t *ok, int32_t *iters);

/* Same with single-precision symbols (half the PCIe bytes).  The LLR is formed as (double) y * (2 / sigma^2), rounded
 * to the kernel's message type — the path of acg_ldpc_decode_batch_dev with y_is_f64 = 0.  A caller holding doubles
 * who wants the reference's exact llr = 2y / sigma^2 (channel.h:14-16) uses acg_ldpc_decode_batch. */
int acg_ldpc_decode_batch_f32(acg_ldpc_decoder *dec, const float *y, int64_t frames, double snr, uint8_t *bits,
                              uint8_t *ok, int32_t *iters);

/* Same, buffers already resident in HBM (this is what bench.py times).
 *   y_dev        device, frames*n of float (y_is_f64=0) or double (y_is_f64=1)
 *   bits_dev     device, frames*words uint32, words = (n+31)/32; bit v of a frame = word v>>5, bit v&31
 *   ok_dev       device, frames bytes;  iters_dev device, frames int32 (may be NULL)
 *   stream       hipStream_t to launch on (NULL = the decoder's own stream); asynchronous.  The output buffers of
 *                two launches in flight must not overlap; see "Streams" at the top of this file. */
int acg_ldpc_decode_batch_dev(acg_ldpc_decoder *dec, const void *y_dev, int32_t y_is_f64, int64_t frames,
                              double snr, uint32_t *bits_dev, uint8_t *ok_dev, int32_t *iters_dev, void *stream);
/* block until the decoder's own stream is idle */
int acg_ldpc_decoder_sync(acg_ldpc_decoder *dec);
/* duration in ms of the most recent decode/mc kernel launch on this handle, measured with the HIP event pair that
 * launch recorded on its own stream (every launch owns a pair: launches of one handle overlapping on two streams never
 * pair each other's events); synchronises on the stop event */
float acg_ldpc_decoder_last_kernel_ms(acg_ldpc_decoder *dec);
/* bytes of LDS per frame, frames resident per CU, lanes per frame chosen for this code (diagnostics).  Streamed engines:
 * 0 bytes of LDS per frame, 1 lane per frame, 64 frames per block; QP-ADMM's grid_blocks = the number of slabs */
void acg_ldpc_decoder_layout(const acg_ldpc_decoder *dec, int32_t *lds_bytes_per_frame, int32_t *lanes_per_frame,
                             int32_t *frames_per_block, int32_t *grid_blocks);

/* one line naming the engine / kernel instance / launch shape this handle uses (diagnostics; bench.py records it with every
 * timed leg).  Writes at most cap bytes incl. the terminating 0; returns the size the full text needs. */
int32_t acg_ldpc_decoder_describe(const acg_ldpc_decoder *dec, char *buf, int32_t cap);

/* ---- two-stage decoding: a second decoder for the frames the first fails (build-added) ------ */

/* A cascade owns TWO decoders for one code on one device: a cheap one that sees every frame and a strong one that sees only
 * the frames the cheap one gives up on.  Semantics, per frame.  Let (w1, ok1, it1) be what stage 0 returns for the frame.
 *   ok1 = 1   the cascade returns (w1, 1, it1) and stage = 1;
 *   ok1 = 0   it returns (w2, ok2, it2) and stage = 2: what stage 1 returns for the same symbols at the same snr.
 * iters is the count of the stage that produced the result (a second-stage frame spent max_iter of the first on top of it);
 * the flag is that stage's flag (QP-ADMM reports 1 for every frame it touches).  A frame's result depends on the frame only,
 * not on the batch it is in, so the cascade equals the two handles run by hand: stage 0 on everything, stage 1 on the compacted
 * failed rows, the results put back.  Any two decoders are accepted, quantized handles included (symbol entrance).  A first
 * stage that never fails (QP-ADMM without its guard) leaves the second idle; max_iter = 0 or a guard decoder as first stage
 * sends every frame on.  Neither is an error.
 * Device path, per chunk of at most 65536 frames / 256 MiB of symbols (the bound of acg_ldpc_decode_batch's staging) on the
 * caller's stream: stage 0 into the caller's outputs -> cascade_select_kernel (the ascending list of the frames with ok = 0 and
 * their number K) -> K comes to the host in one small copy followed by a wait on the stream: THE ONE HOST WAIT PER CHUNK -> if
 * K > 0: cascade_gather_kernel (their symbol rows into a compact batch), stage 1 over K frames through the ordinary launch path
 * (work-counter ring, event pair and stream rules at the top of this header), cascade_scatter_kernel (words, flag, iterations,
 * stage = 2 back to their rows).  The tail of the last chunk is asynchronous, as acg_ldpc_decode_batch_dev is: outputs are
 * complete once the stream is idle.  The hand-over buffers belong to the cascade, so two calls on different streams are ordered
 * on the device, not concurrent.  A call holds the cascade's mutex, then stage 0's, then stage 1's.
 * Posterior hand-over.  When stage 0 is a handle of acg_ldpc_decoder_create_quantized and stage 1 is OSD, a failed frame's
 * POSTERIORS go on, not its symbols: stage 0's result is unchanged, and for ok1 = 0 the cascade returns what
 * acg_ldpc_osd_decode_batch_dev returns for the int16 posteriors that stage 0's integer entrance writes for the frame (those
 * after max_iter iterations).  Per chunk: acg_ldpc_quantize_dev -> stage 0's integer entrance with post_dev (equal to its symbol
 * entrance by the rule above) -> select -> cascade_gather_kernel on the posterior rows -> OSD's integer entrance over K frames ->
 * scatter; still one host wait.  The host entries and acg_ldpc_cascade_mc_run take the same route (a host chunk is copied to the
 * device) and return the same results.  Every other pairing with OSD as a stage hands over symbols as above; OSD on channel
 * reliabilities is weak, see "OSD". */
typedef struct acg_ldpc_cascade acg_ldpc_cascade;
/* q_first / q_second: NULL = that stage comes from acg_ldpc_decoder_create, else from acg_ldpc_decoder_create_quantized with that
 * quantiser.  Refused (non-zero, message in acg_ldpc_last_error): null code, params or out; params that resolve to different
 * devices (-1 = the current device); whatever the two create calls refuse, with their message prefixed "first: " / "second: ". */
int acg_ldpc_cascade_create(const acg_ldpc_code *code, const acg_ldpc_params *first, const acg_ldpc_quant *q_first,
                            const acg_ldpc_params *second, const acg_ldpc_quant *q_second, acg_ldpc_cascade **out);
void acg_ldpc_cascade_destroy(acg_ldpc_cascade *c);
/* the two decoders, borrowed (stage 0 / 1; anything else: NULL): ordinary handles for describe, layout, or a decode of their
 * own; never destroy them */
acg_ldpc_decoder *acg_ldpc_cascade_stage(acg_ldpc_cascade *c, int32_t stage);
/* "<first>+<second>" of acg_ldpc_decoder_name, e.g. "MS+BP", "BP+QP-ADMM" */
const char *acg_ldpc_cascade_name(const acg_ldpc_cascade *c);
/* "cascade <name> | first: <describe line> | second: <describe line> | chunk=<frames per chunk> last_second_frames=<K>
 * handover=posteriors|symbols", chunk and K of the most recent call; buf / cap / return value as acg_ldpc_decoder_describe */
int32_t acg_ldpc_cascade_describe(const acg_ldpc_cascade *c, char *buf, int32_t cap);

/* buffers as acg_ldpc_decode_batch_dev; stage_dev: device, frames bytes, written 1 or 2 for every frame (may be NULL, and so may
 * iters_dev); stream: NULL = stage 0's own stream.  frames == 0 is a no-op that returns 0.  Refused with a message, nothing
 * launched: a null cascade, frames < 0, a null y_dev with frames > 0, null bits_dev or ok_dev.  A K outside 0 ... chunk read back
 * from the device fails the call without a further launch. */
int acg_ldpc_cascade_decode_batch_dev(acg_ldpc_cascade *c, const void *y_dev, int32_t y_is_f64, int64_t frames, double snr,
                                      uint32_t *bits_dev, uint8_t *ok_dev, int32_t *iters_dev, uint8_t *stage_dev, void *stream);
/* host buffers as acg_ldpc_decode_batch (iters and stage may be NULL): a composition of the host paths of the two handles —
 * stage 0's pipelined decode over all frames, a host gather of the failed rows, stage 1's decode over them, a host scatter;
 * nothing new runs on the device.  Same results and refusals as the device entry. */
int acg_ldpc_cascade_decode_batch(acg_ldpc_cascade *c, const double *y, int64_t frames, double snr, uint8_t *bits, uint8_t *ok,
                                  int32_t *iters, uint8_t *stage);
int acg_ldpc_cascade_decode_batch_f32(acg_ldpc_cascade *c, const float *y, int64_t frames, double snr, uint8_t *bits, uint8_t *ok,
                                      int32_t *iters, uint8_t *stage);
/* of the most recent decode or Monte-Carlo call on this cascade: frames handed to the second stage, device ms of the first /
 * second decoder's launches summed over the chunks (host entries: of the last launch of each).  Waits for the second stage's
 * last launch, which the device entry leaves running; call it before the stage handles are launched on again.  Any pointer may
 * be NULL. */
int acg_ldpc_cascade_last_call(acg_ldpc_cascade *c, int64_t *second_frames, float *first_ms, float *second_ms);

/* ---- Monte-Carlo loop (experiment.h) --------------------------------------------------- */

typedef struct acg_ldpc_mc_cfg {
    int64_t frames;       /* frames to simulate in THIS call */
    int64_t first_frame;  /* global index of the first frame (shard offset; seeds derive from the global index) */
    double snr;           /* Es/N0 dB, sigma^2 = 10^(-snr/10)/2 (channel.h:12) */
    uint64_t seed;        /* Philox key (device noise).  Host mt19937 mode ignores it: frame i uses mt19937(i+1) */
    int32_t noise;        /* ACG_LDPC_NOISE_* */
    const uint8_t *codewords; /* host, n_codewords*n bytes, frame g transmits codewords[g % n_codewords];
                                 NULL = all-zero codeword */
    int64_t n_codewords;
} acg_ldpc_mc_cfg;

/* mirrors ExperimentResult + HammingDistanceTracker (experiment.h:25-68) */
typedef struct acg_ldpc_mc_result {
    int64_t correct, pseudo, total;
    int64_t sum_hamming, sum_hamming_ok, sum_hamming_wrong;
    int64_t sum_iters;   /* sweeps executed, for the mean-iterations figure */
    double time_sec;     /* wall time of the call */
    double kernel_ms;    /* device time of the decode kernel(s) */
} acg_ldpc_mc_result;

/* replaces multithread_experiment (experiment.h:125-139): transmit + decode + classify
 * (correct / pseudo-codeword / fail) + raw-channel Hamming statistics, all on the device. */
int acg_ldpc_mc_run(acg_ldpc_decoder *dec, const acg_ldpc_mc_cfg *cfg, acg_ldpc_mc_result *res);
/* merge_exp_results (experiment.h:70-78): a += b (used to combine per-GPU shards on the host) */
void acg_ldpc_mc_merge(acg_ldpc_mc_result *a, const acg_ldpc_mc_result *b);

/* acg_ldpc_mc_run through a cascade (two-stage decoding, above): both noise modes, codewords and first_frame as there, the
 * counters the same for any chunking and sharding.  Every frame goes noise (AWGN kernel, or the host generator and a copy) ->
 * the cascade's device path, chunk by chunk, with the classification kernel run on stage 0's outputs before the scatter (first)
 * and on the merged outputs (total).  A first decoder with a fused Monte-Carlo kernel does not use it here: the second stage
 * needs the symbols. */
typedef struct acg_ldpc_cascade_result {
    acg_ldpc_mc_result total;   /* the returned outputs classified as acg_ldpc_mc_run classifies; kernel_ms = both stages */
    acg_ldpc_mc_result first;   /* seven counters = acg_ldpc_mc_run(stage 0, cfg); kernel_ms of its launches */
    int64_t second_frames;      /* frames handed to stage 1 (ok = 0 after stage 0).  = first.total - first.correct - first.pseudo
                                   whenever stage 0's flag is the zero syndrome: every BP engine, and a QP-ADMM guard decoder */
    int64_t second_correct, second_pseudo, second_sum_iters;  /* of those frames: total.correct = first.correct + second_correct,
                                                                 total.pseudo = first.pseudo + second_pseudo */
    double  second_kernel_ms;
} acg_ldpc_cascade_result;
/* Errors (non-zero, message, nothing launched): null c, cfg or res; a bad cfg as for acg_ldpc_mc_run. */
int acg_ldpc_cascade_mc_run(acg_ldpc_cascade *c, const acg_ldpc_mc_cfg *cfg, acg_ldpc_cascade_result *res);
/* shards: everything adds */
void acg_ldpc_cascade_merge(acg_ldpc_cascade_result *a, const acg_ldpc_cascade_result *b);

/* ---- Monte-Carlo detail run: bit errors and a log of the frames that are not correct ------- */

/* The classification of exp() (experiment.h:109-120) sorts a frame into correct / pseudo-codeword / everything else and keeps
 * counters only.  The detail run extends it (build-added; the reference has no post-decoding bit error count):
 * the frames that are not correct are split by what the decoder returned, their bit errors are counted, and the first `cap`
 * of them are written out as events a caller can replay (device noise is keyed on the global frame index alone).
 *
 * A frame whose decoder returned NO word (flag false: BP ran out of iterations, bp.h:198; the QP-ADMM guard fired,
 * qp_admm.h:112-114) contributes NOTHING to bit_errors — the reference returns an empty vector there and no word is invented
 * for it.  bit_errors / (total * n) is therefore the bit error rate over RETURNED words: the undetected bit errors for BP
 * (its returned words are codewords: correct or pseudo), all bit errors for QP-ADMM (which returns a word for every frame
 * unless the guard fires).  word_frames is the denominator for a rate per returned word: bit_errors / (word_frames * n). */
typedef struct acg_ldpc_mc_detail {
    acg_ldpc_mc_result base;      /* field for field what acg_ldpc_mc_run returns for the same cfg (the two times aside) */
    int64_t word_frames;          /* frames whose decoder returned a word (flag set): BP correct + pseudo; QP-ADMM all but guard */
    int64_t bit_errors;           /* sum over word_frames of d_H(word, sent), bits >= n masked off */
    int64_t noncodeword_frames;   /* flag set but H*word != 0 (QP-ADMM; 0 for BP, whose flag IS the zero syndrome) */
    int64_t sum_syndrome_weight;  /* unsatisfied checks summed over noncodeword_frames */
    int64_t n_events;             /* frames that are not correct = total - correct */
    int64_t n_stored;             /* events written to the caller's buffers = min(n_events, cap) */
    int64_t min_pseudo_frame;     /* lowest global frame attaining min_pseudo_weight, -1 if none */
    int32_t min_pseudo_weight;    /* min d_H(word, sent) over pseudo frames, -1 if none.  word ^ sent is a non-zero codeword
                                     there: an upper bound on the minimum distance of the code */
    int32_t reserved;
} acg_ldpc_mc_detail;

/* kind of an event: the "else" branch of experiment.h:110-119 and its pseudo branch, told apart */
enum {
    ACG_LDPC_EVENT_PSEUDO = 1,     /* flag set, zero syndrome, word != sent (experiment.h:115-116) */
    ACG_LDPC_EVENT_NO_WORD = 2,    /* flag false: no word was returned */
    ACG_LDPC_EVENT_NONCODEWORD = 3 /* flag set, H*word != 0 (QP-ADMM always reports true, qp_admm.h:177) */
};

typedef struct acg_ldpc_mc_event { /* 32 bytes */
    int64_t frame;            /* GLOBAL frame index */
    int32_t kind;             /* ACG_LDPC_EVENT_* */
    int32_t iters;            /* sweeps executed, as acg_ldpc_decode_batch reports them */
    int32_t raw_errors;       /* raw-channel hard-decision errors of the frame (the reference's Hamming figure, experiment.h:25-47) */
    int32_t bit_errors;       /* d_H(word, sent); 0 for NO_WORD */
    int32_t syndrome_weight;  /* unsatisfied checks; 0 unless NONCODEWORD */
    int32_t reserved;
} acg_ldpc_mc_event;

/* acg_ldpc_mc_run plus the above, for every decoder the library creates and both noise modes.
 *   events  host, cap entries (may be NULL when cap == 0)
 *   words   host, cap * ((n+31)/32) uint32, or NULL: row k = (returned word) XOR (sent word) of event k, packed as
 *           acg_ldpc_decode_batch_dev packs bits; all-zero for a NO_WORD event; bits >= n are zero
 * Deterministic: the stored events are those of the `cap` LOWEST global frame indices among the frames that are not correct,
 * in ascending frame order, whatever the chunking, the launch shape or the order in which wavefronts finish; n_events counts
 * all of them.  Every frame goes noise kernel -> plain decode -> classification kernel (device noise; decoders with a fused
 * Monte-Carlo kernel do not use it here, so the call is slower than acg_ldpc_mc_run for them), or host noise -> decode ->
 * host classification (ACG_LDPC_NOISE_HOST_MT19937).  A QP-ADMM guard decoder is not refused: every frame is a NO_WORD event.
 * Errors (non-zero, message in acg_ldpc_last_error, nothing launched): null dec, cfg or out; cap < 0; cap > 0 with null
 * events; a bad cfg as for acg_ldpc_mc_run. */
int acg_ldpc_mc_run_detail(acg_ldpc_decoder *dec, const acg_ldpc_mc_cfg *cfg, acg_ldpc_mc_detail *out,
                           acg_ldpc_mc_event *events, uint32_t *words, int64_t cap);
/* a += b for shards, as acg_ldpc_mc_merge does for base: counters add; min_pseudo_weight is the smaller one (-1 = none is
 * ignored, and so is the 0 of an accumulator the caller zeroed), on a tie the lower frame.  n_stored is left as it is: the caller owns the shards' event buffers (concatenate,
 * sort by frame, cut to cap). */
void acg_ldpc_mc_detail_merge(acg_ldpc_mc_detail *a, const acg_ldpc_mc_detail *b);

/* replaces the double loop of qpadmm_params.cpp:64-77: acg_ldpc_mc_run for n_points parameter pairs (alpha[k], mu[k]) of
 * a QP-ADMM decoder on ONE handle.  dec's own alpha and mu are ignored in this call; its max_iter, eps_stop, early_exit,
 * precision, engine and device apply.  Every point simulates the same global frames [first_frame, first_frame + frames)
 * with the same codewords and the same noise, generated once.  res[k] (n_points entries) holds, field for field, what
 * acg_ldpc_mc_run returns on a decoder created with (alpha[k], mu[k]) and the same remaining parameters, except:
 *   time_sec   of EVERY entry is the wall time of the whole call (not a per-point time: do not add them up);
 *   kernel_ms  of an entry is the point's share of device time: the device time of the launch (chunk of points) it ran
 *              in divided by the number of points in that chunk.
 * Guard points, e_min*mu <= alpha (qp_admm.h:108-114), are not an error here (acg_ldpc_mc_run refuses them): no sweep
 * runs and they return what the reference's loop computes — correct = pseudo = 0, total = frames, sum_iters = 0 and the
 * raw-channel Hamming sums, all of them in sum_hamming_wrong (experiment.h:109-120).
 * Sharding by first_frame / frames and acg_ldpc_mc_merge per point work as for acg_ldpc_mc_run.
 * Single launch: decoders on the workgroup-per-frame kernel (lanes_per_frame 0 or 256 on a code it accepts, max_iter > 0;
 * acg_ldpc_decoder_describe says mc_grid=single-launch) decode a chunk of points x frames per launch; the chunk is sized
 * so that its per-frame outputs are those of a 65536-frame decode.  Every other QP-ADMM decoder (lanes_per_frame
 * 16/32/64, the streamed engine, max_iter = 0; mc_grid=per-point) runs the points one after another on this handle,
 * re-parameterised in place — same results, no handle created or destroyed.
 * Errors (non-zero, message in acg_ldpc_last_error, nothing launched): a decoder that is not QP-ADMM, n_points < 1,
 * null pointers. */
int acg_ldpc_mc_run_grid(acg_ldpc_decoder *dec, const acg_ldpc_mc_cfg *cfg, const double *alpha, const double *mu,
                         int32_t n_points, acg_ldpc_mc_result *res);

/* The format search of the fixed-point layered min-sum engine: acg_ldpc_mc_run for n_points quantisers quants[k] on ONE handle
 * of acg_ldpc_decoder_create_quantized.  dec's own quantiser is ignored in this call; its max_iter, early_exit,
 * lanes_per_frame and device apply.  Every point simulates the same global frames [first_frame, first_frame + frames) with
 * the same codewords and the same noise (both noise modes), generated once per block of frames.  res[k] (n_points entries)
 * holds, in its seven integer counters, what acg_ldpc_mc_run returns for *cfg on a handle created with quants[k] and the same
 * acg_ldpc_params;
 *   time_sec   of EVERY entry is the wall time of the whole call (not a per-point time: do not add them up);
 *   kernel_ms  of an entry is the point's share of device time: the device time of the launch (chunk of points) it ran
 *              in divided by the number of points in that chunk.
 * Duplicate points are allowed and return equal counters.  Sharding by first_frame / frames and acg_ldpc_mc_merge per point
 * work as for acg_ldpc_mc_run.  frames == 0 is a no-op that zeroes res and returns 0; max_iter = 0 takes the same path (every
 * frame fails with 0 iterations).
 * Single launch (acg_ldpc_decoder_describe of every quantized handle says mc_quants=single-launch): a launch of the kernel's
 * grid form decodes a chunk of points x frames, the quantiser of a frame read from a device table of 32 bytes per point;
 * the chunk is sized so that its per-frame outputs are those of a 65536-frame decode.  No handle is created or destroyed and
 * nothing is allocated per point.
 * Errors (non-zero, message in acg_ldpc_last_error, nothing launched, res untouched), in this order: null dec, cfg, quants
 * or res; n_points < 1 (both before the handle is looked at); a handle that is not of acg_ldpc_decoder_create_quantized; a
 * bad cfg as for acg_ldpc_mc_run; ANY quants[k] that acg_ldpc_quant_check rejects — the message names k and the rule.  There
 * is no guard point: an invalid format is a caller error. */
int acg_ldpc_mc_run_quants(acg_ldpc_decoder *dec, const acg_ldpc_mc_cfg *cfg, const acg_ldpc_quant *quants, int32_t n_points,
                           acg_ldpc_mc_result *res);

/* replaces the scoring of optimize_H.cpp:16-25 for a BATCH of parity-check matrices: acg_ldpc_mc_run for n_codes codes of one
 * m x n under one set of QP-ADMM parameters.  An evaluator owns one stream, one work-counter ring, one set of staging and
 * output buffers, one table buffer and one counter buffer; it creates no decoder handle and allocates nothing per code.
 * res[k] equals, in its seven integer counters, what acg_ldpc_mc_run returns on a decoder created from codes[k] with *params
 * and fast_setup = 1, given cfgs[k]; time_sec of every entry is the wall time of the call, kernel_ms the device time of the
 * code's launch divided by the codes in that launch.  cfgs[k].codewords / n_codewords are per code; frames, first_frame, snr,
 * seed and noise must be equal in every cfgs[k].  A guard code (e_min*mu <= alpha for that code's e_min) is not an error: it
 * gets what the reference's loop computes from DecodeQPADMM's (zeros, false) (qp_admm.h:112-114), as a guard point of
 * acg_ldpc_mc_run_grid does.  Sharding by first_frame / frames and acg_ldpc_mc_merge per code work as for acg_ldpc_mc_run.
 * Single launch: with parameters that select the workgroup-per-frame kernel (lanes_per_frame 0 or 256, not the streamed
 * engine, max_iter > 0) the codes that kernel accepts are grouped by launch shape (threads per workgroup, passes, lean or
 * general instance) and every group decodes in one launch per chunk of codes x frames (chunked like the parameter grid);
 * acg_ldpc_evaluator_describe then says mc_codes=single-launch groups=<g> chunks=<c>.  Every other code runs through a decoder
 * handle of its own on the evaluator's stream, with the same results (mc_codes=per-code when no code took a shared launch).
 * Errors (non-zero, message in acg_ldpc_last_error, nothing launched): parameters that are not QP-ADMM, n_codes < 1, null
 * pointers, codes of different m or n, cfgs that disagree, no device. */
typedef struct acg_ldpc_evaluator acg_ldpc_evaluator;
int acg_ldpc_evaluator_create(const acg_ldpc_params *params, acg_ldpc_evaluator **out);
void acg_ldpc_evaluator_destroy(acg_ldpc_evaluator *ev);
int acg_ldpc_mc_run_codes(acg_ldpc_evaluator *ev, const acg_ldpc_code *const *codes, int32_t n_codes,
                          const acg_ldpc_mc_cfg *cfgs, acg_ldpc_mc_result *res);
/* one line on what the last acg_ldpc_mc_run_codes of this evaluator did; buf / cap / return value as acg_ldpc_decoder_describe */
int32_t acg_ldpc_evaluator_describe(const acg_ldpc_evaluator *ev, char *buf, int32_t cap);

/* ---- host-side generators used by the reference's drivers (bit-exact, libstdc++) ----------- */

/* replaces gen_random_codewords (utils/channel.h:28-44) with std::mt19937(seed): row i of G (k x n bytes)
 * is XORed in when rnd() % 2 == 0.  out: count*n bytes. */
int acg_ldpc_gen_codewords(const uint8_t *G, int32_t k, int32_t n, uint32_t seed, int64_t count, uint8_t *out);
/* replaces transmit (utils/channel.h:18-26) as driven by exp() (experiment.h:97-99): global frame g uses
 * std::mt19937(g+1) and std::normal_distribution<double>(0, sigma); transmits codewords[g % n_codewords]
 * (NULL = all-zero word).  y: frames*n doubles. */
int acg_ldpc_transmit_host(const uint8_t *codewords, int64_t n_codewords, int32_t n, int64_t first_frame,
                           int64_t frames, double snr, double *y);
/* llr_variance (utils/channel.h:12) */
double acg_ldpc_llr_variance(double snr);

/* device-side AWGN only (utils/channel.h:18-26 with the Philox generator): fills y_dev (frames*n floats)
 * for global frames [first_frame, first_frame+frames). codewords as in acg_ldpc_mc_cfg (host pointer). */
int acg_ldpc_awgn_dev(acg_ldpc_decoder *dec, const acg_ldpc_mc_cfg *cfg, float *y_dev, void *stream);

/* ---- Monte-Carlo runs for punctured and shortened (rate-matched) codes --------------------- */

/* A pattern is n bytes, one per variable (host pointer; NULL = every position sent).  Any other value is refused, and the
 * message names the first offending index. */
enum {
    ACG_LDPC_RM_SENT = 0,      /* transmitted */
    ACG_LDPC_RM_PUNCTURED = 1, /* not transmitted, unknown to the receiver */
    ACG_LDPC_RM_SHORTENED = 2  /* not transmitted, known to the receiver */
};

/* acg_ldpc_mc_run for a rate-matched code, on the handles that have a channel-value entrance: those of
 * acg_ldpc_decoder_create_layered_streamed (fp32 LLRs), acg_ldpc_decoder_create_quantized and
 * acg_ldpc_decoder_create_quantized_streamed (int16 channel values).  Device noise only.
 * Per global frame g and variable v, with bit the bit of codewords[g % n_codewords] (0 for NULL codewords):
 *   symbol   y = fma(sigma32, z, bit ? -1 : +1), z the Philox / Box-Muller sample of (seed, g, quad v >> 2, element v & 3) and
 *            sigma32 as in acg_ldpc_awgn_dev: bit for bit the float that call writes for the position.  A position that is
 *            not sent consumes its sample and discards it, so the noise of the sent positions does not depend on the pattern.
 *   float handle      sent: (float) ((double) y * (2 / sigma^2)), the symbol entrance's own formula for float symbols;
 *                     punctured: +0.0f; shortened: +1048576.0f for bit 0, -1048576.0f for bit 1 (the LLR entrance's clamp).
 *   quantized handle  sent: clamp(rne(llr32 * (float) (1 / llr_step)), +-Cmax) with llr32 as above, NaN -> 0: what
 *                     acg_ldpc_quantize_dev gives for y; punctured: 0; shortened: +Cmax for bit 0, -Cmax for bit 1.
 *   raw errors        of a frame: the SENT positions with (bit == 0 && y <= 0) or (bit == 1 && y > 0).
 *   decode            the handle's channel-value entrance on its ordinary launch path.
 *   classification    correct <=> ok and the word equals the sent word on all n positions (punctured bits must be recovered,
 *                     shortened ones kept); pseudo <=> ok and they differ.  The seven counters of acg_ldpc_mc_result are
 *                     formed as by acg_ldpc_mc_run, with the raw-error count in place of the Hamming figure.
 * snr is Es/N0 of a TRANSMITTED symbol and is not rescaled by the pattern: the energy per information bit of the
 * rate-matched code is the caller's arithmetic.
 * Refused, in this order, with nothing launched: a null dec, cfg or res; a bad cfg (as acg_ldpc_mc_run);
 * cfg->noise == ACG_LDPC_NOISE_HOST_MT19937; a pattern byte above 2; a handle of any other create call.  frames == 0 zeroes
 * res and returns 0.  The frames go in the chunks of acg_ldpc_mc_run's route for engines without a generator of their own;
 * the counters are the same for any chunking and any sharding by first_frame, and acg_ldpc_mc_merge combines shards.
 * Not provided: host (mt19937) noise; a detail run; cascade and OSD stages; the grid, quants and codes forms; engines without
 * a channel-value entrance (every handle of acg_ldpc_decoder_create); repetition or bit selection beyond the three states. */
int acg_ldpc_mc_run_rm(acg_ldpc_decoder *dec, const acg_ldpc_mc_cfg *cfg, const uint8_t *pattern, acg_ldpc_mc_result *res);
/* device-side channel values only, the counterpart of acg_ldpc_awgn_dev: frames*n floats (float handle) or int16 (quantized
 * handles) into out_dev, and, if raw_dev != NULL, frames int32 raw-error counts.  The same rules and refusals (out_dev in the
 * place of res). */
int acg_ldpc_rm_channel_dev(acg_ldpc_decoder *dec, const acg_ldpc_mc_cfg *cfg, const uint8_t *pattern, void *out_dev,
                            int32_t *raw_dev, void *stream);

/* diagnostics (used by tests/): evaluates the device phi(x) = -log(tanh(x/2)) (bp.h:34) of the BP kernels
 * on n host values; f64 selects the double variant. */
int acg_ldpc_debug_phi(const void *x_host, void *out_host, int32_t n, int32_t f64);
/* diagnostics: the phi fast path of the fp32 sum-product sweeps on n float inputs in the kernels' log2(e)-scaled domain;
 * out: 3n uint32 = per input the bits of the full phi, of the check-side path and of the variable-side path (on |x|). */
int acg_ldpc_debug_phi_sat(const void *x_host, void *out_host, int32_t n);
/* diagnostics: the one-series phi of the fixed-work fused sum-product sweeps (phi_large where every evaluating lane of a
 * wavefront has x >= 2, phi_small where every one has x <= 1; in instances that a handle takes unless ACG_BP_NO_PHISPLIT=1 is set at its
 * creation; same results) against the full evaluation on every non-negative fp32 bit pattern, in the kernels'
 * log2(e)-scaled domain.  out: 6 uint32 = patterns in
 * [2, 66) / (0, 1] whose series does not give phi's bits; the smallest such pattern (all ones: none); the bits of the largest
 * finite x with ps >= pl; of the smallest x > 0 with pl >= ps; patterns where max(ps, pl) behind the saturation select does not
 * give phi's bits; the smallest such pattern. */
int acg_ldpc_debug_phi_split(uint32_t *out_host);
/* diagnostics: counters of the fixed-work fused sum-product kernels' freeze path (a latched frame whose message state recurs
 * bit for bit stops sweeping; outputs are those of max_iter sweeps; ACG_BP_NO_FREEZE=1 at handle creation runs every sweep).
 * Waits for the handle's launches, returns what they counted since the previous call (frames frozen; sweeps those frames did
 * not execute), then clears the counters.  enable != 0: later launches count (no effect on a handle without the path: both
 * figures stay 0); enable == 0: counting stops.  A launch counts at most 2^24 - 1 frozen frames. */
int acg_ldpc_debug_freeze_stats(acg_ldpc_decoder *d, int32_t enable, int64_t *frames_frozen, int64_t *sweeps_not_run);
/* diagnostics: the detections of the freeze path, counted while acg_ldpc_debug_freeze_stats has counting on.  A detection (one
 * per frame and snapshot cadence point behind the latch) either only writes the frame's state to its snapshot slot (store pass:
 * the first behind a latch, and every one at which a lane's checksum of its words differs from the one it took at the
 * previous snapshot) or loads the snapshot and compares it word for word (compare pass; ACG_BP_FREEZE_NO_GATE=1 at handle
 * creation: every detection behind the first).  Only a compare pass can freeze a frame.  Waits for the handle's launches,
 * returns the two counts since the previous call and clears them. */
int acg_ldpc_debug_freeze_passes(acg_ldpc_decoder *d, int64_t *store_passes, int64_t *compare_passes);
/* diagnostics: soft state of the device sum-product decoder after `iters` full iterations of bp.h:183-199 without
 * the exit test, for 1..64 frames (y: frames*n doubles).  Outputs are frames*E (edge order: check-major, variables
 * ascending) / frames*n doubles: c2v = messages check->variable, (v2c_mag, v2c_sgn) = the (phi(|x|), sign) pairs
 * variable->check, post = VNode::estimate() (bp.h:85-90).
 * engine: ACG_LDPC_ENGINE_STREAMED (or AUTO) = the HBM engine (fp32: a debug instance of the LDS-DMA ring kernel that ships, with
 * its own sweeps and counted waits; fp64 and node degrees above 12: the register-staged kernel); ACG_LDPC_ENGINE_FUSED = the LDS-resident kernels, read out
 * of LDS by a debug instance of the same kernel: lanes_per_frame 0/32/64 = wavefront groups (node degree <= 8, n <= 12
 * passes), 256 = one workgroup per frame (index table in LDS).  For the fused kernels `post` is the channel LLR plus the
 * sum of the dumped c2v words, added on the host. */
int acg_ldpc_debug_bp_trace(const acg_ldpc_code *code, const double *y, int32_t frames, double snr, int32_t iters,
                            int32_t f64, int32_t engine, int32_t lanes_per_frame, double *c2v, double *v2c_mag,
                            double *v2c_sgn, double *post);

/* diagnostics (host only, no device needed): the task tables of the streamed engine's LDS-DMA ring kernel, 4 int32 per task
 * {first node, nodes, first line / col_ptr entry, lines | wait << 8 | wait_without_stores << 16}; consts (4 int32) receives
 * {wavefronts per workgroup, ring slots, lines per slot, edge lines per variable task}.  tests/test_ring_waits.py replays
 * the kernel's issue order against the counted waits. */
int acg_ldpc_debug_ring_tasks(const acg_ldpc_code *code, int32_t *n_ctask, int32_t *n_vtask, int32_t *ctask, int32_t *vtask,
                              int64_t cap, int32_t *consts);

/* diagnostics (host only, no device needed): the layers of ACG_LDPC_SCHEDULE_LAYERED for this matrix.  lanes = lanes per
 * frame G, n_layers, qc_Z = circulant size if the block rows of a quasi-cyclic H were used (0: greedy colouring);
 * chk (may be NULL) receives n_layers * G check ids in processing order (-1 = empty lane), at most cap entries.
 * Returns 0, or non-zero if the matrix cannot be layered (message in acg_ldpc_last_error). */
int acg_ldpc_debug_layers(const acg_ldpc_code *code, int32_t *lanes, int32_t *n_layers, int32_t *qc_Z, int32_t *chk, int64_t cap);

/* diagnostics (host only, no device needed): the sets of ACG_LDPC_SCHEDULE_LAYERED with one workgroup per frame
 * (lanes_per_frame 256, 512, 1024) for this matrix: checks of one degree that share no variable, of any number — the block
 * rows of a quasi-cyclic H (qc_Z = circulant size), else first-fit colouring in row order (qc_Z = 0).  width = checks in the
 * largest set; chk (may be NULL) receives n_layers * width check ids in processing order, occupied slots first, padded with
 * -1, at most cap entries.  Returns 0, or non-zero if the matrix cannot be layered (check degree above 8, no checks; message
 * in acg_ldpc_last_error). */
int acg_ldpc_debug_layers_block(const acg_ldpc_code *code, int32_t *n_layers, int32_t *width, int32_t *qc_Z, int32_t *chk, int64_t cap);

/* diagnostics (host only, no device needed): the same sets by the same rule for the wide-check engine (bp_layered_wide_kernel):
 * the contract of acg_ldpc_debug_layers_block with check degree up to 32 (non-zero for a check degree above 32). */
int acg_ldpc_debug_layers_wide(const acg_ldpc_code *code, int32_t *n_layers, int32_t *width, int32_t *qc_Z, int32_t *chk, int64_t cap);

/* diagnostics (host only, no device needed): the same sets by the same rule without a bound on the check degree — the order in
 * which a handle of acg_ldpc_decoder_create_quantized_streamed takes the checks, set by set.  The contract of
 * acg_ldpc_debug_layers_wide otherwise (non-zero only for a matrix without checks). */
int acg_ldpc_debug_layers_any(const acg_ldpc_code *code, int32_t *n_layers, int32_t *width, int32_t *qc_Z, int32_t *chk, int64_t cap);

/* diagnostics (host code only: a wait and a copy, no kernel): the state a handle of acg_ldpc_decoder_create_layered_streamed or
 * acg_ldpc_decoder_create_quantized_streamed keeps in its workspace for the tile that used slab `slab` last.  Waits for the
 * device, then copies min(cap_bytes, *slab_bytes) bytes of the slab to out_host.  *slab_bytes (required) is always written: the
 * bytes of one slab, 0 where the handle is refused; out_host = NULL is the size query.  Layout of a slab, T = 64:
 *   float engine      P[n][T] fp32 posteriors (sum-product: in the kernels' log2(e)-scaled domain), then R[E][T] fp32 messages,
 *                     then the scratch of wide sum-product checks (unspecified content), rounded up to 256 bytes;
 *   quantised engine  P[n][T] int16 posteriors, then R[E][T] int8 messages, rounded up to 256 bytes.
 * Edges are in processing order: the sets of acg_ldpc_debug_layers_any, set by set, each check's variables ascending.  Lane l
 * of the slab is frame 64 tile + l of the launch.  A workgroup takes tiles as they come, so which tile a slab held last is
 * known only with one slab (ACG_STREAML_TILES=1 / ACG_STREAMQ_TILES=1 at creation: slab 0 holds the last tile of the last
 * launch).  P of a lane beyond the launch's frames is +0; its R, and every R after a launch with max_iter = 0, is unspecified.
 * Refused with a message: a null handle, a handle of any other create call, slab outside 0 ... tiles - 1, a negative cap_bytes. */
int acg_ldpc_debug_streamed_slab(acg_ldpc_decoder *d, int32_t slab, void *out_host, int64_t cap_bytes, int64_t *slab_bytes);

#ifdef __cplusplus
}
#endif
#endif /* ACG_LDPC_H */
