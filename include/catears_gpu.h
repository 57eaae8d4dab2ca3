/*
 * catears_gpu.h -- C-ABI boundary of the MI355X acoustic-scoring path.
 *
 * The reference (ishine/CatEars, a.k.a. pocketkaldi) computes
 *   PCM -> Fbank::Process -> CMVN::GetFrame -> AcousticModel::Process/EndOfStream
 *       -> Nnet::Propagate -> (- log prior) -> log-likelihood rows
 * on one CPU core, one frame at a time.  This header is the thin extern "C"
 * FFI under which the same path runs as hand-written gfx950 HIP kernels, on
 * whole utterances batched together.  Plain pointers, sizes and opaque
 * handles only; every entry point returns an int status (CE_GPU_OK == 0) and
 * never throws across the ABI.  The message of the last failure on the
 * calling thread is returned by ce_gpu_last_error().
 *
 * Pointers named d_* are device (HBM) pointers; h_* are host pointers.  All
 * device work is enqueued on the context's stream (asynchronous) unless a
 * function says otherwise.
 *
 * No entry asks more of a device pointer than its element's alignment (4
 * bytes for float / int32, 1 for uint8) or more of a leading dimension than
 * ld >= the row's width: a matrix may be a strided view into the middle of a
 * larger allocation.  Aligned, dense rows are faster; no entry writes
 * outside the rows it is given, and the nnet entries (nnet_propagate,
 * nnet_propagate_blocks, am_forward) give the same bits wherever their input
 * and output lie (tests/test_gpu_caller_buffers.py).  ce_gpu_sum_f64 alone
 * documents an order that depends on the alignment.
 *
 * Reference interfaces replaced (all paths relative to the reference root):
 *   Fbank::Process            src/fbank.h:57-59,  src/fbank.cc:265-314
 *   CMVN::CMVN / GetFrame     src/cmvn.h:22-26,   src/cmvn.cc:100-119
 *   AcousticModel::Read       src/am.h:34-35,     src/am.cc:26-64
 *   AcousticModel::Process /
 *   EndOfStream / ComputeBatch src/am.h:41-47,    src/am.cc:82-164
 *   Nnet::Read / Propagate    src/nnet.h:229-232, src/nnet.cc:273-307
 *   MatMat (cblas_sgemm)      src/matrix.h:248-251, src/matrix.cc:300-323
 *   Quantize                  src/matrix.h:238-240, src/matrix.cc:366-387
 *   MatMat_U8U8F32            src/matrix.h:254-260, src/matrix.cc:389-420
 *   ce_stt_last_error         src/ce_stt.h:74-76 (per-thread here, not global)
 */
#ifndef CATEARS_GPU_H_
#define CATEARS_GPU_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CE_GPU_OK 0
#define CE_GPU_EINVAL (-2)    /* bad argument / shape (reference: assert)        */
#define CE_GPU_EHIP (-3)      /* HIP runtime error                                */
#define CE_GPU_EIO (-4)       /* cannot open / read a file (Status::IOError)      */
#define CE_GPU_ECORRUPT (-5)  /* malformed model/config (Status::Corruption)      */
#define CE_GPU_ENOTSUP (-6)   /* model topology this path does not run            */
#define CE_GPU_ENOMEM (-7)    /* device allocation failed (std::bad_alloc)        */

/* Feature geometry fixed at compile time in the reference (src/fbank.h:7-13). */
#define CE_GPU_FBANK_DIM 40
#define CE_GPU_FRAME_SHIFT 160
#define CE_GPU_FRAME_LENGTH 400

typedef struct ce_gpu_ctx ce_gpu_ctx;     /* device + stream + workspaces + fbank tables */
typedef struct ce_gpu_model ce_gpu_model; /* device-resident nnet, log prior, contexts   */
typedef struct ce_gpu_plan ce_gpu_plan;   /* geometry of one batch of utterances         */
typedef struct ce_gpu_sessions ce_gpu_sessions; /* n_slots live audio streams, state in HBM */

/* Message of the last failure on this thread ("" if none). */
const char *ce_gpu_last_error(void);

/* Library version string, "catears-mi355x <abi> (gfx950)".  ABI history
 * (INTEGRATION.md §5): 0.1 round 1; 0.2 ce_gpu_loglik_gather gained `dim`
 * (argument 5) -- a caller built against 0.1 must be rebuilt; 0.3 adds the
 * int16 PCM entry points (ce_gpu_fbank_s16, ce_gpu_score_s16) and the fast
 * fbank mode (ce_gpu_ctx_set_fbank); 0.4 ce_gpu_sum_f64(_many) and
 * ce_gpu_ctx_set_wide_tiles; 0.5 no environment switch in the product
 * library; 0.6 adds the device-resident sessions (ce_gpu_sessions_*) and
 * ce_gpu_debug_counters; 0.7 adds calibrated static int8
 * (ce_gpu_quant_params_from_range, ce_gpu_model_calibrate,
 * ce_gpu_model_quantize_static, ce_gpu_model_quant_params); the latency mode
 * of static int8 (ce_gpu_i8_latency_plan, ce_gpu_debug_i8_latency_launches,
 * the config key gpu_int8_ranges) only adds to 0.7, and so does the plain
 * bf16 GEMM mode (CE_GPU_GEMM_BF16, ce_gpu_gemm_mode_from_name, the config
 * key gpu_gemm), and so do the incremental session sets
 * (ce_gpu_sessions_create_ex, ce_gpu_sessions_stats), and so does the
 * re-layout onto padded widths (ce_gpu_model_pad_widths,
 * ce_gpu_model_padded_widths, the config key gpu_pad_widths), and so do the
 * row steps in the matrix-core programs (ce_gpu_model_admit_row_ops,
 * ce_gpu_debug_rowop_chain, the config key gpu_row_ops), and so do the row
 * steps of a static int8 model that write the next layer's bytes
 * (ce_gpu_debug_rowop_chain_q, ce_gpu_debug_i8_static_launches), and so do
 * the reusable plans (ce_gpu_plan_create_reusable, ce_gpu_plan_assign,
 * ce_gpu_plan_capacity, ce_gpu_debug_plan_tables). */
const char *ce_gpu_version(void);

/* ------------------------------------------------------------ context --- */

/* Create a context on `device` that enqueues on `stream` (a hipStream_t; NULL
 * = the legacy default stream).  Builds the fbank tables on the host with the
 * reference's formulas (Hamming window src/fbank.cc:248-255, mel banks
 * src/fbank.cc:103-163, split-radix tables src/srfft.cc:74-122) and uploads
 * them once. */
int ce_gpu_ctx_create(int device, void *stream, ce_gpu_ctx **out);
int ce_gpu_ctx_destroy(ce_gpu_ctx *ctx);
/* Later calls enqueue on `stream`.  The switch is ordered: `stream` waits
 * (device-side, no host block) for everything already queued on the old
 * stream, which may still be using the context's workspaces -- so the old
 * stream must still be alive when this is called (switch first, destroy the
 * old stream afterwards; destroying a stream the context still uses is
 * undefined, as for any HIP call on a destroyed stream). */
int ce_gpu_ctx_set_stream(ce_gpu_ctx *ctx, void *stream);
/* Block the host until all work enqueued through ctx has finished. */
int ce_gpu_ctx_synchronize(ce_gpu_ctx *ctx);
/* Synchronizes ctx's stream, returns in *overflow whether an f16x3 GEMM
 * (CE_GPU_GEMM_F16X3) met an activation outside its range since the last
 * call, and clears the word.  When set, the log-likelihoods computed through
 * ctx since the last call are not fp32-accurate. */
int ce_gpu_ctx_overflow(ce_gpu_ctx *ctx, int *overflow);
/* Latency mode (on = 1) for callers that score small batches one at a time
 * -- the streaming AcousticModel::Process path (src/am.cc:115-142, a
 * chunk_size + left + right row block per call) or one utterance per call.
 * The fp32 nnet GEMMs of ctx (default bf16x6 mode) then split their K
 * dimension into slices -- at most 256 blocks of 64 output units per row
 * tile, at most 8 K-tiles of 32 per slice: TDNN-S 16 slices for its
 * 3072 x 1024 and 1024 x 1024 layers, 4 for 1024 x 3456 -- each slice loading
 * all its weights at once, and a second kernel sums the slices' partials in
 * slice order (for the last layer, inside the finalize launch).  The slice
 * count depends on K and N only, so results do not depend on the row count
 * and propagate_blocks still returns each block exactly the rows it gets
 * alone.  Results differ from the default mode's only by fp32 summation
 * order.  Measured on MI355X (TDNN-S, one stream): 92 us per 70-row chunk
 * (761 us in the default mode), 390 us per 1018-row utterance (780 us);
 * past ~2000 rows the default mode is faster.  Off (0, the default) is the
 * throughput mode for full 4096-row batches.
 *   Static int8 models (ce_gpu_model_quantize_static): on, a Linear whose row
 * block is at most the measured crossover (ce_gpu_i8_latency_plan returns
 * slices > 0) runs as a split-K pair as well -- int32 slice partials, then a
 * reduce that restores the zero points and writes fp32 or the next layer's
 * bytes.  The accumulators are integers modulo 2^32, so the rows are the
 * bits of the mode off for every split; larger blocks take the throughput
 * kernel automatically, and a caller may leave the mode on for any batch.
 *   Dynamic int8 models (ce_gpu_model_quantize) ignore the mode: their
 * parameters need a reduction over the block first.
 *   Plain bf16 models (CE_GPU_GEMM_BF16): on, every Linear whose row block is
 * at most ce_gpu_bf16_latency_max_rows rows (280) runs on a second kernel that
 * spreads the block over the chip by its outputs -- one wave per 16 units x
 * 16 frames, both operands loaded from global memory straight into a register
 * ring, no LDS, no barrier -- instead of walking K behind one barrier per
 * K-tile.  No split-K: the same MFMA per K-tile in ascending order into one
 * accumulator and the same epilogue, so the rows are the bits of the mode
 * off; larger blocks take the throughput kernels automatically, and a caller
 * may leave the mode on for any batch. */
int ce_gpu_ctx_set_latency(ce_gpu_ctx *ctx, int on);

/* The largest row block that a plain bf16 Linear runs on the latency kernel
 * when its context is in latency mode (the measured crossover), on the host
 * (no device).  The rule depends on the row count only, which it may because
 * the bits do not depend on the kernel.  CE_GPU_EINVAL for NULL. */
int ce_gpu_bf16_latency_max_rows(int *max_rows);

/* The slice rule of the static int8 latency mode, on the host (no device,
 * like ce_gpu_quant_params_from_range): a Linear of `kpad` K-bytes (its K
 * padded to 128) and `n` outputs scored on `rows` rows runs as *slices
 * K-slices of *k_steps_per_slice 64-byte steps each (the last one may hold
 * fewer, never none), about one block per CU.  *slices = 0: the throughput
 * kernel (rows above the crossover, or kpad not a multiple of 128).  The rule
 * may depend on rows because the bits do not.  CE_GPU_EINVAL for a NULL
 * pointer or a non-positive argument. */
int ce_gpu_i8_latency_plan(int kpad, int n, int rows, int *slices, int *k_steps_per_slice);

/* Tile shape of ctx's throughput-mode bf16x6 GEMMs (round 5): on (1), every
 * layer runs the direct-weight kernel on 128 x 128 tiles -- twice the blocks
 * of the 256 x 128 default, so a hidden layer of a 4072-row batch fills all
 * 256 CUs (140 vs 202 us alone) at 38 % more CU time.  For a batch scored
 * while no other is in flight (a pipeline's first and last, or one batch on
 * an idle GPU); the default suits batches that share the chip.  Same bits
 * either way (tests/test_gpu_x6_variants.py).  Replaces nothing in the
 * reference (a scheduling choice of this implementation). */
int ce_gpu_ctx_set_wide_tiles(ce_gpu_ctx *ctx, int on);

/* Fbank kernel of ctx's ce_gpu_fbank / ce_gpu_fbank_s16 / ce_gpu_score*:
 *   CE_GPU_FBANK_EXACT (default) the reference's operation order
 *       (src/fbank.cc:44-245, src/srfft.cc:124-459): pre-log mel energies
 *       bit-identical to Fbank::Process, log-mel within 1e-5;
 *   CE_GPU_FBANK_FAST  the exact kernel's lane program built with FMA
 *       contraction and a single-precision pre-emphasis (23 % fewer
 *       instructions; C2 2.53 vs 2.26 G frames/s on one MI355X): log-mel within
 *       1e-4 of the reference on speech (and of its Kaldi dump), and as close
 *       to the exact float64 result as the reference's own fp32 order is
 *       (max 1.03e-4 vs the reference's 1.07e-4, p99.9 2.7e-5;
 *       tests/test_gpu_fbank_fast.py).  Deterministic: a frame's features
 *       do not depend on the batch it is computed in, nor on the kernels
 *       that run beside it on other streams (bit-identical to a serial
 *       re-score in the pipelined bench, tests/test_gpu_determinism.py;
 *       round 4's four-step fast kernel missed this in ~2 % of launches,
 *       DESIGN.md §8b). */
#define CE_GPU_FBANK_EXACT 0
#define CE_GPU_FBANK_FAST 1
int ce_gpu_ctx_set_fbank(ce_gpu_ctx *ctx, int mode);

/* Kernel timing for roofline reporting: while enabled, every launch of the
 * given kernel class is bracketed by a pair of HIP events on the context's
 * stream.  ce_gpu_ctx_profile_read synchronizes, returns the summed event
 * durations (ms) and launch count of the class since it was enabled, and
 * resets them.  Classes: 0 = TDNN GEMM, A operand in 16-byte vectors
 * (layers whose input width is a multiple of 32); 1 = TDNN GEMM, gathered A
 * (first layer); 2 = fbank; 3 = CMVN; 4 = log-softmax/prior finalize. */
#define CE_GPU_PROF_GEMM 0
#define CE_GPU_PROF_GEMM_GATHER 1
#define CE_GPU_PROF_FBANK 2
#define CE_GPU_PROF_CMVN 3
#define CE_GPU_PROF_FINALIZE 4
#define CE_GPU_PROF_QUANT 5 /* int8 path: per-layer min/max + quantize passes (static int8: also a
                               row-step launch that writes the next Linear's bytes in a pass's place) */
#define CE_GPU_PROF_CLASSES 6
int ce_gpu_ctx_profile(ce_gpu_ctx *ctx, int enable);
/* Restrict the timing to the classes whose bit (1 << class) is set in
 * `mask` (default: all).  Back-to-back GEMM launches of one call share their
 * boundary events, so timing only CE_GPU_PROF_GEMM costs one event record
 * per GEMM launch. */
int ce_gpu_ctx_profile_classes(ce_gpu_ctx *ctx, unsigned mask);
int ce_gpu_ctx_profile_read(ce_gpu_ctx *ctx, int kernel_class, double *total_ms, int64_t *launches);

/* Per-launch intervals for kernels that overlap across streams: record a
 * device-wide time origin on `stream` (before the launches of interest), then
 * read each launch's [start, end] in ms after it.  Consumes the records like
 * profile_read; fails with CE_GPU_EINVAL (and the needed *count) if capacity
 * is too small. */
int ce_gpu_profile_anchor(int device, void *stream);
int ce_gpu_ctx_profile_intervals(ce_gpu_ctx *ctx, int kernel_class, double *h_start_ms, double *h_end_ms,
                                 int capacity, int *count);

/* Window marker for an external kernel trace (rocprofv3 --kernel-trace):
 * launches one empty kernel, catears::trace_mark_kernel, of `tag` (1..64)
 * workgroups on `stream`.  bench.py marks the start (tag 1) and end (tag 2)
 * of its timed steps, and tools/trace_summary.py --window summarises only
 * the launches between the two.  Measurement plumbing; no reference
 * counterpart. */
int ce_gpu_trace_mark(int device, void *stream, int tag);

/* Process-wide counts of the device allocations and releases the library has
 * made so far: every hipMalloc / hipFree behind its buffers, and the pinned
 * host buffers and events of a session set.  A serving loop (or a test)
 * reads them before and after a stretch of calls to show that the stretch
 * allocated nothing.  Either pointer may be NULL.  Measurement plumbing; no
 * reference counterpart. */
int ce_gpu_debug_counters(int64_t *device_allocs, int64_t *device_frees);
/* Process-wide count of the static int8 latency GEMM's launches
 * (i8_lat_gemm_kernel; counted on the host when one is enqueued): shows which
 * of the two int8 kernels a call took.  Measurement plumbing as above. */
int ce_gpu_debug_i8_latency_launches(int64_t *gemms);
/* The same for the plain bf16 latency GEMM (gemm_bf16_lat_kernel). */
int ce_gpu_debug_bf16_latency_launches(int64_t *gemms);
/* One launch of the kernel behind an admitted model's row steps
 * (ce_gpu_model_admit_row_ops), for tests and tools: the n_ops <= 4 row ops
 * h_ops (CE_GPU_ROW_*; h_scale[q] / h_offset[q] device vectors of a
 * BatchNorm) applied in turn to `rows` rows of `dim` columns of d_x, leading
 * dimension ld, in place -- the bits of ce_gpu_rowwise called once per op.
 * With d_out16 the rows leave as bf16 (round to nearest even) there instead,
 * width16 >= dim columns at leading dimension ld16 (the columns behind dim
 * converted as they are; d_x is then working memory).  Enqueues on the
 * context's stream.  Measurement plumbing as above. */
int ce_gpu_debug_rowop_chain(ce_gpu_ctx *ctx, int n_ops, const int *h_ops, int rows, int dim, float *d_x, int ld,
                             const float *const *h_scale, const float *const *h_offset, uint16_t *d_out16, int ld16,
                             int width16);
/* The same launch in the form a static int8 model's row steps end on
 * (ce_gpu_model_quantize_static): the n_ops <= 4 row ops (0: none, a pure
 * quantize) on `rows` rows of `dim` columns of d_x, then every row leaves as
 * the next Linear's input bytes under (scale, zero_point) -- Quantize of one
 * element (src/matrix.cc:378-386) less 128, the bytes of the model's quantize
 * pass -- in d_q, leading dimension ldq >= dim, the bytes [dim, ldq) of a row
 * written as 0; d_rowsum[r] receives row r's sum of those bytes and
 * d_zero[r] is cleared, for r < rows.  d_x is left as it is for dim <= 4096
 * and is working memory beyond.  The parameters travel by value (the entry
 * keeps a device copy of its own).  CE_GPU_EINVAL for n_ops > 4, dim <= 0,
 * ld < dim, ldq < dim or a NULL pointer.  Enqueues on the context's stream.
 * Measurement plumbing as above. */
int ce_gpu_debug_rowop_chain_q(ce_gpu_ctx *ctx, int n_ops, const int *h_ops, int rows, int dim, float *d_x, int ld,
                               const float *const *h_scale, const float *const *h_offset, float scale,
                               int32_t zero_point, int8_t *d_q, int ldq, int32_t *d_rowsum, int32_t *d_zero);
/* Process-wide counts of what the static int8 program has enqueued (counted
 * on the host): quantize passes, row-step launches (one per run of up to four
 * row steps), and those of them that stored the next Linear's bytes in place
 * of a quantize pass.  Shows which hand-over a model's layers took.  Any
 * pointer may be NULL.  Measurement plumbing as above. */
int ce_gpu_debug_i8_static_launches(int64_t *quantize_passes, int64_t *row_launches, int64_t *row_launches_q);
/* Hostile residue for tests (tests/test_gpu_stale_memory.py): the three
 * entries below overwrite device memory the library owns with a 32-bit word
 * of the caller's choice, so that a call which reads such memory before it
 * has written it gives different bits.  Debug only: no product path calls
 * them, and nothing here reads the environment.
 *
 * ce_gpu_debug_fill_allocs is process-wide, like the counters above.  While
 * `on` is nonzero every device allocation the library makes (contexts,
 * models, plans, session sets, workspaces as they grow) is filled with `word`
 * before the allocating call goes on -- the fill is complete when the
 * allocation returns (a trailing 1-3 bytes take the word's low byte).  Off by
 * default; off costs one relaxed atomic load per allocation. */
int ce_gpu_debug_fill_allocs(int on, uint32_t word);
/* Fills, on the context's stream, every device buffer of the context that a
 * call must write before it reads: the nnet activation workspace, the scratch
 * buffer (the spliced first-layer block, int8 operand bytes, row sums,
 * parameters and min / max partials, ce_gpu_quantize's and the u8 GEMM's
 * partials), the latency GEMMs' slice partials, the row maps of
 * ce_gpu_nnet_propagate_blocks and the parameter record of
 * ce_gpu_debug_rowop_chain_q -- whichever of them exist.  Left alone, because
 * they carry an invariant from one call to the next: the fbank tables
 * (constant since ce_gpu_ctx_create), the f16x3 overflow word (sticky until
 * ce_gpu_ctx_overflow reads it) and the experiments library's split-K tickets
 * (zero between launches by construction).  *bytes (may be NULL) receives the
 * bytes filled. */
int ce_gpu_debug_fill_ctx(ce_gpu_ctx *ctx, uint32_t word, int64_t *bytes);
/* Fills, on the stream of the set's context, the set's per-push scratch (the
 * fbank temporary and the device copy of the push descriptor) and, for each
 * of the n slots h_slots names, that slot's regions of the staging buffer,
 * the raw and normalised feature rings and the CMVN carry, and in an
 * incremental set its cached context rows and their row sums.  Meant for a
 * slot after ce_gpu_sessions_reset, which must read none of them before it
 * has rewritten them.  Any slot may be listed: a live slot's later rows are
 * then garbage by design.  n == 0 fills the per-push scratch alone. */
int ce_gpu_debug_fill_sessions(ce_gpu_sessions *s, uint32_t word, int n, const int32_t *h_slots);
/* Downloads one device table of a plan (either kind), for tests and tools:
 * which = 0 sample_off, 1 frame_off (n_utt + 1 int64 each), 2 block_utt
 * (int32 per fbank block, one word for none), 3 row_src, 4 row_dst (int32 per
 * packed row), 5 row_edge (uint32 per packed row) -- the length the current
 * assignment uses, not the capacity.  *bytes receives that length; h_out
 * (capacity_bytes of room; NULL asks for the length alone) receives the
 * words.  Synchronizes the plan's context first.  Measurement plumbing as
 * above. */
int ce_gpu_debug_plan_tables(const ce_gpu_plan *p, int which, void *h_out, int64_t capacity_bytes, int64_t *bytes);

/* -------------------------------------------------------------- model --- */

/* AcousticModel::Read (src/am.cc:26-64): reads the key=value config (keys
 * nnet, prior, left_context, right_context, chunk_size, num_pdfs, tid2pdf;
 * relative paths resolved against the config's directory,
 * src/configuration.cc:52-66), the NN02 nnet (src/nnet.cc:221-293), the VEC0
 * prior (then log, src/am.cc:41-44) and the tid2pdf map; uploads weights.
 * One key of this implementation's own: gpu_int8_ranges = <path> (resolved
 * like nnet / prior) names a VEC0 of 2 * num_linear floats min0 max0 min1
 * max1 ... (ce_gpu_model_quantize_static's h_ranges, e.g. what
 * ce_gpu_model_calibrate returned); the loaded model is then switched with
 * ce_gpu_model_quantize_static.  A wrong count or a bad range fails with
 * that call's CE_GPU_EINVAL text prefixed with the file name.
 * Another: gpu_gemm = <name> (a name of ce_gpu_gemm_mode_from_name) switches
 * the loaded model with ce_gpu_model_set_gemm; an unknown name fails with
 * CE_GPU_EINVAL and the key and value in the text, a mode the model does not
 * allow with CE_GPU_ENOTSUP.  Beside gpu_int8_ranges it is accepted and has
 * no effect (the int8 form wins).
 * A third: gpu_pad_widths = 1 re-lays the loaded model with
 * ce_gpu_model_pad_widths before gpu_gemm is applied, so gpu_gemm = bf16
 * works on a model of any width; a value other than 0 or 1, or the value 1
 * beside gpu_int8_ranges, fails with CE_GPU_EINVAL and the key(s) in the
 * text before anything is uploaded.
 * A fourth: gpu_row_ops = 1 applies ce_gpu_model_admit_row_ops to the loaded
 * model before gpu_pad_widths and gpu_gemm; a value other than 0 or 1 fails
 * with CE_GPU_EINVAL and "gpu_row_ops = <value>" in the text.  Beside
 * gpu_int8_ranges it is accepted and has no effect.
 * Fails with CE_GPU_ENOTSUP for a topology whose whole-utterance result
 * would differ from the reference's chunked one. */
int ce_gpu_model_load_config(ce_gpu_ctx *ctx, const char *config_path, ce_gpu_model **out);

/* The same from explicit files; left/right context as AcousticModel reads
 * them from its config (src/am.cc:48-50). */
int ce_gpu_model_load(ce_gpu_ctx *ctx, const char *nnet_path, const char *prior_path,
                      int left_context, int right_context, ce_gpu_model **out);

/* Shape of a loaded model.  Any output pointer may be NULL. */
int ce_gpu_model_info(const ce_gpu_model *m, int *left_context, int *right_context,
                      int *input_dim, int *num_pdfs, int *num_linear, int64_t *num_params);

/* Switch a loaded model to the int8 path (BASELINE config C5): every
 * LinearLayer becomes Quantize + MatMat_U8U8F32 + bias (src/matrix.cc:329-420
 * -- the pieces the reference ships but never wires into Nnet,
 * src/nnet.cc:29).  Weights are quantized once here, per tensor; activations
 * per layer and per chunk of packed rows (the layer input block, before the
 * splice -- the same parameters as quantizing the spliced block); the int32
 * accumulation is exact (gemmlowp's ring), bias / ReLU / BatchNorm /
 * LogSoftmax stay fp32.  Irreversible for this model handle.
 * Batch dependence: like the reference's per-call Quantize, an activation
 * tensor's (scale, zero point) come from the whole block being scored, so in
 * ce_gpu_am_forward / ce_gpu_score an utterance's int8 log-likelihoods depend
 * on which utterances share its packed chunk.  ce_gpu_nnet_propagate_blocks
 * quantizes every block on its own instead, so there each block gets exactly
 * the rows it gets alone (the AcousticModel batcher's contract).
 * A model in the static int8 form (below) is refused with CE_GPU_EINVAL. */
int ce_gpu_model_quantize(ce_gpu_ctx *ctx, ce_gpu_model *m);

/* ---- calibrated static int8: one frozen (scale, zero point) per Linear ---
 *
 * The dynamic int8 form above takes every activation tensor's parameters
 * from the block being scored.  The static form measures each Linear's input
 * range once on representative audio (ce_gpu_model_calibrate), freezes the
 * parameters of that range in the model (ce_gpu_model_quantize_static) and
 * quantizes every activation with them.
 *
 * Contract: for a static int8 model, every row that ce_gpu_am_forward,
 * ce_gpu_score(_s16), ce_gpu_nnet_propagate, ce_gpu_nnet_propagate_blocks and
 * ce_gpu_sessions_push produce depends only on the input rows it covers.
 * Its bits are the same whatever shares its chunk, whatever the plan's
 * max_rows, and however the audio is pushed; ce_gpu_nnet_propagate windows
 * long blocks and ce_gpu_nnet_propagate_blocks scores all blocks in one
 * launch sequence, as for fp32.  Values outside the calibrated range clamp
 * to byte 0 or 255 (Quantize's clamp, src/matrix.cc:378-386).  The dynamic
 * int8 form keeps its definition, its bits and its CE_GPU_ENOTSUP in
 * sessions. */

/* The (scale, zero point) the reference's Quantize picks for a tensor whose
 * extremes are min and max: FindMinMax's seeding (a max below FLT_MIN becomes
 * FLT_MIN, src/matrix.cc:331-345) followed by ComputeQuantizationParams
 * (src/matrix.cc:348-362): scale = (max - min) / 255 in double, stored as
 * float; zero_point = round(-min / scale), unclamped.  Needs no device.
 * Non-finite input, min > max, or a scale that is not finite and positive:
 * CE_GPU_EINVAL. */
int ce_gpu_quant_params_from_range(float min, float max, float *scale, int32_t *zero_point);

/* Runs the plan's utterances (d_feats: the plan's feature rows, as for
 * ce_gpu_am_forward) through the model in its current GEMM mode
 * (CE_GPU_GEMM_FP32 or CE_GPU_GEMM_BF16X6; the plane modes keep no fp32
 * activations: CE_GPU_ENOTSUP) and folds, per Linear i, the min / max of that
 * Linear's input -- the block entering its Splice, over the rows the
 * reference chain holds there, with FindMinMax's comparisons -- into
 * h_ranges[2 i] and h_ranges[2 i + 1] (num_linear of ce_gpu_model_info
 * pairs).  accumulate = 0 starts from FindMinMax's seeds (FLT_MAX, FLT_MIN);
 * accumulate = 1 folds into the caller's values, so a corpus can be fed batch
 * by batch.  m must not be quantized.  Host-synchronous; allocates. */
int ce_gpu_model_calibrate(ce_gpu_ctx *ctx, const ce_gpu_model *m, const ce_gpu_plan *p, const float *d_feats,
                           int accumulate, float *h_ranges);

/* Switch a loaded model to the static int8 form: weights quantized exactly
 * as ce_gpu_model_quantize does, activations of Linear i with
 * ce_gpu_quant_params_from_range(h_ranges[2 i], h_ranges[2 i + 1]).
 * n_ranges != num_linear or a bad range: CE_GPU_EINVAL, model unchanged.  A
 * model already quantized (either form): CE_GPU_EINVAL.  Irreversible. */
int ce_gpu_model_quantize_static(ce_gpu_ctx *ctx, ce_gpu_model *m, const float *h_ranges, int n_ranges);

/* The frozen activation parameters of a static int8 model, one per Linear
 * (for logging and tests): copies min(capacity, *count) of each; *count = 0
 * for a model that is not static int8.  Either array may be NULL. */
int ce_gpu_model_quant_params(const ce_gpu_model *m, float *h_scale, int32_t *h_zero_point, int capacity,
                              int *count);

/* Matrix-core form of the fp32 Linear layers (LinearLayer::Propagate ->
 * MatMat -> cblas_sgemm, src/nnet.cc:22-36, src/matrix.cc:300-323):
 *   CE_GPU_GEMM_FP32   v_mfma_f32_32x32x2_f32 (exact fp32 products)
 *   CE_GPU_GEMM_BF16X6 every fp32 operand split exactly into three bf16
 *                      planes, six bf16 MFMA products per pair accumulated in
 *                      fp32; the dropped cross terms are < 2^-25 |w x|, below
 *                      one fp32 rounding, so the result is an fp32 GEMM
 *                      (differently ordered sum), on the 16x faster bf16
 *                      matrix cores.  Operands stay fp32 in HBM and are
 *                      split on their way into LDS.
 *   CE_GPU_GEMM_F16X3  every operand, scaled by a power of two, as two fp16
 *                      planes (22-23 significant bits), three fp16 MFMA
 *                      products in two fp32 accumulators; dropped term
 *                      < 2^-22 |w x|.  Log-likelihood error measured equal to
 *                      the FP32 path's.  Hidden activations must stay below
 *                      1.6e7 in magnitude (and finite): otherwise the
 *                      context's overflow word is set (ce_gpu_ctx_overflow)
 *                      and those results must be recomputed in another mode.
 * Models load in CE_GPU_GEMM_BF16X6 when their program allows it (every
 * Linear's input width after the first a multiple of 32, output widths
 * multiples of 4, every ReLU/BatchNorm fused into a Linear), else FP32.
 * F16X3 (22-23 significant bits per operand, not a full fp32 significand)
 * is opt-in.  Only the experiments library (make EXPERIMENTS=1) reads the
 * environment's CATEARS_NNET_GEMM (0-4, the numbers below) as the default;
 * the product library reads no environment.  Setting a mode the model does
 * not allow returns CE_GPU_ENOTSUP. */
#define CE_GPU_GEMM_FP32 0
#define CE_GPU_GEMM_BF16X6 1
#define CE_GPU_GEMM_F16X3 2
/* BF16X6 with the operands kept as bf16 planes in HBM (each layer's
 * epilogue writes its output split; 6 B per element instead of 4).  The same
 * products in the same order as BF16X6: bit-identical results. */
#define CE_GPU_GEMM_BF16X6_PLANES 3
/* Plain bf16: not an fp32-accurate mode, and never a default.  Definition:
 *   - every Linear computes y_j = sum_k bf16(a_k) * bf16(w_kj), bf16(.) the
 *     round-to-nearest-even of the fp32 value; the products are exact and
 *     accumulated in fp32 in ascending K, in one accumulator per output
 *     (one v_mfma_f32_16x16x32_bf16 per 32 k);
 *   - bias / ReLU / BatchNorm are applied in fp32 in the reference's rounding
 *     order, as in the other modes;
 *   - a hidden Linear's output is stored as bf16(y) -- the same function as
 *     rounding at the consumer, since in a program this mode accepts the only
 *     consumer is the next Linear; the last Linear writes fp32, and the
 *     finalize (LogSoftmax, minus log prior) is unchanged;
 *   - every row depends on its own input rows only: its bits do not depend
 *     on the row count, the tile shape the host picks, its position in the
 *     block or what shares the launch (every tile shape uses the one MFMA
 *     shape and K order, and there is no split-K).
 * Same precondition as the other plane modes (CE_GPU_ENOTSUP otherwise).
 * ce_gpu_ctx_set_latency and ce_gpu_ctx_set_wide_tiles are ignored in this
 * mode; ce_gpu_model_calibrate refuses it (CE_GPU_ENOTSUP);
 * ce_gpu_model_quantize(_static) behave as before, the int8 form winning
 * over the GEMM mode.  bf16 has fp32's exponent range: no overflow word.
 * Across layers the result is not independent of the fp32 summation order:
 * a last-place difference in a hidden y can move bf16(y) by 2^-9 relative
 * (DESIGN.md §5). */
#define CE_GPU_GEMM_BF16 4
int ce_gpu_model_set_gemm(ce_gpu_model *m, int mode);
int ce_gpu_model_get_gemm(const ce_gpu_model *m, int *mode);
/* The CE_GPU_GEMM_* number of a mode name: "fp32", "bf16x6", "bf16x6p"
 * (CE_GPU_GEMM_BF16X6_PLANES), "f16x3", "bf16".  Any other name, or a NULL
 * argument: CE_GPU_EINVAL.  Needs no device. */
int ce_gpu_gemm_mode_from_name(const char *name, int *mode);

/* Re-lays a loaded model onto padded layer widths, so that a net of any
 * width can run the matrix-core modes above (and with them latency mode, wide
 * tiles and sessions in bf16x6 / bf16).  Opt-in: a model outside the
 * envelope of CE_GPU_GEMM_BF16X6 still loads as CE_GPU_GEMM_FP32.
 *   Every hidden Linear's output width goes up to the next multiple of 32,
 * the last Linear's to the next multiple of 4; a later Linear's input width
 * is the previous padded width, splice segment s holding its true columns at
 * s * padded_width with zero weight columns behind them.  A padded unit has
 * zero weights, a zero bias and, under a fused BatchNorm, scale 1 and
 * offset 0: its activation is +0 after any post chain, in every mode, and it
 * meets only zero weights in the next layer.  Every weight image is rebuilt,
 * the load-time rule is applied again, and the model ends in the mode it
 * would have loaded in (CE_GPU_GEMM_BF16X6 in the product library).
 *   Definition of the modes on a padded model: a mode's definition applies
 * to the padded program.  A pad contributes products that are exactly zero,
 * so each mode computes the original net under its own definition, with a K
 * order that has zeros inserted at the segment ends: for the fp32-class
 * modes again an fp32 GEMM in another summation order; for CE_GPU_GEMM_BF16
 * every invariance listed above holds unchanged; on exact-integer nets every
 * mode gives the original net's bits.  (Non-finite activations are outside
 * this: 0 * inf is NaN.)
 *   The model keeps the net's own widths: ce_gpu_model_info reports the same
 * input_dim, num_pdfs and num_params as before, no entry point reads or
 * writes a pad column of a caller's buffer, LogSoftmax and the prior run over
 * num_pdfs columns, and ce_gpu_model_calibrate folds the true columns only.
 * In latency mode the last layer's slice reduce is its own launch when that
 * layer was padded (the fused finalize needs num_pdfs % 4 == 0); same bits.
 *   Returns CE_GPU_OK and changes nothing for a model already inside the
 * envelope; CE_GPU_ENOTSUP, nothing changed, for a program with an unfused row
 * op; CE_GPU_EINVAL for an int8 model of either form.  On a padded model
 * ce_gpu_model_quantize and ce_gpu_model_quantize_static return
 * CE_GPU_EINVAL (the int8 programs take any width on the unpadded model, and
 * a zero pad column is not neutral under an unclamped zero point).
 * Irreversible for this model handle.  Host-synchronous; allocates.  Like
 * the quantize entries it belongs right after the load: a session set sizes
 * its caches from the model's widths when it is created. */
int ce_gpu_model_pad_widths(ce_gpu_ctx *ctx, ce_gpu_model *m);

/* Admits a loaded model's row steps to the matrix-core programs.  A layer
 * that cannot be a Linear's fused epilogue -- every Normalize and Softmax, a
 * LogSoftmax that is not the last layer, a fifth post op or a second
 * BatchNorm behind one Linear, any ReLU / BatchNorm behind one of those
 * (NormalizeLayer, SoftmaxLayer, LogSoftmaxLayer, ReLULayer, BatchNormLayer:
 * src/nnet.cc:106-175; the layer loop of Nnet::Propagate, src/nnet.cc:295-307)
 * -- is a step of its own, and a model with one loads as CE_GPU_GEMM_FP32 and
 * takes no other mode.  Opt-in: after this call the load-time rule looks at
 * the Linear layers only, the rule is applied again (a model whose Linears
 * fit the envelope ends in CE_GPU_GEMM_BF16X6 in the product library),
 * ce_gpu_model_set_gemm accepts CE_GPU_GEMM_FP32, CE_GPU_GEMM_BF16X6 and
 * CE_GPU_GEMM_BF16, and ce_gpu_model_pad_widths accepts the model (a row
 * step keeps its true width: Normalize's D and the sums cover true columns
 * only, the pad columns stay +0).  CE_GPU_GEMM_BF16X6_PLANES and
 * CE_GPU_GEMM_F16X3 stay CE_GPU_ENOTSUP for a model that has a row step.
 *   A row step is a function of one fp32 row with exactly ce_gpu_rowwise's
 * arithmetic and summation order, so a given fp32 row gives the same bits in
 * every program, whatever the row count, the leading dimension or latency
 * mode.  fp32 and bf16x6 run the steps in place on the fp32 block the Linear
 * before them wrote (in latency mode after its slice reduce; the fused
 * reduce + finalize is taken only when no row step follows the last Linear).
 * In CE_GPU_GEMM_BF16 a Linear that row steps follow writes fp32, the steps
 * run in fp32 and the last of them stores bf16 (round to nearest even) for
 * the next Linear: a value is still rounded to bf16 exactly once.  An
 * all-zero row under Normalize gives NaN, as in the reference.
 *   Sessions of either kind, ce_gpu_model_calibrate (CE_GPU_GEMM_FP32 and
 * CE_GPU_GEMM_BF16X6; a Linear's range is taken after the row steps before
 * it), ce_gpu_model_quantize and ce_gpu_model_quantize_static work on an
 * admitted model as on any other.
 *   Idempotent.  Returns CE_GPU_OK and changes nothing for a model without a
 * row step; CE_GPU_EINVAL for an int8 model of either form (the int8
 * programs run row steps as they are).  Like ce_gpu_model_pad_widths it
 * belongs right after the load, before pad_widths and set_gemm (the config
 * key gpu_row_ops = 1 applies it there). */
int ce_gpu_model_admit_row_ops(ce_gpu_ctx *ctx, ce_gpu_model *m);

/* Each Linear's output width as the net has it (h_true) and as the model
 * runs it (h_padded; equal unless ce_gpu_model_pad_widths changed it), for
 * logging and tests: copies min(capacity, *count) of each, *count = the
 * number of Linear layers.  Either array may be NULL. */
int ce_gpu_model_padded_widths(const ce_gpu_model *m, int *h_true, int *h_padded, int capacity, int *count);

/* tid2pdf map (AcousticModel::TransitionPdfIdMap, src/am.h:38-40).  Copies
 * min(capacity, size) ints to h_out and returns the size via *size. */
int ce_gpu_model_tid2pdf(const ce_gpu_model *m, int32_t *h_out, int capacity, int *size);
int ce_gpu_model_destroy(ce_gpu_model *m);

/* Nnet::Read (src/nnet.cc:273-293) from an in-memory NN02 image (the bytes
 * Nnet::Read consumes).  h_prior (prior_dim probabilities, log taken as in
 * src/am.cc:40-44) may be NULL for a bare Nnet.  left/right_context < 0 take
 * the context from the network's Narrow layers; otherwise they must agree. */
int ce_gpu_model_load_mem(ce_gpu_ctx *ctx, const void *nnet, int64_t nbytes, const float *h_prior,
                          int prior_dim, int left_context, int right_context, ce_gpu_model **out);

/* Nnet::Read (src/nnet.cc:221-293) without a device: parses an NN02 image
 * exactly as ce_gpu_model_load_mem does -- CE_GPU_EIO "IOError: failed to
 * read: ..." for a truncated image (also for a section whose declared length
 * runs past the end, where the reference would first try to allocate it),
 * CE_GPU_ECORRUPT with the reference's messages for a wrong tag, a VEC0
 * section size, a MAT0 row width or an unknown layer type -- and reports the
 * layer count and the header's left / right context (any pointer may be
 * NULL).  Needs no GPU and touches none. */
int ce_gpu_nnet_check_mem(const void *nnet, int64_t nbytes, int *num_layers, int *left, int *right);

/* --------------------------------------------------------------- plan --- */

/* Frames of one utterance of n samples: 0 if n < 400 else 1 + (n - 400) / 160
 * (src/fbank.cc:35-42, snip-edges). */
int64_t ce_gpu_fbank_num_frames(int64_t num_samples);

/* Describe a batch of n_utt utterances laid out back to back in one PCM
 * buffer (utterance u starts at sample sum_{v<u} h_num_samples[v]).  Frames
 * and log-likelihood rows are laid out the same way (utterance u's rows start
 * at sum_{v<u} T_v).  If `model` is non-NULL the plan also packs the
 * utterances into nnet chunks of at most `max_rows` rows each (T_u + L + R
 * rows per utterance; longer utterances are split into segments that overlap
 * by L + R input rows, which the reference shows gives identical rows,
 * src/am.cc:73-80).  max_rows <= 0 selects 4096. */
int ce_gpu_plan_create(ce_gpu_ctx *ctx, const ce_gpu_model *model, const int64_t *h_num_samples,
                       int n_utt, int max_rows, ce_gpu_plan **out);
/* Totals of a plan; any output may be NULL. */
int ce_gpu_plan_info(const ce_gpu_plan *p, int *n_utt, int64_t *total_samples,
                     int64_t *total_frames, int *n_chunks, int *max_chunk_rows);
/* Per-utterance frame (= log-likelihood row) offsets, n_utt + 1 entries. */
int ce_gpu_plan_frame_offsets(const ce_gpu_plan *p, int64_t *h_out);
int ce_gpu_plan_destroy(ce_gpu_plan *p);

/* A plan whose utterance lengths can be replaced.  Reserves, once, every
 * device table and a ring of pinned descriptor buffers for any assignment of
 * at most max_utts utterances and max_total_samples samples (and, with a
 * model, any packing of those at max_rows; max_rows <= 0 selects 4096).
 * Starts as the empty assignment (n_utt = 0).  Bound to ctx: use it only in
 * calls on that context, and destroy it before the context.  CE_GPU_EINVAL
 * for a non-positive max_utts or max_total_samples and for max_rows smaller
 * than the model's L + R + 1.  Every entry that takes a const ce_gpu_plan *
 * accepts a reusable plan. */
int ce_gpu_plan_create_reusable(ce_gpu_ctx *ctx, const ce_gpu_model *model, int max_utts,
                                int64_t max_total_samples, int max_rows, ce_gpu_plan **out);
/* Replace the lengths: afterwards the plan equals what ce_gpu_plan_create
 * gives for them (tables, chunks, ce_gpu_plan_info, frame offsets).  Ordered
 * on the context's stream behind everything already enqueued with the old
 * lengths.  Allocates, frees and synchronizes nothing: the host writes a
 * descriptor of O(n_utt + segments) words and a kernel expands it into the
 * tables.  The host blocks only when the ring entry it needs still has its
 * copy in flight, that is, only when a ring's worth of assigns are all
 * unfinished.  CE_GPU_EINVAL -- with the plan left at its previous assignment
 * and nothing enqueued -- for n_utt < 0 or above max_utts, a negative length,
 * more than max_total_samples samples in all, and for a plan that came from
 * ce_gpu_plan_create. */
int ce_gpu_plan_assign(ce_gpu_plan *p, const int64_t *h_num_samples, int n_utt);
/* What ce_gpu_plan_create_reusable reserves for a model of context (left,
 * right): the most frames, packed segments and packed rows of any assignment
 * within the capacity.  Host arithmetic only: needs no GPU and touches none.
 * Any output may be NULL. */
int ce_gpu_plan_capacity(int max_utts, int64_t max_total_samples, int max_rows, int left, int right,
                         int64_t *max_frames, int64_t *max_segments, int64_t *max_packed_rows);

/* ------------------------------------------------------------ compute --- */

/* Fbank::Process over every utterance of the plan (one-shot, equivalent to
 * streaming, src/fbank.cc:265-314): d_pcm holds total_samples floats at raw
 * int16 scale (src/pcm_reader.cc:174); d_feats receives total_frames x 40
 * log-mel energies.  If d_mel is non-NULL the pre-log mel energies (same
 * shape) are written too (debug / parity). */
int ce_gpu_fbank(ce_gpu_ctx *ctx, const ce_gpu_plan *p, const float *d_pcm, float *d_feats,
                 float *d_mel);

/* The same from 16-bit PCM as it sits in a WAV payload (little-endian int16,
 * utterances back to back at the plan's sample offsets): the int16 -> float
 * conversion WaveReader::Process does on the host (src/pcm_reader.cc:148-190,
 * :174) happens in the kernel's loads, exactly, so the features are
 * bit-identical to ce_gpu_fbank on the converted floats -- at 2 B per sample
 * of HBM (and PCIe) traffic instead of 4. */
int ce_gpu_fbank_s16(ce_gpu_ctx *ctx, const ce_gpu_plan *p, const int16_t *d_pcm, float *d_feats,
                     float *d_mel);

/* Online CMVN (src/cmvn.cc:35-110) over every utterance: d_global_stats is
 * the 41-float VEC0 payload (40 sums + count); frames are processed in order
 * per utterance exactly like GetFrame(0), GetFrame(1), ...  d_out must not
 * overlap d_feats (the window subtracts frames read 600 steps earlier). */
int ce_gpu_cmvn(ce_gpu_ctx *ctx, const ce_gpu_plan *p, const float *d_global_stats,
                const float *d_feats, float *d_out);

/* AcousticModel::Process* + EndOfStream for every utterance of the plan:
 * d_feats is total_frames x input_dim; d_loglik receives total_frames x
 * num_pdfs rows of nnet output minus log prior (src/am.cc:104-112). */
int ce_gpu_am_forward(ce_gpu_ctx *ctx, const ce_gpu_model *m, const ce_gpu_plan *p,
                      const float *d_feats, float *d_loglik);

/* Nnet::Propagate (src/nnet.cc:295-307) on one block of rows already padded
 * by the caller, optionally followed by AcousticModel::ComputeBatch's prior
 * subtraction (src/am.cc:104-112): d_in is rows x input_dim (row stride ld_in
 * floats), d_out receives (rows - L - R) x num_pdfs where L, R are the rows the
 * network's Narrow layers drop.  rows must exceed L + R (the reference's
 * Narrow passes shorter blocks through unchanged, src/nnet.cc:186-189; that
 * degenerate case is CE_GPU_EINVAL here). */
int ce_gpu_nnet_propagate(ce_gpu_ctx *ctx, const ce_gpu_model *m, const float *d_in, int rows, int ld_in,
                          int subtract_prior, float *d_out);

/* The same over n_blocks independent padded blocks laid back to back in d_in
 * (block b has h_rows[b] > L + R rows); d_out receives every block's
 * rows - L - R output rows back to back.  One launch sequence for all blocks:
 * the call a serving loop makes to score the ready chunks of many streams
 * at once (catears_amd/host AcousticModel batching).  Host-synchronous with
 * respect to the previous call on this context.  Every block's output equals
 * what ce_gpu_nnet_propagate gives for it alone (bit-exact; an int8 model
 * runs the blocks one by one so its quantization parameters stay per block). */
int ce_gpu_nnet_propagate_blocks(ce_gpu_ctx *ctx, const ce_gpu_model *m, const float *d_in, int ld_in,
                                 const int32_t *h_rows, int n_blocks, int subtract_prior, float *d_out);

/* The whole path: fbank -> (CMVN if d_global_stats != NULL) -> nnet -> - log
 * prior.  d_feats_ws must hold 2 x total_frames x 40 floats (features and
 * normalised features). */
int ce_gpu_score(ce_gpu_ctx *ctx, const ce_gpu_model *m, const ce_gpu_plan *p,
                 const float *d_pcm, const float *d_global_stats, float *d_feats_ws,
                 float *d_loglik);

/* ce_gpu_score from 16-bit PCM (ce_gpu_fbank_s16 as its first stage). */
int ce_gpu_score_s16(ce_gpu_ctx *ctx, const ce_gpu_model *m, const ce_gpu_plan *p, const int16_t *d_pcm,
                     const float *d_global_stats, float *d_feats_ws, float *d_loglik);

/* ----------------------------------------------------------- sessions --- */
/* Live audio that arrives in pieces, scored incrementally: the reference's
 * own contract (ce_stt_process feeds Fbank::Process per read, src/fbank.cc:
 * 265-314; CMVN::GetFrame src/cmvn.cc:100-119; AcousticModel::Process per
 * frame, src/am.cc:115-142) for n_slots concurrent streams at once, with
 * every stream's state in HBM: the unconsumed sample tail (at most 399
 * samples), the CMVN running sums and its 600-frame window, and the nnet's
 * left context.  ("Session", because "stream" means a HIP stream here.)
 *
 * Let a slot have received samples x[0..S) since its last reset and F =
 * ce_gpu_fbank_num_frames(S).  After any sequence of pushes ending with
 * CE_GPU_SESSION_EOS the rows the slot produced, concatenated, are
 * bit-identical to the F rows ce_gpu_score / ce_gpu_score_s16 give for the
 * one-utterance plan of x on the same context (same GEMM mode, latency and
 * fbank settings, same d_global_stats or none).  Before EOS a push emits
 * every row whose right context is complete: max(0, F - R) rows in total so
 * far.  Which other slots share a push, and in which order, changes no bit.
 * The host knows every count by arithmetic and never reads device state.
 *
 * A push allocates, frees and synchronizes nothing: its descriptors travel
 * through a ring of pinned buffers with one asynchronous copy, and
 * ce_gpu_sessions_create reserves every workspace (bounded by 4096 packed
 * nnet rows per launch sequence, whatever n_slots x max_chunk_samples is).
 *
 * int8 models: CE_GPU_ENOTSUP (their rows depend on the batch).  A model
 * whose input is not 40-dim fbank or that has no prior: CE_GPU_EINVAL.  One
 * session set per context; calls on it are not thread-safe. */

/* d_global_stats: 41 floats (device, must outlive the set), NULL = no CMVN.
 * max_chunk_samples: the most samples one slot may receive in one push. */
int ce_gpu_sessions_create(ce_gpu_ctx *ctx, const ce_gpu_model *m, const float *d_global_stats,
                           int n_slots, int max_chunk_samples, ce_gpu_sessions **out);
/* The same with flags (0: exactly ce_gpu_sessions_create; an unknown bit:
 * CE_GPU_EINVAL).
 *
 * CE_GPU_SESSIONS_INCREMENTAL: the set keeps, per slot and per Linear, the
 * last c rows of that layer's input (c = the span of the layer's splice
 * indices), so a push of k new positions packs k + H nnet rows per slot (H =
 * the largest c) instead of k + L + R.  The contract of push / push_s16 /
 * reset is unchanged: the same row counts, the same order, the same bits.
 * GEMM modes fp32, bf16x6 and bf16 and static int8, with latency mode on or
 * off; CE_GPU_GEMM_BF16X6_PLANES and CE_GPU_GEMM_F16X3: CE_GPU_ENOTSUP.  The
 * set records the model's form (GEMM mode, static int8) at create; a push
 * after it changed is CE_GPU_EINVAL and changes no state. */
#define CE_GPU_SESSIONS_INCREMENTAL 1u
int ce_gpu_sessions_create_ex(ce_gpu_ctx *ctx, const ce_gpu_model *m, const float *d_global_stats,
                              int n_slots, int max_chunk_samples, unsigned flags, ce_gpu_sessions **out);
/* Host counters since create (no device access; any pointer may be NULL):
 * lead_rows = H (0 when the set is not incremental), the pushes that
 * succeeded (n > 0), the packed nnet rows they scored and the chunks (launch
 * sequences of at most 4096 packed rows) those ran as. */
int ce_gpu_sessions_stats(const ce_gpu_sessions *s, int *lead_rows, int64_t *pushes, int64_t *packed_rows,
                          int64_t *chunks);
/* Waits for the pushes in flight, then frees the set.  Destroy it before its
 * context and its model. */
int ce_gpu_sessions_destroy(ce_gpu_sessions *s);
/* Slot starts a new utterance (ordered on the context's stream, no host block). */
int ce_gpu_sessions_reset(ce_gpu_sessions *s, int slot);

#define CE_GPU_SESSION_EOS 1   /* flag: this push ends the slot's utterance */
/* Advance n distinct slots.  Push i gives slot h_slot[i] h_num_samples[i]
 * (>= 0) new samples, laid back to back in d_pcm in push order (float at raw
 * int16 scale, as ce_gpu_fbank).  h_flags may be NULL (no flags).  d_loglik
 * receives the newly complete log-likelihood rows of push 0, then push 1, ...
 * (num_pdfs floats each); h_rows_out[i] = rows push i produced.  If
 * capacity_rows is too small: CE_GPU_EINVAL, h_rows_out still filled with the
 * needed counts, no state changed, nothing enqueued.  EOS with F == 0 yields
 * no rows; after EOS the slot accepts nothing until it is reset
 * (CE_GPU_EINVAL). */
int ce_gpu_sessions_push(ce_gpu_sessions *s, int n, const int32_t *h_slot, const int32_t *h_num_samples,
                         const int32_t *h_flags, const float *d_pcm, float *d_loglik,
                         int64_t capacity_rows, int32_t *h_rows_out);
/* The same from 16-bit PCM (as ce_gpu_fbank_s16): the same bits. */
int ce_gpu_sessions_push_s16(ce_gpu_sessions *s, int n, const int32_t *h_slot, const int32_t *h_num_samples,
                             const int32_t *h_flags, const int16_t *d_pcm, float *d_loglik,
                             int64_t capacity_rows, int32_t *h_rows_out);

/* ------------------------------------------------------- linear algebra --- */

/* MatMat (src/matrix.cc:300-323): C[m x n] = A[m x k] * B[k x n], all
 * row-major with leading dimensions lda/ldb/ldc (in floats), fp32 in, fp32
 * MFMA accumulate. */
int ce_gpu_sgemm(ce_gpu_ctx *ctx, int m, int n, int k, const float *d_a, int lda,
                 const float *d_b, int ldb, float *d_c, int ldc);

/* Quantize (src/matrix.cc:329-387): per-tensor asymmetric uint8 with the
 * reference's min/max (max initialised to FLT_MIN), scale = (max-min)/255
 * (double, stored float), zero point = round(-min/scale) unclamped.  d_q
 * receives count bytes; the parameters are written to d_params as
 * {float scale, int32 zero_point} (device, 8 bytes) so the call stays
 * asynchronous. */
int ce_gpu_quantize(ce_gpu_ctx *ctx, const float *d_x, int64_t count, uint8_t *d_q,
                    void *d_params);

/* MatMat_U8U8F32 (src/matrix.cc:389-420 -> gemmlowp EightBitIntGemm):
 * C[m x n] = float(int32 sum_k (A-zpA)(B-zpB)) * (sA*sB), A m x k and B k x n
 * row-major uint8, parameters read from the device records written by
 * ce_gpu_quantize.  The int32 accumulator is bit-exact. */
int ce_gpu_gemm_u8u8f32(ce_gpu_ctx *ctx, int m, int n, int k, const uint8_t *d_a,
                        const void *d_params_a, const uint8_t *d_b, const void *d_params_b,
                        float *d_c);

/* The same, int32 accumulators out (no scaling): the quantity gemmlowp's
 * GemmWithOutputPipeline produces before the float stage. */
int ce_gpu_gemm_u8u8i32(ce_gpu_ctx *ctx, int m, int n, int k, const uint8_t *d_a,
                        const void *d_params_a, const uint8_t *d_b, const void *d_params_b,
                        int32_t *d_c);

/* ------------------------------------------------------ layer primitives --- */
/* Single layers for Layer::Propagate (src/nnet.h:34-42) outside a fused
 * program.  All enqueue on the context's stream. */

/* LinearLayer::Propagate (src/nnet.cc:22-43): out = in * W + b, W in_dim x
 * out_dim row-major (MAT0 layout) with row stride ld_w; d_b may be NULL. */
int ce_gpu_linear(ce_gpu_ctx *ctx, int rows, int in_dim, int out_dim, const float *d_in, int ld_in,
                  const float *d_w, int ld_w, const float *d_b, float *d_out, int ld_out);

/* SpliceLayer::Propagate (src/nnet.cc:50-95): out (rows x dim*n_idx, dense)
 * row t = concat_s in[clamp(t + h_idx[s], 0, rows - 1)].  h_idx is host
 * memory, 1 <= n_idx <= CE_GPU_MAX_SPLICE. */
#define CE_GPU_MAX_SPLICE 32
int ce_gpu_splice(ce_gpu_ctx *ctx, int rows, int dim, const float *d_in, int ld_in, const int32_t *h_idx,
                  int n_idx, float *d_out);

/* In-place per-row layers: ReLU (src/nnet.cc:149-160), BatchNorm (x*scale
 * then +offset, :106-123), LogSoftmax (:137-146), Softmax, Normalize
 * (:163-178).  d_scale/d_offset only for BatchNorm. */
#define CE_GPU_ROW_RELU 0
#define CE_GPU_ROW_BATCHNORM 1
#define CE_GPU_ROW_LOGSOFTMAX 2
#define CE_GPU_ROW_SOFTMAX 3
#define CE_GPU_ROW_NORMALIZE 4
int ce_gpu_rowwise(ce_gpu_ctx *ctx, int op, int rows, int dim, float *d_x, int ld, const float *d_scale,
                   const float *d_offset);

/* Decoder::LogLikelihood (src/decoder.cc:97-102) in bulk, on the device:
 *   d_out[i] = am_scale * d_loglik[d_row[i] * ld + d_tid2pdf[d_trans[i]]]
 * for n (frame, transition-id) pairs -- the acoustic costs of a frame's
 * active arcs (ProcessEmitting, src/decoder.cc:327,350 negate them), so a
 * decoder reads n floats instead of whole 3456-wide rows.  `dim` is the row
 * width (num_pdfs, <= ld).  A pair whose frame is outside [0, rows), whose
 * transition id is outside [0, n_tid) or whose pdf (d_tid2pdf entry, e.g.
 * from a corrupt model file) is outside [0, dim) yields NaN (the reference
 * indexes out of bounds there). */
int ce_gpu_loglik_gather(ce_gpu_ctx *ctx, const float *d_loglik, int rows, int ld, int dim,
                         const int32_t *d_tid2pdf,
                         int n_tid, const int32_t *d_row, const int32_t *d_trans, int n, float am_scale,
                         float *d_out);

/* Column subset of a log-likelihood block: d_out[r * n_cols + j] =
 * d_loglik[r * ld + d_cols[j]] (NaN for a column outside [0, dim)) -- the
 * pdfs a decoding graph can reach, compacted before the D2H copy. */
int ce_gpu_loglik_columns(ce_gpu_ctx *ctx, const float *d_loglik, int rows, int ld, int dim,
                          const int32_t *d_cols, int n_cols, float *d_out);

/* *d_acc += the float64 sum of the n floats at d_x, on `stream` (a
 * hipStream_t; NULL = the null stream) of the current device; d_part is
 * device scratch for CE_GPU_SUM_PARTS doubles.  Each element is widened to
 * double before it is added.  Deterministic, not order-free: the summation
 * order depends on n, on whether d_x is 16-byte aligned (float4 or scalar
 * loads) and, in the _many form, on the whole list of buffers (the grid is
 * sized by the largest one and the buffers share per-thread accumulators) --
 * the same buffers at the same alignments give the same bits, the same rows
 * at another offset or folded with other buffers may differ in the last
 * places.  No reference counterpart: the consumer of the
 * log-likelihood rows gathered to rank 0 -- bench.py and
 * catears_amd/shard.py RowGather fold every row into this checksum, at HBM
 * speed where torch's float64 reduction runs at about a third of it. */
#define CE_GPU_SUM_PARTS 1024
int ce_gpu_sum_f64(void *stream, const float *d_x, int64_t n, double *d_part, double *d_acc);
/* The same over up to CE_GPU_SUM_MAX_BUFS buffers in one launch pair (host
 * arrays of device pointers and lengths): rank 0 folds every peer's rows of a
 * step at once, without a launch per peer. */
#define CE_GPU_SUM_MAX_BUFS 16
int ce_gpu_sum_f64_many(void *stream, int count, const float *const *d_x, const int64_t *n, double *d_part,
                        double *d_acc);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* CATEARS_GPU_H_ */
