// nnet_programs.h -- what the entries that run a network (capi.cc, model.cc,
// sessions.cc) need of nnet_programs.cc; score_packed_rows and
// reserve_packed_rows are declared in internal.h.
#pragma once

#include "internal.h"

namespace catears {

// CATEARS_SKIP (measurement builds only, -DCATEARS_DIAG: wrong results, timing
// only): launches left out of every call, to price each stage of a pipeline
// by its absence -- 1 first GEMM layer, 2 finalize, 4 fbank, 8 CMVN, 16 last
// GEMM layer, 32 the hidden GEMM layers, 64 the int8 path's min / max and
// Quantize passes.  0 in the product library.
int diag_skip();

// ce_gpu_model_calibrate's tap: before each Linear runs, the (min, max) of
// its input block (held rows only) is folded into ranges[2 * linear ..].
struct CalibTap {
  float *ranges = nullptr;  // device, 2 per Linear
  void *part = nullptr;     // minmax partials (i8_params_scratch_bytes)
  const uint32_t *row_edge = nullptr;
  int linear = 0;
};

// The index of the program's last Linear step: the one whose output width is
// the leading dimension of the program's output.
size_t last_gemm_step(const ce_gpu_model *m);

// Grows ctx->scratch to `bytes` (the stream is synchronized before a buffer
// still in use is replaced).
int ensure_scratch(ce_gpu_ctx *ctx, size_t bytes);

// Runs the program's steps on `rows` packed rows starting at x (row_map: the
// first layer's packed row -> source row, or NULL for identity), in the
// model's GEMM mode.  Returns the last activation via *y / *ldy, or leaves
// the last layer's reduce to the finalize (*tail, latency mode).
int run_steps(ce_gpu_ctx *ctx, const ce_gpu_model *m, const float *x, int ldx, int rows, const int *row_map,
              const uint32_t *row_edge, const float **y, int *ldy, LatTail *tail = nullptr, CalibTap *tap = nullptr,
              const IncrChunk *inc = nullptr);

// What the static int8 program has enqueued in this process, counted on the
// host (ce_gpu_debug_i8_static_launches): quantize passes, row-step launches
// (one per chain of up to kRowChainMax steps), and those of them that stored
// the next Linear's bytes.
void i8_static_launch_counts(int64_t *quantize_passes, int64_t *row_launches, int64_t *row_launches_q);

// The latency GEMM may defer its last layer's reduce into the finalize only
// when the fused finalize can write the caller's output: it stores 16-byte
// row chunks (launch_lat_finalize), so out and the log prior must be 16-byte
// aligned.  Otherwise the layer keeps its own reduce launch and the ordinary
// finalize (scalar path for unaligned rows) runs -- decided before any GEMM
// is launched.
bool lat_tail_ok(const float *out, const float *log_prior);

// launch_finalize on rows first .. first + rows - 1 of run_steps' output
// (or of its deferred latency tail: the last layer's reduce in the same
// launch)
int finalize_output(ce_gpu_ctx *ctx, const float *y, int ldy, int first, int rows, int dim, bool log_softmax,
                    const float *log_prior, const int *row_dst, float *out, const LatTail &tail = LatTail());

}  // namespace catears
