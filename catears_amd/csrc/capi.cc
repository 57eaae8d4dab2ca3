// capi.cc -- extern "C" entry points of libcatears_hip (include/catears_gpu.h)
// that belong to no object of their own: HIP errors, DevBuf and the
// allocation counters, the experiments library's knobs, launch profiling,
// contexts, batch plans, fbank / CMVN / am_forward / nnet_propagate / score
// with the argument checking around the nnet programs (nnet_programs.cc),
// the stand-alone op entries and the debug entries.  The model object and the
// ce_gpu_model_* entries are in model.cc, the sessions in sessions.cc.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "internal.h"
#include "model_io.h"
#include "nnet_programs.h"

namespace catears {

// ---------------------------------------------------------------- errors --

int hip_fail(hipError_t e, const char *what) {
  return fail(CE_GPU_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

// ---------------------------------------------------------------- DevBuf --

// ce_gpu_debug_counters
static std::atomic<int64_t> g_device_allocs{0}, g_device_frees{0};
void count_device_alloc() { g_device_allocs.fetch_add(1, std::memory_order_relaxed); }
void count_device_free() { g_device_frees.fetch_add(1, std::memory_order_relaxed); }

// ce_gpu_debug_fill_allocs
static std::atomic<int> g_fill_allocs{0};
static std::atomic<uint32_t> g_fill_word{0};

int debug_fill(hipStream_t s, void *p, size_t bytes, uint32_t word, int64_t *total) {
  if (!p || bytes == 0) return CE_GPU_OK;
  const size_t words = bytes / 4, rest = bytes % 4;
  if (words) CE_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p), (int)word, words, s));
  if (rest) CE_HIP(hipMemsetAsync(static_cast<char *>(p) + words * 4, (int)(word & 0xff), rest, s));
  if (total) *total += (int64_t)bytes;
  return CE_GPU_OK;
}

int DevBuf::alloc(size_t n) {
  release();
  if (n == 0) return CE_GPU_OK;
  hipError_t e = hipMalloc(&ptr, n);
  if (e != hipSuccess) {
    ptr = nullptr;
    (void)hipGetLastError();
    return fail(CE_GPU_ENOMEM, fmt("hipMalloc(%zu) failed: %s", n, hipGetErrorString(e)));
  }
  count_device_alloc();
  bytes = n;
  if (g_fill_allocs.load(std::memory_order_relaxed)) {
    // ce_gpu_debug_fill_allocs: nothing may take a fresh allocation for zeros.
    // The null stream and a device-wide wait: the buffer's first user may be
    // on any stream, a non-blocking one included.
    CE_TRY(debug_fill(nullptr, ptr, n, g_fill_word.load(std::memory_order_relaxed)));
    CE_HIP(hipDeviceSynchronize());
  }
  return CE_GPU_OK;
}

int DevBuf::upload(const void *src, size_t n) {
  CE_TRY(alloc(n));
  if (n) CE_HIP(hipMemcpy(ptr, src, n, hipMemcpyHostToDevice));
  return CE_GPU_OK;
}

void DevBuf::release() {
  if (ptr) {
    (void)hipFree(ptr);
    count_device_free();
  }
  ptr = nullptr;
  bytes = 0;
}

#ifdef CATEARS_DIAG
int knob_env(const char *name, int dflt) {
  const char *e = getenv(name);
  return e && *e ? atoi(e) : dflt;
}
#endif

// ------------------------------------------------------------ profiling --

static hipEvent_t pool_event(ce_gpu_ctx *ctx) {
  if (!ctx->event_pool.empty()) {
    hipEvent_t e = ctx->event_pool.back();
    ctx->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

ProfScope::ProfScope(ce_gpu_ctx *c, int k) : ctx(c), cls(k) {
  if (!ctx->profiling || !(ctx->prof_mask & (1u << cls))) {
    ctx->chain_end = nullptr;  // an untimed launch breaks a chain
    return;
  }
  hipEvent_t a = nullptr;
  bool own_a = true;
  if (ctx->chain_open && ctx->chain_end && ctx->chain_cls == cls) {
    a = ctx->chain_end;
    own_a = false;
  } else {
    a = pool_event(ctx);
    if (!a) return;
  }
  b = pool_event(ctx);
  if (!b) {
    if (own_a) ctx->event_pool.push_back(a);
    ctx->chain_end = nullptr;
    return;
  }
  if (own_a) (void)hipEventRecord(a, ctx->stream);
  ctx->timed.push_back({cls, a, b, own_a});
}

ProfScope::~ProfScope() {
  if (!b) return;
  (void)hipEventRecord(b, ctx->stream);
  if (ctx->chain_open) {
    ctx->chain_end = b;
    ctx->chain_cls = cls;
  }
}

}  // namespace catears

using namespace catears;

// =================================================================== ABI ==

extern "C" {

const char *ce_gpu_last_error(void) { return last_error(); }

const char *ce_gpu_version(void) { return "catears-mi355x 0.7 (gfx950)"; }

int ce_gpu_ctx_create(int device, void *stream, ce_gpu_ctx **out) {
  if (!out) return fail(CE_GPU_EINVAL, "out is NULL");
  *out = nullptr;
  int n = 0;
  CE_HIP(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(CE_GPU_EINVAL, fmt("no HIP device %d (have %d)", device, n));
  CE_HIP(hipSetDevice(device));
  std::unique_ptr<ce_gpu_ctx> c(new (std::nothrow) ce_gpu_ctx());
  if (!c) return fail(CE_GPU_ENOMEM, "out of host memory");
  c->device = device;
  c->stream = static_cast<hipStream_t>(stream);
  build_fbank_tables(&c->host_tables);
  CE_TRY(c->d_tables.upload(&c->host_tables, sizeof(FbankTables)));
  *out = c.release();
  return CE_GPU_OK;
}

int ce_gpu_ctx_destroy(ce_gpu_ctx *ctx) {
  if (!ctx) return CE_GPU_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (auto &t : ctx->timed) {
    if (t.own_a) (void)hipEventDestroy(t.a);
    (void)hipEventDestroy(t.b);
  }
  for (hipEvent_t e : ctx->event_pool) (void)hipEventDestroy(e);
  delete ctx;
  return CE_GPU_OK;
}

int ce_gpu_ctx_set_stream(ce_gpu_ctx *ctx, void *stream) {
  if (!ctx) return fail(CE_GPU_EINVAL, "ctx is NULL");
  hipStream_t next = static_cast<hipStream_t>(stream);
  if (next != ctx->stream) {
    // Work already queued on the old stream may still use the context's
    // workspaces; the new stream starts after it (no host wait).
    CE_HIP(hipSetDevice(ctx->device));
    hipEvent_t done;
    CE_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    hipError_t e = hipEventRecord(done, ctx->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(next, done, 0);
    (void)hipEventDestroy(done);
    CE_HIP(e);
    ctx->stream = next;
  }
  return CE_GPU_OK;
}

int ce_gpu_ctx_overflow(ce_gpu_ctx *ctx, int *overflow) {
  if (!ctx || !overflow) return fail(CE_GPU_EINVAL, "NULL argument");
  *overflow = 0;
  if (!ctx->overflow.ptr) return CE_GPU_OK;
  CE_HIP(hipSetDevice(ctx->device));
  CE_HIP(hipStreamSynchronize(ctx->stream));
  CE_HIP(hipMemcpy(overflow, ctx->overflow.ptr, sizeof(int), hipMemcpyDeviceToHost));
  CE_HIP(hipMemset(ctx->overflow.ptr, 0, sizeof(int)));
  return CE_GPU_OK;
}

int ce_gpu_ctx_set_latency(ce_gpu_ctx *ctx, int on) {
  if (!ctx) return fail(CE_GPU_EINVAL, "NULL argument");
  ctx->latency = on ? 1 : 0;
  return CE_GPU_OK;
}

int ce_gpu_ctx_set_wide_tiles(ce_gpu_ctx *ctx, int on) {
  if (!ctx) return fail(CE_GPU_EINVAL, "NULL argument");
  ctx->wide_tiles = on ? 1 : 0;
  return CE_GPU_OK;
}

int ce_gpu_ctx_set_fbank(ce_gpu_ctx *ctx, int mode) {
  if (!ctx) return fail(CE_GPU_EINVAL, "NULL argument");
  if (mode != CE_GPU_FBANK_EXACT && mode != CE_GPU_FBANK_FAST) return fail(CE_GPU_EINVAL, "unknown fbank mode");
  ctx->fbank_mode = mode;
  return CE_GPU_OK;
}

int ce_gpu_ctx_synchronize(ce_gpu_ctx *ctx) {
  if (!ctx) return fail(CE_GPU_EINVAL, "ctx is NULL");
  CE_HIP(hipStreamSynchronize(ctx->stream));
  return CE_GPU_OK;
}

int ce_gpu_ctx_profile(ce_gpu_ctx *ctx, int enable) {
  if (!ctx) return fail(CE_GPU_EINVAL, "ctx is NULL");
  ctx->profiling = enable != 0;
  return CE_GPU_OK;
}

int ce_gpu_ctx_profile_classes(ce_gpu_ctx *ctx, unsigned mask) {
  if (!ctx) return fail(CE_GPU_EINVAL, "ctx is NULL");
  ctx->prof_mask = mask;
  return CE_GPU_OK;
}

int ce_gpu_ctx_profile_read(ce_gpu_ctx *ctx, int kernel_class, double *total_ms, int64_t *launches) {
  if (!ctx || kernel_class < 0 || kernel_class >= CE_GPU_PROF_CLASSES) return fail(CE_GPU_EINVAL, "bad argument");
  CE_HIP(hipStreamSynchronize(ctx->stream));
  double ms = 0.0;
  int64_t n = 0;
  std::vector<ce_gpu_ctx::Timed> keep;
  for (const ce_gpu_ctx::Timed &t : ctx->timed) {
    if (t.cls != kernel_class) {
      keep.push_back(t);
      continue;
    }
    float e = 0.0f;
    CE_HIP(hipEventElapsedTime(&e, t.a, t.b));
    ms += e;
    ++n;
    if (t.own_a) ctx->event_pool.push_back(t.a);
    ctx->event_pool.push_back(t.b);
  }
  ctx->timed.swap(keep);
  if (total_ms) *total_ms = ms;
  if (launches) *launches = n;
  return CE_GPU_OK;
}

static hipEvent_t g_anchor[64];

int ce_gpu_profile_anchor(int device, void *stream) {
  if (device < 0 || device >= 64) return fail(CE_GPU_EINVAL, "bad device");
  CE_HIP(hipSetDevice(device));
  if (!g_anchor[device]) CE_HIP(hipEventCreate(&g_anchor[device]));
  CE_HIP(hipEventRecord(g_anchor[device], static_cast<hipStream_t>(stream)));
  return CE_GPU_OK;
}

int ce_gpu_debug_counters(int64_t *device_allocs, int64_t *device_frees) {
  if (device_allocs) *device_allocs = g_device_allocs.load(std::memory_order_relaxed);
  if (device_frees) *device_frees = g_device_frees.load(std::memory_order_relaxed);
  return CE_GPU_OK;
}

int ce_gpu_debug_i8_latency_launches(int64_t *gemms) {
  if (gemms) *gemms = i8_lat_launch_count();
  return CE_GPU_OK;
}

int ce_gpu_i8_latency_plan(int kpad, int n, int rows, int *slices, int *k_steps_per_slice) {
  if (!slices || !k_steps_per_slice) return fail(CE_GPU_EINVAL, "NULL argument");
  if (kpad <= 0 || n <= 0 || rows <= 0) return fail(CE_GPU_EINVAL, "i8_latency_plan: kpad, n and rows must be positive");
  i8_lat_plan(kpad, n, rows, slices, k_steps_per_slice);
  return CE_GPU_OK;
}

int ce_gpu_debug_bf16_latency_launches(int64_t *gemms) {
  if (gemms) *gemms = b16_lat_launch_count();
  return CE_GPU_OK;
}

int ce_gpu_bf16_latency_max_rows(int *max_rows) {
  if (!max_rows) return fail(CE_GPU_EINVAL, "NULL argument");
  *max_rows = b16_lat_max_rows();
  return CE_GPU_OK;
}

int ce_gpu_trace_mark(int device, void *stream, int tag) {
  if (device < 0 || device >= 64 || tag < 1 || tag > 64) return fail(CE_GPU_EINVAL, "bad device or tag");
  CE_HIP(hipSetDevice(device));
  return launch_trace_mark(static_cast<hipStream_t>(stream), tag);
}

int ce_gpu_ctx_profile_intervals(ce_gpu_ctx *ctx, int kernel_class, double *h_start_ms, double *h_end_ms,
                                 int capacity, int *count) {
  if (!ctx || !count || kernel_class < 0 || kernel_class >= CE_GPU_PROF_CLASSES)
    return fail(CE_GPU_EINVAL, "bad argument");
  hipEvent_t anchor = ctx->device < 64 ? g_anchor[ctx->device] : nullptr;
  if (!anchor) return fail(CE_GPU_EINVAL, "no anchor recorded (ce_gpu_profile_anchor)");
  CE_HIP(hipStreamSynchronize(ctx->stream));
  CE_HIP(hipEventSynchronize(anchor));
  int n = 0;
  for (const ce_gpu_ctx::Timed &t : ctx->timed) n += t.cls == kernel_class;
  *count = n;
  if (n > capacity || (n > 0 && (!h_start_ms || !h_end_ms)))
    return fail(CE_GPU_EINVAL, fmt("capacity %d < %d launches", capacity, n));
  std::vector<ce_gpu_ctx::Timed> keep;
  int i = 0;
  for (const ce_gpu_ctx::Timed &t : ctx->timed) {
    if (t.cls != kernel_class) {
      keep.push_back(t);
      continue;
    }
    float a = 0.0f, b = 0.0f;
    CE_HIP(hipEventElapsedTime(&a, anchor, t.a));
    CE_HIP(hipEventElapsedTime(&b, anchor, t.b));
    h_start_ms[i] = a;
    h_end_ms[i] = b;
    ++i;
    if (t.own_a) ctx->event_pool.push_back(t.a);
    ctx->event_pool.push_back(t.b);
  }
  ctx->timed.swap(keep);
  return CE_GPU_OK;
}

int64_t ce_gpu_fbank_num_frames(int64_t n) {
  return n < kWinLen ? 0 : 1 + (n - kWinLen) / kShift;
}

int ce_gpu_plan_create(ce_gpu_ctx *ctx, const ce_gpu_model *model, const int64_t *h_num_samples, int n_utt,
                       int max_rows, ce_gpu_plan **out) {
  if (!ctx || !out || n_utt < 0 || (n_utt > 0 && !h_num_samples)) return fail(CE_GPU_EINVAL, "bad argument");
  *out = nullptr;
  CE_HIP(hipSetDevice(ctx->device));
  std::unique_ptr<ce_gpu_plan> p(new (std::nothrow) ce_gpu_plan());
  if (!p) return fail(CE_GPU_ENOMEM, "out of host memory");
  p->ctx = ctx;
  p->device = ctx->device;
  p->n_utt = n_utt;
  p->sample_off.assign(n_utt + 1, 0);
  p->frame_off.assign(n_utt + 1, 0);
  for (int u = 0; u < n_utt; ++u) {
    if (h_num_samples[u] < 0) return fail(CE_GPU_EINVAL, "negative sample count");
    p->sample_off[u + 1] = p->sample_off[u] + h_num_samples[u];
    p->frame_off[u + 1] = p->frame_off[u] + ce_gpu_fbank_num_frames(h_num_samples[u]);
  }
  p->total_samples = p->sample_off[n_utt];
  p->total_frames = p->frame_off[n_utt];
  if (p->total_frames >= (int64_t)INT32_MAX) return fail(CE_GPU_EINVAL, "too many frames in one plan");
  // fbank block -> first utterance
  const int fpb = fbank_frames_per_block();
  const int64_t blocks = (p->total_frames + fpb - 1) / fpb;
  std::vector<int32_t> block_utt(std::max<int64_t>(blocks, 1), 0);
  {
    int u = 0;
    for (int64_t b = 0; b < blocks; ++b) {
      while (p->frame_off[u + 1] <= b * fpb) ++u;
      block_utt[b] = u;
    }
  }
  p->fbank_blocks = (int)blocks;
  CE_TRY(p->d_sample_off.upload(p->sample_off.data(), p->sample_off.size() * 8));
  CE_TRY(p->d_frame_off.upload(p->frame_off.data(), p->frame_off.size() * 8));
  CE_TRY(p->d_block_utt.upload(block_utt.data(), block_utt.size() * 4));

  if (model) {
    const int L = model->left, R = model->right;
    if (max_rows <= 0) max_rows = 4096;
    if (max_rows < L + R + 1) return fail(CE_GPU_EINVAL, "max_rows smaller than the nnet context");
    p->has_model = true;
    p->left = L;
    p->right = R;
    std::vector<int32_t> src, dst;
    std::vector<uint32_t> edge;
    ce_gpu_plan::Chunk cur;
    auto close = [&]() {
      if (cur.rows > 0) {
        p->max_chunk_rows = std::max(p->max_chunk_rows, cur.rows);
        p->chunks.push_back(cur);
      }
      cur = ce_gpu_plan::Chunk();
      cur.map_base = (int64_t)src.size();
    };
    cur.map_base = 0;
    for (int u = 0; u < n_utt; ++u) {
      const int64_t T = p->frame_off[u + 1] - p->frame_off[u];
      int64_t t = 0;
      while (t < T) {
        int64_t room = max_rows - cur.rows - L - R;
        if (room < T - t && cur.rows > 0) {  // start the utterance in a fresh chunk
          close();
          room = max_rows - L - R;
        }
        const int64_t n = std::min(T - t, room);
        const int64_t seg_rows = n + L + R;
        for (int64_t j = 0; j < seg_rows; ++j) {
          edge.push_back(row_edge_word(j, seg_rows - 1 - j));
          int64_t fr = t - L + j;
          fr = fr < 0 ? 0 : (fr > T - 1 ? T - 1 : fr);
          src.push_back((int32_t)(p->frame_off[u] + fr));
          dst.push_back(j >= L && j < L + n ? (int32_t)(p->frame_off[u] + t + j - L) : -1);
        }
        cur.rows += (int)(n + L + R);
        t += n;
      }
    }
    close();
    if (!src.empty()) {
      CE_TRY(p->d_row_src.upload(src.data(), src.size() * 4));
      CE_TRY(p->d_row_dst.upload(dst.data(), dst.size() * 4));
      CE_TRY(p->d_row_edge.upload(edge.data(), edge.size() * 4));
    }
  }
  *out = p.release();
  return CE_GPU_OK;
}

int ce_gpu_plan_info(const ce_gpu_plan *p, int *n_utt, int64_t *total_samples, int64_t *total_frames,
                     int *n_chunks, int *max_chunk_rows) {
  if (!p) return fail(CE_GPU_EINVAL, "plan is NULL");
  if (n_utt) *n_utt = p->n_utt;
  if (total_samples) *total_samples = p->total_samples;
  if (total_frames) *total_frames = p->total_frames;
  if (n_chunks) *n_chunks = (int)p->chunks.size();
  if (max_chunk_rows) *max_chunk_rows = p->max_chunk_rows;
  return CE_GPU_OK;
}

int ce_gpu_plan_frame_offsets(const ce_gpu_plan *p, int64_t *h_out) {
  if (!p || !h_out) return fail(CE_GPU_EINVAL, "NULL argument");
  memcpy(h_out, p->frame_off.data(), sizeof(int64_t) * p->frame_off.size());
  return CE_GPU_OK;
}

int ce_gpu_plan_destroy(ce_gpu_plan *p) {
  if (p) plan_release_ring(p);  // a reusable plan's pinned descriptor ring (plans.cc)
  delete p;
  return CE_GPU_OK;
}

int ce_gpu_fbank(ce_gpu_ctx *ctx, const ce_gpu_plan *p, const float *d_pcm, float *d_feats, float *d_mel) {
  if (!ctx || !p || (p->total_frames > 0 && (!d_pcm || !d_feats))) return fail(CE_GPU_EINVAL, "NULL argument");
  ProfScope prof(ctx, CE_GPU_PROF_FBANK);
  if (diag_skip() & 4) return CE_GPU_OK;
  const FbankTables *t = ctx->d_tables.as<FbankTables>();
#ifdef CATEARS_EXPERIMENTS
  // timing only: phase A without its lane-dependent twiddle cases
  static const int nocase = CE_KNOB("CATEARS_FB_NOCASE", 0);
  if (nocase && ctx->fbank_mode != CE_GPU_FBANK_FAST) return launch_fbank_nocase(ctx->stream, t, p, d_pcm, d_feats, d_mel);
#endif
  return ctx->fbank_mode == CE_GPU_FBANK_FAST ? launch_fbank_fma(ctx->stream, t, p, d_pcm, d_feats, d_mel)
                                              : launch_fbank(ctx->stream, t, p, d_pcm, d_feats, d_mel);
}

int ce_gpu_fbank_s16(ce_gpu_ctx *ctx, const ce_gpu_plan *p, const int16_t *d_pcm, float *d_feats, float *d_mel) {
  if (!ctx || !p || (p->total_frames > 0 && (!d_pcm || !d_feats))) return fail(CE_GPU_EINVAL, "NULL argument");
  ProfScope prof(ctx, CE_GPU_PROF_FBANK);
  const FbankTables *t = ctx->d_tables.as<FbankTables>();
  return ctx->fbank_mode == CE_GPU_FBANK_FAST ? launch_fbank_fma_s16(ctx->stream, t, p, d_pcm, d_feats, d_mel)
                                              : launch_fbank_s16(ctx->stream, t, p, d_pcm, d_feats, d_mel);
}

int ce_gpu_cmvn(ce_gpu_ctx *ctx, const ce_gpu_plan *p, const float *d_global_stats, const float *d_feats,
                float *d_out) {
  if (!ctx || !p || !d_global_stats || (p->total_frames > 0 && (!d_feats || !d_out)))
    return fail(CE_GPU_EINVAL, "NULL argument");
  const char *a = reinterpret_cast<const char *>(d_feats), *b = reinterpret_cast<const char *>(d_out);
  const size_t bytes = (size_t)p->total_frames * kMel * sizeof(float);
  if (bytes && a < b + bytes && b < a + bytes) return fail(CE_GPU_EINVAL, "cmvn: d_out overlaps d_feats");
  ProfScope prof(ctx, CE_GPU_PROF_CMVN);
  if (diag_skip() & 8) return CE_GPU_OK;
  return launch_cmvn(ctx->stream, p, d_global_stats, d_feats, d_out);
}


int ce_gpu_am_forward(ce_gpu_ctx *ctx, const ce_gpu_model *m, const ce_gpu_plan *p, const float *d_feats,
                      float *d_loglik) {
  if (!ctx || !m || !p) return fail(CE_GPU_EINVAL, "NULL argument");
  if (!p->has_model || p->left != m->left || p->right != m->right)
    return fail(CE_GPU_EINVAL, "plan was not built for this model's context");
  if (p->chunks.empty()) return CE_GPU_OK;
  if (!d_feats || !d_loglik) return fail(CE_GPU_EINVAL, "NULL argument");
  if (!m->log_prior.ptr) return fail(CE_GPU_EINVAL, "am_forward needs a model loaded with a prior");
  if (m->left != m->net_left || m->right != m->net_right)
    return fail(CE_GPU_EINVAL, "model context differs from its network's");
  for (const ce_gpu_plan::Chunk &c : p->chunks) {
    CE_TRY(score_packed_rows(ctx, m, d_feats, c.rows, p->d_row_src.as<int>() + c.map_base,
                             p->d_row_edge.as<uint32_t>() + c.map_base, p->d_row_dst.as<int>() + c.map_base,
                             d_loglik));
  }
  return CE_GPU_OK;
}

int ce_gpu_nnet_propagate(ce_gpu_ctx *ctx, const ce_gpu_model *m, const float *d_in, int rows, int ld_in,
                          int subtract_prior, float *d_out) {
  if (!ctx || !m || !d_in || !d_out) return fail(CE_GPU_EINVAL, "NULL argument");
  if (ld_in < m->input_dim) return fail(CE_GPU_EINVAL, "ld_in smaller than the nnet input");
  const int out_rows = rows - m->net_left - m->net_right;
  if (out_rows <= 0)
    return fail(CE_GPU_EINVAL, fmt("nnet_propagate: %d rows do not cover the network context (%d, %d)", rows,
                                   m->net_left, m->net_right));
  if (subtract_prior && !m->log_prior.ptr) return fail(CE_GPU_EINVAL, "model has no prior");
  const int ctx_rows = m->net_left + m->net_right;
  if ((!m->int8 || m->int8_static) && rows > kPropagateWindow) {
    // A very long block (hours of audio in one call) runs as overlapping
    // windows: output row t needs input rows t .. t + L + R only, so the
    // windows give the same bits as one pass, keep every GEMM operand well
    // inside the kernels' 32-bit row offsets and bound the workspace.  (A
    // dynamic int8 model quantizes per call, so it keeps the single pass; a
    // static one has frozen parameters and is windowed like fp32.)
    const int step = kPropagateWindow - ctx_rows;
    for (int o = 0; o < out_rows; o += step) {
      const int n = std::min(step, out_rows - o);
      CE_TRY(ce_gpu_nnet_propagate(ctx, m, d_in + (size_t)o * ld_in, n + ctx_rows, ld_in, subtract_prior,
                                   d_out + (size_t)o * m->num_pdfs));
    }
    return CE_GPU_OK;
  }
  const float *y = nullptr;
  int ldy = 0;
  LatTail tail;
  CE_TRY(run_steps(ctx, m, d_in, ld_in, rows, nullptr, nullptr, &y, &ldy,
                   lat_tail_ok(d_out, m->log_prior.as<float>()) ? &tail : nullptr));
  ProfScope prof(ctx, CE_GPU_PROF_FINALIZE);
  return finalize_output(ctx, y, ldy, m->net_left, out_rows, m->num_pdfs, m->final_log_softmax,
                         subtract_prior ? m->log_prior.as<float>() : nullptr, nullptr, d_out, tail);
}

int ce_gpu_nnet_propagate_blocks(ce_gpu_ctx *ctx, const ce_gpu_model *m, const float *d_in, int ld_in,
                                 const int32_t *h_rows, int n_blocks, int subtract_prior, float *d_out) {
  if (!ctx || !m || !d_in || !d_out || !h_rows || n_blocks < 1) return fail(CE_GPU_EINVAL, "bad argument");
  if (ld_in < m->input_dim) return fail(CE_GPU_EINVAL, "ld_in smaller than the nnet input");
  if (subtract_prior && !m->log_prior.ptr) return fail(CE_GPU_EINVAL, "model has no prior");
  const int L = m->net_left, R = m->net_right;
  int64_t total = 0;
  for (int b = 0; b < n_blocks; ++b) {
    if (h_rows[b] <= L + R)
      return fail(CE_GPU_EINVAL, fmt("nnet_propagate_blocks: block %d has %d rows, context is (%d, %d)", b,
                                     h_rows[b], L, R));
    total += h_rows[b];
  }
  if (total >= INT32_MAX / 2) return fail(CE_GPU_EINVAL, "too many rows");
  if (m->int8 && !m->int8_static) {
    // per-tensor activation parameters are reduced over the block being
    // scored: one block per call keeps each block's rows its own
    const float *in = d_in;
    float *o = d_out;
    for (int b = 0; b < n_blocks; ++b) {
      CE_TRY(ce_gpu_nnet_propagate(ctx, m, in, h_rows[b], ld_in, subtract_prior, o));
      in += (size_t)h_rows[b] * ld_in;
      o += (size_t)(h_rows[b] - L - R) * m->num_pdfs;
    }
    return CE_GPU_OK;
  }
  const int rows = (int)total;
  // per packed row: output row (or -1) and distances to its block's edges;
  // written only after the previous call's kernels are done with them
  CE_HIP(hipStreamSynchronize(ctx->stream));
  ctx->h_blk_maps.resize(2 * (size_t)rows);
  int32_t *dst = ctx->h_blk_maps.data();
  uint32_t *edge = reinterpret_cast<uint32_t *>(dst + rows);
  int r = 0, out = 0;
  for (int b = 0; b < n_blocks; ++b) {
    const int n = h_rows[b];
    for (int j = 0; j < n; ++j, ++r) {
      dst[r] = (j >= L && j < n - R) ? out++ : -1;
      edge[r] = row_edge_word(j, n - 1 - j);
    }
  }
  const size_t bytes = ctx->h_blk_maps.size() * 4;
  if (ctx->blk_maps.bytes < bytes) CE_TRY(ctx->blk_maps.alloc(bytes));
  CE_HIP(hipMemcpyAsync(ctx->blk_maps.ptr, ctx->h_blk_maps.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
  const int32_t *d_dst = ctx->blk_maps.as<int32_t>();
  const uint32_t *d_edge = reinterpret_cast<const uint32_t *>(d_dst + rows);
  const float *y = nullptr;
  int ldy = 0;
  // blocks are independent: the rows a Splice reads across a block boundary
  // only feed rows that block's Narrow drops
  LatTail tail;
  CE_TRY(run_steps(ctx, m, d_in, ld_in, rows, nullptr, d_edge, &y, &ldy,
                   lat_tail_ok(d_out, m->log_prior.as<float>()) ? &tail : nullptr));
  ProfScope prof(ctx, CE_GPU_PROF_FINALIZE);
  return finalize_output(ctx, y, ldy, 0, rows, m->num_pdfs, m->final_log_softmax,
                         subtract_prior ? m->log_prior.as<float>() : nullptr, d_dst, d_out, tail);
}

static int score_feats(ce_gpu_ctx *ctx, const ce_gpu_model *m, const ce_gpu_plan *p, const float *d_global_stats,
                       float *d_feats_ws, float *d_loglik) {
  const float *feats = d_feats_ws;
  if (d_global_stats) {
    float *norm = d_feats_ws + (size_t)p->total_frames * kMel;
    CE_TRY(ce_gpu_cmvn(ctx, p, d_global_stats, d_feats_ws, norm));
    feats = norm;
  }
  return ce_gpu_am_forward(ctx, m, p, feats, d_loglik);
}

int ce_gpu_score(ce_gpu_ctx *ctx, const ce_gpu_model *m, const ce_gpu_plan *p, const float *d_pcm,
                 const float *d_global_stats, float *d_feats_ws, float *d_loglik) {
  if (!ctx || !m || !p) return fail(CE_GPU_EINVAL, "NULL argument");
  if (m->input_dim != kMel) return fail(CE_GPU_EINVAL, "nnet input is not 40-dim fbank");
  CE_TRY(ce_gpu_fbank(ctx, p, d_pcm, d_feats_ws, nullptr));
  return score_feats(ctx, m, p, d_global_stats, d_feats_ws, d_loglik);
}

int ce_gpu_score_s16(ce_gpu_ctx *ctx, const ce_gpu_model *m, const ce_gpu_plan *p, const int16_t *d_pcm,
                     const float *d_global_stats, float *d_feats_ws, float *d_loglik) {
  if (!ctx || !m || !p) return fail(CE_GPU_EINVAL, "NULL argument");
  if (m->input_dim != kMel) return fail(CE_GPU_EINVAL, "nnet input is not 40-dim fbank");
  CE_TRY(ce_gpu_fbank_s16(ctx, p, d_pcm, d_feats_ws, nullptr));
  return score_feats(ctx, m, p, d_global_stats, d_feats_ws, d_loglik);
}

int ce_gpu_sgemm(ce_gpu_ctx *ctx, int m, int n, int k, const float *d_a, int lda, const float *d_b, int ldb,
                 float *d_c, int ldc) {
  if (!ctx || m < 0 || n < 0 || k < 0) return fail(CE_GPU_EINVAL, "bad argument");
  if (m == 0 || n == 0) return CE_GPU_OK;
  if (k == 0) {
    for (int i = 0; i < m; ++i) CE_HIP(hipMemsetAsync(d_c + (size_t)i * ldc, 0, sizeof(float) * n, ctx->stream));
    return CE_GPU_OK;
  }
  if (lda < k || ldb < n || ldc < n) return fail(CE_GPU_EINVAL, "leading dimension too small");
  GemmArgs a;
  a.x = d_a;
  a.ldx = lda;
  a.m = m;
  a.n = n;
  a.k = k;
  a.kpad = (int)round_up(k, gemm_k_align());
  a.din = k;
  a.nseg = 1;
  a.w = d_b;
  a.ldw = ldb;
  a.b_nmajor = true;
  a.y = d_c;
  a.ldy = ldc;
  return launch_gemm_f32(ctx->stream, a);
}

int ce_gpu_quantize(ce_gpu_ctx *ctx, const float *d_x, int64_t count, uint8_t *d_q, void *d_params) {
  if (!ctx || !d_x || !d_q || !d_params) return fail(CE_GPU_EINVAL, "NULL argument");
  CE_TRY(ensure_scratch(ctx, 1024 * 8));
  return launch_quantize(ctx->stream, d_x, count, d_q, d_params, ctx->scratch.ptr);
}

static int gemm_u8(ce_gpu_ctx *ctx, int m, int n, int k, const uint8_t *d_a, const void *d_pa,
                   const uint8_t *d_b, const void *d_pb, float *d_cf, int32_t *d_ci) {
  if (!ctx || !d_a || !d_pa || !d_b || !d_pb || (!d_cf && !d_ci)) return fail(CE_GPU_EINVAL, "NULL argument");
  if (m <= 0 || n <= 0 || k <= 0) return fail(CE_GPU_EINVAL, "gemm_u8: empty operand (reference asserts)");
  CE_TRY(ensure_scratch(ctx, gemm_u8_scratch_bytes(m, n, k)));
  return launch_gemm_u8_ws(ctx->stream, m, n, k, d_a, d_pa, d_b, d_pb, d_cf, d_ci, ctx->scratch.ptr);
}

int ce_gpu_gemm_u8u8f32(ce_gpu_ctx *ctx, int m, int n, int k, const uint8_t *d_a, const void *d_params_a,
                        const uint8_t *d_b, const void *d_params_b, float *d_c) {
  return gemm_u8(ctx, m, n, k, d_a, d_params_a, d_b, d_params_b, d_c, nullptr);
}

int ce_gpu_gemm_u8u8i32(ce_gpu_ctx *ctx, int m, int n, int k, const uint8_t *d_a, const void *d_params_a,
                        const uint8_t *d_b, const void *d_params_b, int32_t *d_c) {
  return gemm_u8(ctx, m, n, k, d_a, d_params_a, d_b, d_params_b, nullptr, d_c);
}

static_assert(kRowRelu == CE_GPU_ROW_RELU && kRowBatchNorm == CE_GPU_ROW_BATCHNORM &&
                  kRowLogSoftmax == CE_GPU_ROW_LOGSOFTMAX && kRowSoftmax == CE_GPU_ROW_SOFTMAX &&
                  kRowNormalize == CE_GPU_ROW_NORMALIZE,
              "row-op numbering");

int ce_gpu_linear(ce_gpu_ctx *ctx, int rows, int in_dim, int out_dim, const float *d_in, int ld_in,
                  const float *d_w, int ld_w, const float *d_b, float *d_out, int ld_out) {
  if (!ctx || rows < 0 || in_dim < 0 || out_dim < 0) return fail(CE_GPU_EINVAL, "bad argument");
  if (rows == 0 || out_dim == 0) return CE_GPU_OK;
  if (!d_in || !d_w || !d_out) return fail(CE_GPU_EINVAL, "NULL argument");
  if (in_dim == 0) return fail(CE_GPU_EINVAL, "linear: empty input");
  if (ld_in < in_dim || ld_w < out_dim || ld_out < out_dim) return fail(CE_GPU_EINVAL, "leading dimension too small");
  GemmArgs a;
  a.x = d_in;
  a.ldx = ld_in;
  a.m = rows;
  a.n = out_dim;
  a.k = in_dim;
  a.kpad = (int)round_up(in_dim, gemm_k_align());
  a.din = in_dim;
  a.nseg = 1;
  a.w = d_w;
  a.ldw = ld_w;
  a.b_nmajor = true;
  a.bias = d_b;
  a.y = d_out;
  a.ldy = ld_out;
  ProfScope prof(ctx, CE_GPU_PROF_GEMM_GATHER);
  return launch_gemm_f32(ctx->stream, a);
}

int ce_gpu_splice(ce_gpu_ctx *ctx, int rows, int dim, const float *d_in, int ld_in, const int32_t *h_idx,
                  int n_idx, float *d_out) {
  if (!ctx || rows < 0 || dim < 0 || n_idx < 1 || n_idx > CE_GPU_MAX_SPLICE || !h_idx)
    return fail(CE_GPU_EINVAL, "bad argument");
  if (rows == 0 || dim == 0) return CE_GPU_OK;
  if (!d_in || !d_out || ld_in < dim) return fail(CE_GPU_EINVAL, "bad operand");
  return launch_splice(ctx->stream, rows, dim, d_in, ld_in, h_idx, n_idx, d_out);
}

int ce_gpu_rowwise(ce_gpu_ctx *ctx, int op, int rows, int dim, float *d_x, int ld, const float *d_scale,
                   const float *d_offset) {
  if (!ctx || rows < 0 || dim < 0 || ld < dim) return fail(CE_GPU_EINVAL, "bad argument");
  if (op < CE_GPU_ROW_RELU || op > CE_GPU_ROW_NORMALIZE) return fail(CE_GPU_EINVAL, "unknown row op");
  if (op == CE_GPU_ROW_BATCHNORM && (!d_scale || !d_offset)) return fail(CE_GPU_EINVAL, "BatchNorm needs scale/offset");
  if (rows == 0 || dim == 0) return CE_GPU_OK;
  if (!d_x) return fail(CE_GPU_EINVAL, "NULL argument");
  return launch_rowop_raw(ctx->stream, op, dim, d_scale, d_offset, d_x, ld, rows);
}

int ce_gpu_loglik_gather(ce_gpu_ctx *ctx, const float *d_loglik, int rows, int ld, int dim,
                         const int32_t *d_tid2pdf, int n_tid, const int32_t *d_row, const int32_t *d_trans, int n,
                         float am_scale, float *d_out) {
  if (!ctx || rows < 0 || dim < 0 || ld < dim || n_tid < 0 || n < 0) return fail(CE_GPU_EINVAL, "bad argument");
  if (n == 0) return CE_GPU_OK;
  if (!d_loglik || !d_tid2pdf || !d_row || !d_trans || !d_out) return fail(CE_GPU_EINVAL, "NULL argument");
  CE_HIP(hipSetDevice(ctx->device));
  return launch_loglik_gather(ctx->stream, d_loglik, rows, ld, dim, d_tid2pdf, n_tid, d_row, d_trans, n, am_scale, d_out);
}

int ce_gpu_loglik_columns(ce_gpu_ctx *ctx, const float *d_loglik, int rows, int ld, int dim,
                          const int32_t *d_cols, int n_cols, float *d_out) {
  if (!ctx || rows < 0 || dim < 0 || ld < dim || n_cols < 0) return fail(CE_GPU_EINVAL, "bad argument");
  if (rows == 0 || n_cols == 0) return CE_GPU_OK;
  if (!d_loglik || !d_cols || !d_out) return fail(CE_GPU_EINVAL, "NULL argument");
  CE_HIP(hipSetDevice(ctx->device));
  return launch_loglik_columns(ctx->stream, d_loglik, rows, ld, dim, d_cols, n_cols, d_out);
}

int ce_gpu_sum_f64(void *stream, const float *d_x, int64_t n, double *d_part, double *d_acc) {
  return ce_gpu_sum_f64_many(stream, 1, &d_x, &n, d_part, d_acc);
}

int ce_gpu_sum_f64_many(void *stream, int count, const float *const *d_x, const int64_t *n, double *d_part,
                        double *d_acc) {
  if (count < 0 || count > CE_GPU_SUM_MAX_BUFS || (count > 0 && (!d_x || !n)))
    return fail(CE_GPU_EINVAL, "sum_f64: bad buffer list");
  bool any = false;
  for (int k = 0; k < count; ++k) {
    if (n[k] < 0) return fail(CE_GPU_EINVAL, "bad argument");
    if (n[k] > 0 && !d_x[k]) return fail(CE_GPU_EINVAL, "NULL argument");
    any = any || n[k] > 0;
  }
  if (!any) return CE_GPU_OK;
  if (!d_part || !d_acc) return fail(CE_GPU_EINVAL, "NULL argument");
  return launch_sum_f64(reinterpret_cast<hipStream_t>(stream), count, d_x, n, d_part, d_acc);
}

int ce_gpu_debug_rowop_chain(ce_gpu_ctx *ctx, int n_ops, const int *h_ops, int rows, int dim, float *d_x, int ld,
                             const float *const *h_scale, const float *const *h_offset, uint16_t *d_out16, int ld16,
                             int width16) {
  if (!ctx || n_ops < 0 || n_ops > kRowChainMax || (n_ops > 0 && !h_ops) || rows < 0 || dim < 0)
    return fail(CE_GPU_EINVAL, "bad argument");
  if (rows == 0 || dim == 0) return CE_GPU_OK;
  if (!d_x) return fail(CE_GPU_EINVAL, "NULL argument");
  RowChain ch;
  ch.n = n_ops;
  ch.dim = dim;
  for (int q = 0; q < n_ops; ++q) {
    ch.kind[q] = h_ops[q];
    ch.scale[q] = h_scale ? h_scale[q] : nullptr;
    ch.offset[q] = h_offset ? h_offset[q] : nullptr;
  }
  return launch_rowop_chain(ctx->stream, ch, d_x, ld, rows, d_out16, ld16, width16);
}

int ce_gpu_debug_rowop_chain_q(ce_gpu_ctx *ctx, int n_ops, const int *h_ops, int rows, int dim, float *d_x, int ld,
                               const float *const *h_scale, const float *const *h_offset, float scale,
                               int32_t zero_point, int8_t *d_q, int ldq, int32_t *d_rowsum, int32_t *d_zero) {
  if (!ctx || n_ops < 0 || n_ops > kRowChainMax || (n_ops > 0 && !h_ops) || rows < 0 || dim <= 0 || ld < dim ||
      ldq < dim)
    return fail(CE_GPU_EINVAL, "bad argument");
  if (!d_x || !d_q || !d_rowsum || !d_zero) return fail(CE_GPU_EINVAL, "NULL argument");
  if (rows == 0) return CE_GPU_OK;
  CE_HIP(hipSetDevice(ctx->device));
  // the parameters as the kernel reads a layer's: a QP in device memory,
  // written in stream order (an earlier call's launch has read its own)
  if (!ctx->debug_qp.ptr) CE_TRY(ctx->debug_qp.alloc(256));
  uint32_t scale_bits;
  memcpy(&scale_bits, &scale, 4);
  CE_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ctx->debug_qp.ptr), (int)scale_bits, 1, ctx->stream));
  CE_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(static_cast<char *>(ctx->debug_qp.ptr) + 4), zero_point, 1,
                           ctx->stream));
  RowChain ch;
  ch.n = n_ops;
  ch.dim = dim;
  for (int q = 0; q < n_ops; ++q) {
    ch.kind[q] = h_ops[q];
    ch.scale[q] = h_scale ? h_scale[q] : nullptr;
    ch.offset[q] = h_offset ? h_offset[q] : nullptr;
  }
  return launch_rowop_chain_q(ctx->stream, ch, d_x, ld, rows, dim, d_q, ldq, ctx->debug_qp.ptr, d_rowsum, d_zero);
}

int ce_gpu_debug_i8_static_launches(int64_t *quantize_passes, int64_t *row_launches, int64_t *row_launches_q) {
  i8_static_launch_counts(quantize_passes, row_launches, row_launches_q);
  return CE_GPU_OK;
}

int ce_gpu_debug_fill_allocs(int on, uint32_t word) {
  g_fill_word.store(word, std::memory_order_relaxed);
  g_fill_allocs.store(on ? 1 : 0, std::memory_order_relaxed);
  return CE_GPU_OK;
}

int ce_gpu_debug_fill_ctx(ce_gpu_ctx *ctx, uint32_t word, int64_t *bytes) {
  if (!ctx) return fail(CE_GPU_EINVAL, "ctx is NULL");
  CE_HIP(hipSetDevice(ctx->device));
  int64_t total = 0;
  // every buffer a call writes before it reads (the header names them and
  // the three it leaves alone: d_tables, overflow, lat_tickets)
  for (const DevBuf *b : {&ctx->workspace, &ctx->scratch, &ctx->lat_part, &ctx->blk_maps, &ctx->debug_qp})
    CE_TRY(debug_fill(ctx->stream, b->ptr, b->bytes, word, &total));
  if (bytes) *bytes = total;
  return CE_GPU_OK;
}

}  // extern "C"
