// sessions.hip -- the state-carrying kernels of the device-resident sessions
// (ce_gpu_sessions_push, sessions.cc): what turns the whole-utterance
// kernels into an incremental Fbank::Process / CMVN::GetFrame
// (src/fbank.cc:265-314, src/cmvn.cc:100-119) whose state never leaves HBM.
//
//   session_stage_kernel   new samples behind each pushed slot's tail
//                          (int16 or float in, float staged: the conversion
//                          WaveReader::Process does, src/pcm_reader.cc:174);
//   session_carry_kernel   after the fbank launch, the unconsumed samples
//                          back to the front of the slot's staging region;
//   cmvn_resume_kernel     the CMVN rounding chain continued at frame t0 from
//                          the slot's carry, the window's leaving frames read
//                          from the slot's ring of raw features;
//   session_copy_kernel    without CMVN: the fbank temporary into the
//                          normalised ring;
//   session_ctx_exchange_kernel  incremental sets: a Linear's cached context
//                          rows into the lead rows of every block of a
//                          chunk, the blocks' last rows back as the new cache.
// Every kernel takes the push list (SessionPush, internal.h) the host wrote
// for this call; block index = position in that list.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../cmvn_ops.h"
#include "../internal.h"

namespace catears {
namespace {

constexpr int kStageThreads = 256;

template <typename Sample>
__global__ __launch_bounds__(kStageThreads) void session_stage_kernel(const SessionPush *__restrict__ push,
                                                                      const Sample *__restrict__ pcm,
                                                                      float *__restrict__ stage, int64_t stride) {
  const SessionPush p = push[blockIdx.y];
  const Sample *src = pcm + p.pcm_off;
  float *dst = stage + (int64_t)p.slot * stride + p.tail;
  for (int i = blockIdx.x * kStageThreads + threadIdx.x; i < p.n_new; i += gridDim.x * kStageThreads)
    dst[i] = (float)src[i];
}

// Source and destination overlap: the block reads the whole remainder (at
// most kWinLen - 1 samples once a frame was consumed, one per thread) before
// any thread writes.
constexpr int kCarryThreads = 512;
static_assert(kCarryThreads >= kWinLen - 1, "carry: one thread per remaining sample");

__global__ __launch_bounds__(kCarryThreads) void session_carry_kernel(const SessionPush *__restrict__ push,
                                                                      float *stage, int64_t stride) {
  const SessionPush p = push[blockIdx.x];
  if (p.frames == 0) return;  // nothing consumed: the tail only grew
  const int used = p.frames * kShift, rest = p.tail + p.n_new - used;
  float *base = stage + (int64_t)p.slot * stride;
  const int i = threadIdx.x;
  float v = 0.0f;
  if (i < rest) v = base[used + i];
  __syncthreads();
  if (i < rest) base[i] = v;
}

// Frames per tile of the chain: the tile's loads are issued together, ahead
// of its four dependent steps.
constexpr int kResumeTile = 4;

// One wave per pushed slot, lane d = dimension d (as cmvn_kernel).
__global__ __launch_bounds__(64) void cmvn_resume_kernel(const SessionPush *__restrict__ push,
                                                         const float *__restrict__ gstats,
                                                         const float *__restrict__ tmp, float *raw, int raw_cap,
                                                         float *__restrict__ norm, int norm_cap, float *carry_all) {
  __shared__ float s_alpha[kCmvnWindow], s_neg[kCmvnWindow + 1];
  const SessionPush p = push[blockIdx.x];
  if (p.frames == 0) return;  // uniform
  const int d = threadIdx.x;
  cmvn_fill_tables(s_alpha, s_neg, gstats[kMel], d);
  // the push's raw frames join the slot's ring first: lane d copies column d,
  // so every ring element the chain below reads was written by its own lane
  // (in this launch or an earlier one)
  float *ring = raw + (int64_t)p.slot * raw_cap * kMel;
  const float *x = tmp + (int64_t)p.tmp_row * kMel;
  if (d < kMel)
    for (int i = 0; i < p.frames; ++i) ring[(int64_t)((p.t0 + i) % raw_cap) * kMel + d] = x[(int64_t)i * kMel + d];
  __syncthreads();
  if (d >= kMel) return;
  const float g = gstats[d];
  const float ng600 = s_neg[kCmvnWindow];
  float *y = norm + (int64_t)p.slot * norm_cap * kMel + d;
  float *cp = carry_all + (int64_t)p.slot * kMel + d;
  float carry = p.t0 == 0 ? 0.0f : *cp;  // a reset slot starts a new chain
  const int t1 = p.t0 + p.frames;
  for (int t = p.t0; t < t1; t += kResumeTile) {
    float c[kResumeTile], o[kResumeTile];
#pragma unroll
    for (int i = 0; i < kResumeTile; ++i) {
      const int tt = min(t + i, t1 - 1);
      c[i] = ring[(int64_t)(tt % raw_cap) * kMel + d];
      // frame tt - 600 is still in the ring: raw_cap >= 600 + the push's frames
      o[i] = tt >= kCmvnWindow ? ring[(int64_t)((tt - kCmvnWindow) % raw_cap) * kMel + d] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < kResumeTile; ++i) {
      const int tt = t + i;
      if (tt < t1) {
        float v;
        if (tt < kCmvnWindow - 1)
          v = cmvn_step<kSmooth>(carry, c[i], o[i], s_alpha[tt], s_neg[tt], g);
        else if (tt == kCmvnWindow - 1)
          v = cmvn_step<kPlain>(carry, c[i], o[i], 0.0f, ng600, g);
        else
          v = cmvn_step<kWindowed>(carry, c[i], o[i], 0.0f, ng600, g);
        y[(int64_t)(tt % norm_cap) * kMel] = v;
      }
    }
  }
  *cp = carry;
}

__global__ __launch_bounds__(64) void session_copy_kernel(const SessionPush *__restrict__ push,
                                                          const float *__restrict__ tmp, float *__restrict__ norm,
                                                          int norm_cap) {
  const SessionPush p = push[blockIdx.y];
  const int d = threadIdx.x;
  if (d >= kMel) return;
  float *y = norm + (int64_t)p.slot * norm_cap * kMel + d;
  const float *x = tmp + (int64_t)p.tmp_row * kMel + d;
  for (int i = blockIdx.x; i < p.frames; i += gridDim.x) y[(int64_t)((p.t0 + i) % norm_cap) * kMel] = x[(int64_t)i * kMel];
}

// One thread owns one column chunk (a V: 16 bytes, or 4 where an operand is
// not 16-byte aligned) of one block (SessionBlock, internal.h) through all of
// that block's rows, so nothing it reads is written by another thread: no
// barrier, no LDS.  First the c lead rows in front of the block's new rows
// from the slot's cache (zeros for a fresh slot), then the block's last c
// rows into the cache -- with k < c some of those are lead rows the thread
// has just written, which is why the order matters and why the buffer and the
// cache are not __restrict__.  The row-sum words of a block (static int8) are
// one such column, moved by one thread with plain stores: the GEMM that
// added into them has finished.
constexpr int kXchgThreads = 256;

__device__ __forceinline__ uint4 xchg_zero(uint4 *) { return make_uint4(0u, 0u, 0u, 0u); }
__device__ __forceinline__ uint32_t xchg_zero(uint32_t *) { return 0u; }

template <typename V>
__global__ __launch_bounds__(kXchgThreads) void session_ctx_exchange_kernel(const SessionBlock *__restrict__ blocks,
                                                                            char *buf, int64_t ld_bytes, int ncol,
                                                                            int lead, int c, char *cache,
                                                                            int64_t row_cap, int32_t *rowsum,
                                                                            int32_t *sums) {
  const SessionBlock b = blocks[blockIdx.y];
  const int col = blockIdx.x * kXchgThreads + threadIdx.x;
  const int64_t first = b.row0 + lead - c;  // the first lead row this layer reads
  if (col < ncol) {
    char *x = buf + (int64_t)col * sizeof(V);
    char *cp = cache + (int64_t)b.slot * c * row_cap + (int64_t)col * sizeof(V);
    for (int j = 0; j < c; ++j) {
      V v = xchg_zero(static_cast<V *>(nullptr));
      if (!b.fresh) v = *reinterpret_cast<const V *>(cp + j * row_cap);
      *reinterpret_cast<V *>(x + (first + j) * ld_bytes) = v;
    }
    for (int j = 0; j < c; ++j)
      *reinterpret_cast<V *>(cp + j * row_cap) = *reinterpret_cast<const V *>(x + (first + b.k + j) * ld_bytes);
  }
  if (rowsum && blockIdx.x == 0 && threadIdx.x == 0) {
    int32_t *sp = sums + (int64_t)b.slot * c;
    for (int j = 0; j < c; ++j) rowsum[first + j] = b.fresh ? 0 : sp[j];
    for (int j = 0; j < c; ++j) sp[j] = rowsum[first + b.k + j];
  }
}

template <typename Sample>
int launch_stage_t(hipStream_t s, const SessionPush *d_push, int n, int max_new, const Sample *pcm, float *stage,
                   int64_t stride) {
  if (n <= 0 || max_new <= 0) return CE_GPU_OK;
  const int bx = std::min((max_new + kStageThreads - 1) / kStageThreads, 1024);
  hipLaunchKernelGGL((session_stage_kernel<Sample>), dim3(bx, n), dim3(kStageThreads), 0, s, d_push, pcm, stage,
                     stride);
  CE_HIP(hipGetLastError());
  return CE_GPU_OK;
}

}  // namespace

int launch_session_stage(hipStream_t s, const SessionPush *d_push, int n, int max_new, const float *pcm, float *stage,
                         int64_t stride) {
  return launch_stage_t(s, d_push, n, max_new, pcm, stage, stride);
}

int launch_session_stage_s16(hipStream_t s, const SessionPush *d_push, int n, int max_new, const int16_t *pcm,
                             float *stage, int64_t stride) {
  return launch_stage_t(s, d_push, n, max_new, pcm, stage, stride);
}

int launch_session_carry(hipStream_t s, const SessionPush *d_push, int n, float *stage, int64_t stride) {
  if (n <= 0) return CE_GPU_OK;
  hipLaunchKernelGGL(session_carry_kernel, dim3(n), dim3(kCarryThreads), 0, s, d_push, stage, stride);
  CE_HIP(hipGetLastError());
  return CE_GPU_OK;
}

int launch_session_cmvn(hipStream_t s, const SessionPush *d_push, int n, int total_frames, const float *gstats,
                        const float *tmp, float *raw, int raw_cap, float *norm, int norm_cap, float *carry) {
  if (n <= 0 || total_frames <= 0) return CE_GPU_OK;
  if (gstats) {
    hipLaunchKernelGGL(cmvn_resume_kernel, dim3(n), dim3(64), 0, s, d_push, gstats, tmp, raw, raw_cap, norm, norm_cap,
                       carry);
  } else {
    const int bx = std::min(total_frames, 256);
    hipLaunchKernelGGL(session_copy_kernel, dim3(bx, n), dim3(64), 0, s, d_push, tmp, norm, norm_cap);
  }
  CE_HIP(hipGetLastError());
  return CE_GPU_OK;
}

int launch_session_exchange(hipStream_t s, const IncrChunk &inc, int linear, void *buf, size_t row_bytes,
                            size_t ld_bytes, int32_t *rowsum) {
  if (linear < 0 || linear >= inc.n_layers) return fail(CE_GPU_EINVAL, "session exchange: no such layer");
  const IncrLayer &l = inc.layers[linear];
  if (l.c == 0 || inc.n_blocks == 0) return CE_GPU_OK;
  if (!buf || !l.cache || l.c > inc.lead || row_bytes == 0 || row_bytes > l.row_cap || row_bytes > ld_bytes ||
      (rowsum && !l.sums) || inc.n_blocks > 65535)
    return fail(CE_GPU_EINVAL, "session exchange: bad geometry");
  const uintptr_t mis = reinterpret_cast<uintptr_t>(buf) | reinterpret_cast<uintptr_t>(l.cache) | row_bytes |
                        ld_bytes | l.row_cap;
  if (mis & 3) return fail(CE_GPU_ENOTSUP, "session exchange: rows not 4-byte aligned");
  const bool wide = (mis & 15) == 0;
  const int ncol = (int)(row_bytes / (wide ? 16 : 4));
  const dim3 grid((ncol + kXchgThreads - 1) / kXchgThreads, inc.n_blocks), block(kXchgThreads);
  char *x = static_cast<char *>(buf);
  if (wide)
    hipLaunchKernelGGL(session_ctx_exchange_kernel<uint4>, grid, block, 0, s, inc.blocks, x, (int64_t)ld_bytes, ncol,
                       inc.lead, l.c, l.cache, (int64_t)l.row_cap, rowsum, l.sums);
  else
    hipLaunchKernelGGL(session_ctx_exchange_kernel<uint32_t>, grid, block, 0, s, inc.blocks, x, (int64_t)ld_bytes,
                       ncol, inc.lead, l.c, l.cache, (int64_t)l.row_cap, rowsum, l.sums);
  CE_HIP(hipGetLastError());
  return CE_GPU_OK;
}

}  // namespace catears
