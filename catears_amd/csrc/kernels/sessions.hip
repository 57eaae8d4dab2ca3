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
//                          normalised ring.
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

}  // namespace catears
