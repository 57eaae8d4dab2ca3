// cmvn.hip -- online (sliding-window) CMVN for every utterance of a batch.
//
// Replaces CMVN::GetFrame called for frames 0, 1, 2, ... (src/cmvn.cc:35-110).
// The reference carries the 41 running sums between frames as float with a
// double temporary per step (cmvn.cc:42-67), so the running sum of dimension d
// is an inherently sequential rounding chain.  The kernel therefore gives one
// lane to each (utterance, dimension) chain -- 40 lanes of one wave per
// utterance, reading one 160-byte feature row per step -- and replays the
// chain exactly: same float/double promotions, same order, no FMA (built with
// -ffp-contract=off).  The frame count is an exact small integer, so every
// lane recomputes it instead of carrying lane 40.  Output is bit-identical to
// the reference for any input.
#include <hip/hip_runtime.h>

#include "../cmvn_ops.h"
#include "../internal.h"

namespace catears {
namespace {

constexpr int kWindow = kCmvnWindow;

#ifndef CMVN_TILE
#define CMVN_TILE 48
#endif
// frames prefetched into registers per tile of the chain: 48 took the C4
// batch's CMVN from 0.098 to 0.092 ms (tools/experiments/gpu_r5j.sh)
constexpr int kTile = CMVN_TILE;

// The chain's three regimes of t (cmvn_ops.h: t < 599 smoothing, t == 599
// plain, t >= 600 windowed) are each their own loop, so no step carries a
// select, and the per-step work is the reference's arithmetic only (the
// kernel is issue-bound: one wave per utterance, a latency chain per lane).

// The per-frame-index tables (alpha_t, -1 / count_t) are computed once per
// block into LDS (cmvn_fill_tables).
__global__ __launch_bounds__(64) void cmvn_kernel(const int64_t *__restrict__ frame_off,
                                                  const float *__restrict__ gstats,
                                                  const float *__restrict__ in,
                                                  float *__restrict__ out) {
  __shared__ float s_alpha[kWindow], s_neg[kWindow + 1];
  const int u = blockIdx.x, d = threadIdx.x;
  const float g_count = gstats[kMel];
  cmvn_fill_tables(s_alpha, s_neg, g_count, d);
  __syncthreads();
  if (d >= kMel) return;
  const int64_t r0 = frame_off[u];
  const int T = (int)(frame_off[u + 1] - r0);
  if (T == 0) return;
  const float g = gstats[d];
  const float *x = in + r0 * kMel + d;
  float *y = out + r0 * kMel + d;
  const float ng600 = s_neg[kWindow];
  float carry = 0.0f;

  // Frames [t0, t1) in regime M.  Whole tiles: the next tile's rows are
  // prefetched from a base clamped into [0, t1 - kTile] (all valid rows, one
  // base + immediate offsets per tile); the last, partial tile reloads with
  // per-row clamps.
  auto phase = [&](auto MC, int t0, int t1) {
    constexpr int M = decltype(MC)::value;
    if (t0 >= t1) return;
    float c[kTile], o[kTile];
    auto load_tile = [&](int b, float *cc, float *oo) {
      const float *xc = x + (int64_t)b * kMel;
#pragma unroll
      for (int i = 0; i < kTile; ++i) cc[i] = xc[i * kMel];
      if (M == kWindowed) {
        const float *xo = x + (int64_t)max(b - kWindow, 0) * kMel;
#pragma unroll
        for (int i = 0; i < kTile; ++i) oo[i] = xo[i * kMel];
      }
    };
    int t = t0;
    if (t + kTile <= t1) load_tile(t, c, o);
    for (; t + kTile <= t1; t += kTile) {
      float cn[kTile], on[kTile];
      load_tile(max(0, min(t + kTile, t1 - kTile)), cn, on);
      float al[kTile], ng[kTile];
#pragma unroll
      for (int i = 0; i < kTile; ++i) {
        al[i] = M == kSmooth ? s_alpha[t + i] : 0.0f;
        ng[i] = M == kSmooth ? s_neg[t + i] : ng600;
      }
      float *yt = y + (int64_t)t * kMel;
#pragma unroll
      for (int i = 0; i < kTile; ++i) yt[i * kMel] = cmvn_step<M>(carry, c[i], o[i], al[i], ng[i], g);
#pragma unroll
      for (int i = 0; i < kTile; ++i) c[i] = cn[i], o[i] = on[i];
    }
    if (t < t1) {  // partial tile
#pragma unroll
      for (int i = 0; i < kTile; ++i) {
        const int tt = min(t + i, t1 - 1);
        c[i] = x[(int64_t)tt * kMel];
        o[i] = M == kWindowed ? x[(int64_t)(tt - kWindow) * kMel] : 0.0f;
      }
#pragma unroll
      for (int i = 0; i < kTile; ++i) {
        if (t + i < t1) {
          const float al = M == kSmooth ? s_alpha[t + i] : 0.0f;
          const float ng = M == kSmooth ? s_neg[t + i] : ng600;
          y[(int64_t)(t + i) * kMel] = cmvn_step<M>(carry, c[i], o[i], al, ng, g);
        }
      }
    }
  };
  phase(std::integral_constant<int, kSmooth>(), 0, min(T, kWindow - 1));
  phase(std::integral_constant<int, kPlain>(), kWindow - 1, min(T, kWindow));
  phase(std::integral_constant<int, kWindowed>(), kWindow, T);
}

}  // namespace

int launch_cmvn(hipStream_t s, const ce_gpu_plan *p, const float *gstats, const float *in,
                float *out) {
  if (p->n_utt == 0 || p->total_frames == 0) return CE_GPU_OK;
  hipLaunchKernelGGL(cmvn_kernel, dim3(p->n_utt), dim3(64), 0, s, p->d_frame_off.as<int64_t>(),
                     gstats, in, out);
  CE_HIP(hipGetLastError());
  return CE_GPU_OK;
}

}  // namespace catears
