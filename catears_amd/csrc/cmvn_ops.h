// cmvn_ops.h -- the online-CMVN rounding chain shared by the whole-utterance
// kernel (kernels/cmvn.hip) and the resumable one of the device-resident
// sessions (kernels/sessions.hip): one step of CMVN::GetFrame
// (src/cmvn.cc:35-110) and the per-frame-index tables it needs.
#pragma once

#include <hip/hip_runtime.h>

#include "internal.h"

namespace catears {

constexpr int kCmvnWindow = 600;  // PK_ONLINECMVN_WINDOW, src/cmvn.h:10
constexpr int kCmvnGlobal = 200;  // PK_ONLINECMVN_GLOBALFRAMES, src/cmvn.h:11

// The chain of one (utterance, dimension) runs in three regimes of t:
//   t <  599: SmoothStats adds alpha_t * [g, N_g] (count = t + 1 < 600);
//   t == 599: count = 600, neither smoothing nor window subtraction;
//   t >= 600: frame t - 600 leaves the window (no smoothing).
enum CmvnMode { kSmooth, kPlain, kWindowed };

template <int M>
__device__ __forceinline__ float cmvn_step(float &carry, float c, float o, float al, float ng, float g) {
  // ComputeStats (cmvn.cc:35-68): double temp seeded from the float carry
  double acc = (double)carry;
  acc += (double)c;
  if (M == kWindowed) acc += -1.0 * (double)o;
  carry = (float)acc;
  // SmoothStats / Apply (cmvn.cc:80-88, 91-98) are AddVec calls, whose
  // alpha == 1 branch (vector.cc:249-256) adds v instead of 1 * v: the same
  // float, so no select here
  float s = carry;
  if (M == kSmooth) s = s + al * g;
  return c + ng * s;
}

// Everything in SmoothStats/Apply except the per-dimension sums depends only
// on the frame index t (count = min(t+1, 600)) and on N_g, so it is computed
// once per block into LDS: alpha_t (the float scalar of AddVec, cmvn.cc:80-88)
// and neg_t = -(float)(1 / smoothed count) (cmvn.cc:93-97).  For t >= 599 no
// smoothing happens and the count is exactly 600.  Called by all 64 lanes of
// a one-wave block (lane d); the caller synchronizes before reading.
__device__ __forceinline__ void cmvn_fill_tables(float *s_alpha /* kCmvnWindow */, float *s_neg /* kCmvnWindow + 1 */,
                                                 float g_count, int d) {
  for (int t = d; t <= kCmvnWindow; t += 64) {
    float count = (float)(t + 1 < kCmvnWindow ? t + 1 : kCmvnWindow);
    float alpha = 0.0f;
    if ((double)count < kCmvnWindow) {  // SmoothStats (cmvn.cc:70-89)
      double from_global = kCmvnWindow - (double)count;
      if (from_global > kCmvnGlobal) from_global = kCmvnGlobal;
      alpha = (float)(from_global / (double)g_count);
      count = alpha != 1.0f ? count + alpha * g_count : count + g_count;
    }
    if (t < kCmvnWindow) s_alpha[t] = alpha;
    s_neg[t] = -(float)(1 / (double)count);  // Apply (cmvn.cc:91-98)
  }
}

}  // namespace catears
