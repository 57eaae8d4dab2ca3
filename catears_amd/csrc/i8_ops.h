// i8_ops.h -- the int8 output arithmetic shared by the throughput GEMM's
// epilogues (kernels/nnet_i8.hip) and the latency pair's reduce
// (kernels/nnet_i8_lat.hip): the zero-point restore, y in the reference's
// rounding order (src/matrix.cc:389-420), Quantize of one element
// (matrix.cc:378-386) and the byte / row-sum bookkeeping of a requantizing
// producer.  One definition, so the two paths cannot drift apart: their rows
// are bit-identical by construction.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.h"

namespace catears {

struct QP {
  float scale;
  int32_t zp;
};

// The corrected reciprocal product below is the default: 0 differing
// quotients from IEEE division over 68.7e9 random pairs on the GPU
// (tools/probes/qdiv_probe.hip, denormal scales included), the int8 and
// parity tests bit-exact with it, the C5 checksum unchanged, C5 +1.2 %
// (profiles/r05z21_i8_qdiv.txt).  Random pairs never sit on a rounding tie of
// a tiny scale, where the product does differ: qbyte_rscale's threshold and
// tests/test_gpu_quant_ties.py cover that.  -DCATEARS_I8_QDIV=0 builds the
// division.
#ifndef CATEARS_I8_QDIV
#define CATEARS_I8_QDIV 1
#endif

// Quantize (matrix.cc:378-386) of one element -> shifted signed byte.
// CATEARS_I8_QDIV=1: x / scale as q0 = x * r, r = 1 / scale (correctly
// rounded), corrected once, q = fma(fma(-scale, q0, x), r, q0) (Markstein's
// correction: the correctly rounded quotient when r is the correctly rounded
// reciprocal, nothing overflows and the remainder x - scale * q0 does not
// underflow: it must be exact, and below 2^-149 it cannot be); rscale == 0
// (qbyte_rscale: 1 / scale not finite, or a scale so small that the remainder
// can underflow) and non-finite results fall back to the division.
__device__ __forceinline__ int qbyte(float x, float scale, float zp, float rscale = 0.0f) {
#if CATEARS_I8_QDIV
  float q;
  if (rscale != 0.0f) {
    const float q0 = x * rscale;
    q = __builtin_fmaf(__builtin_fmaf(-scale, q0, x), rscale, q0);
    if (__builtin_isinf(q) || __builtin_isnan(q)) q = x / scale;
  } else {
    q = x / scale;
  }
  float v = q + zp;
#else
  (void)rscale;
  float v = x / scale + zp;
#endif
  v = (255.0f < v) ? 255.0f : v;  // std::min(v, 255.0f)
  v = (0.0f < v) ? v : 0.0f;      // std::max(0.0f, v)
  return (int)(uint8_t)roundf(v) - 128;
}

// qbyte's rscale for a layer's scale: 1 / scale, or 0 (the division) when
// that is not finite, the scale is below kQdivMinScale or the build divides.
//
// The threshold.  A wrong last bit of the quotient changes a byte only where
// q + zp can reach an n + 0.5 tie, so only for |q| >= 0.5; for |q| < 1/8 no
// error of the size below moves q + zp across one.  With scale in
// [2^e, 2^(e+1)), ulp(scale) = 2^(e-23), and |q0| >= 2^-3, so ulp(q0) >=
// 2^-26, the product scale * q0 is a multiple of ulp(scale) * 2^-26 =
// 2^(e-49) and x, of q0 * scale's size, of a coarser power of two: so is the
// remainder x - scale * q0, which the inner fma delivers exactly (it has at
// most 24 significant bits) as long as that unit is a float: 2^(e-49) >=
// 2^-149, e >= -100.  (For |q| >= 0.5 alone the unit is ulp(scale) * 2^-24
// and e >= -102 would do; the two binades are the margin that keeps the
// neighbours of the lowest tie, q = 0.5 at zp = 0, exact as well.)  Below
// 2^-100 the remainder is rounded to a multiple of 2^-149 and the corrected
// quotient can be off by one ulp, which moves bytes on ties: 10 of 1785 tie
// inputs of the range [0, 7.6e-37] in an exact emulation
// (tests/quantties.py, which also finds none at or above the threshold over
// its range list).  This holds with fp32 denormals kept, as these kernels
// are built; no model has such a scale, and the test is one compare per
// launch.
constexpr float kQdivMinScale = 0x1p-100f;
__device__ __forceinline__ float qbyte_rscale(float scale) {
  float rs = (CATEARS_I8_QDIV && scale >= kQdivMinScale) ? 1.0f / scale : 0.0f;
  if (__builtin_isinf(rs) || __builtin_isnan(rs)) rs = 0.0f;
  return rs;
}

// Four shifted bytes as one word, first byte lowest.
__device__ __forceinline__ uint32_t i8_pack4(int b0, int b1, int b2, int b3) {
  return (uint32_t)(uint8_t)b0 | ((uint32_t)(uint8_t)b1 << 8) | ((uint32_t)(uint8_t)b2 << 16) |
         ((uint32_t)(uint8_t)b3 << 24);
}

// Sum of the four signed bytes of a word.
__device__ __forceinline__ int byte_sum(int w) {
  const uint32_t u = (uint32_t)w;
  return ((int)(u << 24) >> 24) + ((int)(u << 16) >> 24) + ((int)(u << 8) >> 24) + (w >> 24);
}

// p.off[seg] of a GEMM's argument struct through a select chain: a runtime
// index into the kernel argument's array can force the whole argument struct
// into scratch memory (the readfirstlane keeps the compiler from turning the
// chain back into a load from a selected address)
template <class Args>
__device__ __forceinline__ int seg_off(const Args &p, int seg) {
  int v = __builtin_amdgcn_readfirstlane(p.off[0]);
#pragma unroll
  for (int i = 1; i < 8; ++i) v = seg >= i ? __builtin_amdgcn_readfirstlane(p.off[i]) : v;
  return v;
}

// Row sum of spliced row `row` of a layer input of m rows: the sum over the
// segments of the row sums of rows clamp(row + off[sg], 0, m - 1), modulo
// 2^32.  Static indices into off (a runtime index into a kernel argument's
// array can force the whole argument struct into scratch memory).
__device__ __forceinline__ uint32_t i8_spliced_rowsum(const int32_t *__restrict__ rowsum, int row, int m, int nseg,
                                                      const int (&off)[8]) {
  uint32_t sum = 0;
#pragma unroll
  for (int sg = 0; sg < 8; ++sg) {
    if (sg < nseg) {
      int src = row + off[sg];
      src = src < 0 ? 0 : (src > m - 1 ? m - 1 : src);
      sum += (uint32_t)rowsum[src];
    }
  }
  return sum;
}

// The per-launch constants of the zero-point restore
//   sum (a-zA)(b-zB) = sum a'b' + cB*rowsum(a') + cA*colsum(b') + K*cA*cB
// (cA = 128 - zA, cB = 128 - zB), all modulo 2^32 like gemmlowp's accumulator.
struct I8Restore {
  uint32_t ca, cb, kterm;
  float cscale;  // matrix.cc:404-405
};
__device__ __forceinline__ I8Restore i8_restore(const QP &pa, float w_scale, int32_t w_zp, int k) {
  I8Restore c;
  c.ca = (uint32_t)(128 - pa.zp);
  c.cb = (uint32_t)(128 - w_zp);
  c.kterm = (uint32_t)k * c.ca * c.cb;
  c.cscale = pa.scale * w_scale;
  return c;
}
// the column term: cA * colsum + K cA cB
__device__ __forceinline__ uint32_t i8_cterm(const I8Restore &c, int32_t colsum) {
  return c.ca * (uint32_t)colsum + c.kterm;
}

// One output: acc = sum a'b' (any order: exact modulo 2^32), rterm = cB *
// spliced row sum, cterm = i8_cterm; float(acc) * (sA * sB), + bias (+0 when
// absent: y is never -0 here, an int times a positive scale), then ReLU /
// BatchNorm in the reference's rounding order.
template <int MODE>
__device__ __forceinline__ float i8_output(uint32_t acc, uint32_t rterm, uint32_t cterm, float cscale, float bias,
                                           float sc, float of, const int *post, int npost) {
  const uint32_t v = acc + rterm + cterm;
  float y = (float)(int32_t)v * cscale;
  y = y + bias;
  return apply_post<MODE>(y, sc, of, post, npost);
}

// A requantizing producer's row sum: `sum` added over LANES adjacent lanes
// (a power of two; the lanes that finished bytes of one row), then one
// integer atomic by the group's first lane into the row's word -- exact in
// any order; the word is zero when the launch starts.
template <int LANES>
__device__ __forceinline__ void i8_rowsum_group_add(int sum, bool ok, int32_t *word) {
#pragma unroll
  for (int d = 1; d < LANES; d <<= 1) sum += __shfl_xor(sum, d, 64);
  if (ok && (threadIdx.x & (LANES - 1)) == 0) atomicAdd(word, sum);
}

}  // namespace catears
