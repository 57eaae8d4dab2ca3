// bf16_split.h -- an fp32 value as three bf16 planes, v = h + m + l: the
// exact split of the bf16x6 GEMMs (kernels/gemm_bf16x6.hip, its experiments
// and gemm_bf16x6_lat.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace catears {
namespace split {

__device__ __forceinline__ uint16_t bf16_bits(__bf16 b) { return __builtin_bit_cast(uint16_t, b); }

// v = h + m + l in bf16 (round-to-nearest-even at each step, v_cvt_pk_bf16_f32)
__device__ __forceinline__ void split3(float v, uint16_t *h, uint16_t *m, uint16_t *l) {
  const __bf16 b0 = (__bf16)v;
  const float r1 = v - (float)b0;
  const __bf16 b1 = (__bf16)r1;
  const float r2 = r1 - (float)b1;
  *h = bf16_bits(b0);
  *m = bf16_bits(b1);
  *l = bf16_bits((__bf16)r2);
}

// split3 for two values at once, packed (low half = a): one
// v_cvt_pk_bf16_f32 per plane, the bf16 -> f32 widenings as a shift / mask.
// Bit-identical to split3 on each value (the same RNE conversions and exact
// subtractions).
struct Planes2 {
  uint32_t h, m, l;
};
__device__ __forceinline__ Planes2 split3_pair(float a, float b) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  auto cvt = [](float x, float y) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){x, y}, bf16x2));
  };
  auto lo = [](uint32_t u) { return __builtin_bit_cast(float, u << 16); };
  auto hi = [](uint32_t u) { return __builtin_bit_cast(float, u & 0xffff0000u); };
  const uint32_t p0 = cvt(a, b);
  const float ra = a - lo(p0), rb = b - hi(p0);
  const uint32_t p1 = cvt(ra, rb);
  const float sa = ra - lo(p1), sb = rb - hi(p1);
  return Planes2{p0, p1, cvt(sa, sb)};
}

}  // namespace split
}  // namespace catears
