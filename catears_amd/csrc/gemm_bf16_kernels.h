// gemm_bf16_kernels.h -- the device side that the plain bf16 GEMM's two
// translation units share: kernels/gemm_bf16.hip (the LDS-ring kernel on
// 32 x 32 and 128 x 128 tiles; the mode is defined there) and
// kernels/gemm_bf16_lat.hip (latency mode's register-ring kernel for small
// row blocks).  The kernel arguments, the bf16 pair conversion and the one
// epilogue both kernels end in, so a row's bits cannot depend on which of
// them ran.  Everything is in the unnamed namespace: each translation unit
// compiles its own instantiations.
#pragma once

#include <hip/hip_runtime.h>

#include "internal.h"

namespace catears {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct B16Args {
  const uint16_t *wd;  // weight fragment image (plane 0 is read)
  const uint16_t *x;   // activations, rows x ldx bf16
  const float *bias, *bn_scale, *bn_offset;
  float *y32;          // fp32 output (the last layer), or
  uint16_t *y16;       // bf16 output; ldy elements per row either way
  int wd_kt, ldx, ldy;
  int m, n, kpad, din;
  uint64_t off_packed;  // splice offset of segment s in signed byte s
  int post[4];
  int npost, post_mode;
  int tiles_m, tiles_n, group;
};

// two floats -> two bf16, round to nearest even (v_cvt_pk_bf16_f32), a in the low half
__device__ __forceinline__ uint32_t bf16_pair(float a, float b) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){a, b}, bf16x2));
}

// x6_epilogue's arithmetic: lane holds units n .. n+3 of frame f per fragment
// pair; + bias (an absent one adds -0), post chain in model order.  n % 4 == 0.
template <int TW, int TF, bool OUT16>
__device__ __forceinline__ void b16_epilogue(const B16Args &p, const f32x4 (&acc)[TW][TF], int nw0, int fw0, int lane) {
  with_post_mode(p.post_mode, [&](auto M) {
#pragma unroll
    for (int i = 0; i < TW; ++i) {
      const int n = nw0 + i * 16 + 4 * (lane >> 4);
      if (n >= p.n) continue;
      const f32x4 bias = p.bias ? *reinterpret_cast<const f32x4 *>(p.bias + n) : f32x4{-0.0f, -0.0f, -0.0f, -0.0f};
      const f32x4 sc = p.bn_scale ? *reinterpret_cast<const f32x4 *>(p.bn_scale + n) : f32x4{1.0f, 1.0f, 1.0f, 1.0f};
      const f32x4 of = p.bn_offset ? *reinterpret_cast<const f32x4 *>(p.bn_offset + n) : f32x4{-0.0f, -0.0f, -0.0f, -0.0f};
#pragma unroll
      for (int j = 0; j < TF; ++j) {
        const int f = fw0 + j * 16 + (lane & 15);
        if (f >= p.m) continue;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = apply_post<decltype(M)::value>(acc[i][j][e] + bias[e], sc[e], of[e], p.post, p.npost);
        if constexpr (OUT16) {
          typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
          *reinterpret_cast<u32x2 *>(p.y16 + (int64_t)f * p.ldy + n) = u32x2{bf16_pair(v[0], v[1]), bf16_pair(v[2], v[3])};
        } else {
          *reinterpret_cast<f32x4 *>(p.y32 + (int64_t)f * p.ldy + n) = v;
        }
      }
    }
  });
}

// The argument envelope of both launchers, and every field of *p but the tile
// counts.
inline int b16_fill_args(const X6Gemm &a, B16Args *out) {
  if (a.kpad <= 0 || a.kpad % 32 != 0 || a.din <= 0 || a.din % 32 != 0 || a.nseg < 1 || a.nseg > 8 ||
      a.nseg * a.din != a.kpad)
    return fail(CE_GPU_EINVAL, "gemm_bf16: bad K geometry");
  if (a.n % 4 != 0 || a.ldy % 4 != 0 || a.ldy < a.n || !(a.y32 || a.y16))
    return fail(CE_GPU_EINVAL, "gemm_bf16: output width must be a multiple of 4");
  if (!a.x || a.ldx % 8 != 0 || a.ldx < a.din || (reinterpret_cast<uintptr_t>(a.x) & 15))
    return fail(CE_GPU_EINVAL, "gemm_bf16: activations must be 16-byte aligned rows of at least din");
  if (!a.wd || a.wd_kt * 32 < a.kpad || (reinterpret_cast<uintptr_t>(a.wd) & 15))
    return fail(CE_GPU_EINVAL, "gemm_bf16: weight fragment image does not cover K");
  // the kernels form byte offsets in 32-bit signed arithmetic
  const int64_t npad = (a.n + kX6DirUnits - 1) / kX6DirUnits * kX6DirUnits;
  if ((int64_t)a.m * a.ldx * 2 >= ((int64_t)1 << 31) || npad / 16 * a.wd_kt * 3 * 1024 >= ((int64_t)1 << 31))
    return fail(CE_GPU_EINVAL, "gemm_bf16: operand beyond 2 GiB");
  if (a.npost > 4) return fail(CE_GPU_EINVAL, "gemm_bf16: too many post ops");
  B16Args p;
  p.wd = a.wd;
  p.x = a.x;
  p.bias = a.bias;
  p.bn_scale = a.bn_scale;
  p.bn_offset = a.bn_offset;
  p.y32 = a.y32;
  p.y16 = a.y16;
  p.wd_kt = a.wd_kt;
  p.ldx = a.ldx;
  p.ldy = a.ldy;
  p.m = a.m;
  p.n = a.n;
  p.kpad = a.kpad;
  p.din = a.din;
  p.off_packed = 0;
  for (int i = 0; i < a.nseg; ++i) {
    if (a.off[i] < -128 || a.off[i] > 127) return fail(CE_GPU_ENOTSUP, "gemm_bf16: splice offset beyond +-127");
    p.off_packed |= (uint64_t)(uint8_t)(int8_t)a.off[i] << (8 * i);
  }
  for (int i = 0; i < 4; ++i) p.post[i] = a.post[i];
  p.npost = a.npost;
  p.post_mode = post_mode(a.post, a.npost);
  p.tiles_m = p.tiles_n = 0;
  p.group = 2;  // column tiles per XCD tile group (tile_order.h), as bf16x6
  *out = p;
  return CE_GPU_OK;
}

}  // namespace
}  // namespace catears
