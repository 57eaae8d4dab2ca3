// weight_images.h -- the host arithmetic behind every weight image the
// kernels read: the fp32 / bf16 / fp16 conversions, the transposed and padded
// fp32 matrix, the bf16 plane and fragment images, the scaled fp16 planes, the
// int8 image with its parameters, and ce_gpu_model_pad_widths' re-layout.
// Host vectors in, host vectors out; model.cc uploads what they return.  No
// device code and no device header here: tests/native/weight_images_test.cc
// builds weight_images.cc alone under AddressSanitizer /
// UndefinedBehaviorSanitizer (make sanitize).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

namespace catears {

// gemm_bf16x6d_kernel's unit tile: the fragment image's units are zero-padded
// to a multiple of it.
constexpr int kX6DirUnits = 256;

constexpr size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }

// The four conversions are inline: the image loops call them for every
// element, and in a -fPIC library g++ inlines no function that another
// object could replace (out of line a TDNN-S-sized model loaded in 152 ms
// instead of 110).

// fp32 -> bf16, round to nearest even (v_cvt_pk_bf16_f32; NaN stays NaN).
inline uint16_t bf16_rne(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
inline float bf16_float(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// fp32 -> fp16 bits, round to nearest even (v_cvt_f16_f32), inf beyond 65504.
inline uint16_t f16_rne(float f) {
  uint32_t x;
  memcpy(&x, &f, 4);
  const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
  const uint32_t a = x & 0x7fffffffu;
  if (a >= 0x7f800000u) return sign | 0x7c00u | (a > 0x7f800000u ? 0x200u : 0u);
  if (a >= 0x477ff000u) return sign | 0x7c00u;  // >= 65520 rounds to infinity
  if (a < 0x38800000u) {                          // below 2^-14: subnormal
    float v;
    memcpy(&v, &a, 4);
    return sign | (uint16_t)nearbyintf(v * 16777216.0f);  // units of 2^-24
  }
  const uint32_t r = a - 0x38000000u;  // rebias 127 -> 15
  return sign | (uint16_t)((r + 0xfffu + ((r >> 13) & 1u)) >> 13);
}
inline float f16_float(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
  float v;
  if (e == 0) {
    v = ldexpf((float)m, -24);
  } else if (e == 31) {
    const uint32_t u = 0x7f800000u | (m << 13);
    memcpy(&v, &u, 4);
  } else {
    const uint32_t u = ((e + 112u) << 23) | (m << 13);
    memcpy(&v, &u, 4);
  }
  uint32_t u;
  memcpy(&u, &v, 4);
  u |= sign;
  memcpy(&v, &u, 4);
  return v;
}

// A MAT0 matrix (in x out, row-major) transposed to n x kpad, K-contiguous,
// columns in .. kpad - 1 zero: GemmLayer::wt.
std::vector<float> transpose_padded(const std::vector<float> &w, int in, int out, int kpad);

// The bf16x6 GEMM's weight image: row j of the n x kpad matrix as three bf16
// planes [w0 | w1 | w2], w = w0 + w1 + w2 (the layout in kernels/gemm_bf16x6's
// head comment).
std::vector<uint16_t> bf16_plane_image(const std::vector<float> &wt, int n, int kpad);

// The direct-weight kernel's image (X6Gemm::wd): the same three planes in
// MFMA A-fragment order, round_up(n, kX6DirUnits) x 3 x kpad words, the
// padded units zero.  kpad a multiple of 32.
std::vector<uint16_t> bf16_fragment_image(const std::vector<float> &wt, int n, int kpad);

// The f16x3 GEMM's weight image (kernels/gemm_f16x3): u = w * 2^shift
// with max |u| in [2^14, 2^15), row j = [f16(u) | f16((u - f16(u)) * 2^11)].
// Returns false (no image, *img and *shift untouched) when the weights are
// not all finite.
bool f16_plane_image(const std::vector<float> &wt, int n, int kpad, std::vector<uint16_t> *img, int *shift);

// Quantize (src/matrix.cc:329-387) of one weight matrix: per-tensor
// parameters over the n x k matrix held in wt (n x kpad), then the bytes
// stored shifted (q - 128), n x round_up(k, align), zero padded, with the sum
// of each row of them.
struct Int8Image {
  float scale = 0.0f;
  int32_t zero_point = 0;
  int kpad = 0;
  std::vector<int8_t> q;
  std::vector<int32_t> colsum;
};
Int8Image int8_image(const std::vector<float> &wt, int n, int k, int kpad, int align);

// ComputeQuantizationParams (src/matrix.cc:348-362) of a finite range
// min <= max, with FindMinMax's FLT_MIN seed for max.  False (outputs
// untouched) when the range has no positive finite scale.
bool quant_params_from_range(float min, float max, float *scale, int32_t *zero_point);

// ce_gpu_model_pad_widths' re-layout of one n x kpad weight matrix of nseg
// segments of din columns onto n_pad x kpad_pad: segment s's true columns at
// s * din_pad, zero columns behind them, zero rows for the padded units.
std::vector<float> relayout_padded(const std::vector<float> &wt, int n, int kpad, int nseg, int din, int n_pad,
                                   int kpad_pad, int din_pad);

// v followed by `fill` up to n_pad entries (a padded unit's bias 0, BatchNorm
// scale 1 and offset 0).
std::vector<float> padded_vector(const std::vector<float> &v, int n_pad, float fill);

}  // namespace catears
