// weight_images.cc -- the weight images' host arithmetic (see
// weight_images.h).
#include "weight_images.h"

#include <float.h>
#include <string.h>

#include <algorithm>
#include <cmath>

namespace catears {

std::vector<float> transpose_padded(const std::vector<float> &w, int in, int out, int kpad) {
  std::vector<float> wt((size_t)out * kpad, 0.0f);
  for (int k = 0; k < in; ++k)
    for (int j = 0; j < out; ++j) wt[(size_t)j * kpad + k] = w[(size_t)k * out + j];
  return wt;
}

std::vector<uint16_t> bf16_plane_image(const std::vector<float> &wt, int n, int kpad) {
  std::vector<uint16_t> sp((size_t)n * 3 * kpad);
  for (int j = 0; j < n; ++j)
    for (int k = 0; k < kpad; ++k) {
      const float v = wt[(size_t)j * kpad + k];
      const uint16_t h = bf16_rne(v);
      const float r1 = v - bf16_float(h);
      const uint16_t m = bf16_rne(r1);
      const float r2 = r1 - bf16_float(m);
      uint16_t *row = sp.data() + (size_t)j * 3 * kpad;
      row[k] = h;
      row[kpad + k] = m;
      row[2 * kpad + k] = bf16_rne(r2);
    }
  return sp;
}

std::vector<uint16_t> bf16_fragment_image(const std::vector<float> &wt, int n, int kpad) {
  const int npad = (int)round_up(n, kX6DirUnits), kt = kpad / 32;
  std::vector<uint16_t> img((size_t)npad * 3 * kpad, 0);
  for (int ub = 0; ub < npad / 16; ++ub)
    for (int t = 0; t < kt; ++t)
      for (int l = 0; l < 64; ++l) {
        const int j = ub * 16 + (l & 15), k0 = t * 32 + (l >> 4) * 8;
        if (j >= n) continue;
        for (int e = 0; e < 8; ++e) {
          const float v = wt[(size_t)j * kpad + k0 + e];
          const uint16_t h = bf16_rne(v);
          const float r1 = v - bf16_float(h);
          const uint16_t m = bf16_rne(r1);
          const uint16_t lo = bf16_rne(r1 - bf16_float(m));
          const size_t base = (((size_t)ub * kt + t) * 3) * 512 + (size_t)l * 8 + e;
          img[base] = h;
          img[base + 512] = m;
          img[base + 1024] = lo;
        }
      }
  return img;
}

bool f16_plane_image(const std::vector<float> &wt, int n, int kpad, std::vector<uint16_t> *img, int *shift) {
  float mx = 0.0f;
  for (float v : wt) {
    if (!std::isfinite(v)) return false;
    mx = std::max(mx, std::fabs(v));
  }
  int e = 0;
  if (mx > 0.0f) frexpf(mx, &e);  // mx in [2^(e-1), 2^e)
  *shift = std::max(-100, std::min(100, 15 - e));
  std::vector<uint16_t> sp((size_t)n * 2 * kpad);
  for (int j = 0; j < n; ++j)
    for (int k = 0; k < kpad; ++k) {
      const float u = ldexpf(wt[(size_t)j * kpad + k], *shift);
      const uint16_t h = f16_rne(u);
      uint16_t *row = sp.data() + (size_t)j * 2 * kpad;
      row[k] = h;
      row[kpad + k] = f16_rne((u - f16_float(h)) * 2048.0f);
    }
  img->swap(sp);
  return true;
}

Int8Image int8_image(const std::vector<float> &wt, int n, int k, int kpad, int align) {
  Int8Image im;
  float mn = FLT_MAX, mx = FLT_MIN;  // FindMinMax (matrix.cc:329-345)
  for (int j = 0; j < n; ++j)
    for (int c = 0; c < k; ++c) {
      const float v = wt[(size_t)j * kpad + c];
      if (v > mx) mx = v;
      if (v < mn) mn = v;
    }
  const double scale = (mx - mn) / 255.0;  // ComputeQuantizationParams (matrix.cc:348-362)
  im.zero_point = (int32_t)round(-mn / scale);
  im.scale = (float)scale;
  im.kpad = (int)round_up(k, align);
  // locals in the loop: a byte store may alias any member of *im
  const float w_scale = im.scale;
  const int32_t w_zp = im.zero_point;
  const int kpad_i8 = im.kpad;
  std::vector<int8_t> q((size_t)n * kpad_i8, 0);
  std::vector<int32_t> colsum(n, 0);
  for (int j = 0; j < n; ++j)
    for (int c = 0; c < k; ++c) {
      float v = wt[(size_t)j * kpad + c] / w_scale + w_zp;  // matrix.cc:378-386
      v = std::max(0.0f, std::min(v, 255.0f));
      const int b = (int)(uint8_t)roundf(v) - 128;
      q[(size_t)j * kpad_i8 + c] = (int8_t)b;
      colsum[j] += b;
    }
  im.q.swap(q);
  im.colsum.swap(colsum);
  return im;
}

bool quant_params_from_range(float min, float max, float *scale, int32_t *zero_point) {
  if (max < FLT_MIN) max = FLT_MIN;  // FindMinMax seeds max with FLT_MIN (matrix.cc:331-345)
  const float width = max - min;     // float, as the reference subtracts
  const double s = width / 255.0;    // ComputeQuantizationParams (matrix.cc:348-362)
  if (!(s > 0.0) || !std::isfinite(s) || !((float)s > 0.0f)) return false;
  *zero_point = (int32_t)round(-min / s);
  *scale = (float)s;
  return true;
}

std::vector<float> relayout_padded(const std::vector<float> &wt, int n, int kpad, int nseg, int din, int n_pad,
                                   int kpad_pad, int din_pad) {
  std::vector<float> out((size_t)n_pad * kpad_pad, 0.0f);
  for (int j = 0; j < n; ++j)
    for (int s = 0; s < nseg; ++s)
      memcpy(&out[(size_t)j * kpad_pad + (size_t)s * din_pad], &wt[(size_t)j * kpad + (size_t)s * din],
             (size_t)din * 4);
  return out;
}

std::vector<float> padded_vector(const std::vector<float> &v, int n_pad, float fill) {
  std::vector<float> out(n_pad, fill);
  std::copy(v.begin(), v.end(), out.begin());
  return out;
}

}  // namespace catears
