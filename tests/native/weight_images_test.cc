// weight_images_test.cc -- the weight images' host arithmetic
// (catears_amd/csrc/weight_images.cc alone, no HIP) under AddressSanitizer /
// UndefinedBehaviorSanitizer (make sanitize), checked against the number
// formats' definitions and the layouts the kernel headers document, not
// against a copy of the loops.  Ends with a non-zero status at the first
// failed check, naming it.
//
//   weight_images_asan
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "weight_images.h"

using namespace catears;

#define CHECK(cond, ...)                                        \
  do {                                                          \
    if (!(cond)) {                                              \
      printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond);  \
      printf(__VA_ARGS__);                                      \
      printf("\n");                                             \
      exit(1);                                                  \
    }                                                           \
  } while (0)

static float from_bits(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static uint32_t bits_of(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

static uint32_t g_seed = 20240611u;
static uint32_t next() { return g_seed = g_seed * 1664525u + 1013904223u; }
// uniform in [-1, 1]
static float next_unit() { return (float)((double)(next() >> 8) / 8388607.5 - 1.0); }

static bool bf16_is_nan(uint32_t p) { return (p & 0x7fffu) > 0x7f80u; }
static bool bf16_is_finite(uint32_t p) { return (p & 0x7f80u) != 0x7f80u; }

// bf16 is the upper half of an fp32: every bf16 value converts to itself, a
// midpoint goes to the neighbour with an even pattern, anything else to the
// nearer one.
static void test_bf16() {
  for (uint32_t p = 0; p < 65536; ++p) {
    if (bf16_is_nan(p)) continue;
    CHECK(bits_of(bf16_float((uint16_t)p)) == p << 16, "bf16_float(%04x)", p);
    CHECK(bf16_rne(bf16_float((uint16_t)p)) == p, "round trip of %04x", p);
  }
  for (uint32_t p = 0; p < 65536; ++p) {
    // p and p + 1: neighbours of one sign, p + 1 the larger in magnitude
    if (!bf16_is_finite(p) || !bf16_is_finite(p + 1)) continue;
    const uint32_t mid = p << 16 | 0x8000u, even = p & 1u ? p + 1 : p;
    CHECK(bf16_rne(from_bits(mid)) == even, "midpoint %08x -> %04x", mid, bf16_rne(from_bits(mid)));
    CHECK(bf16_rne(from_bits(mid + 1)) == p + 1, "above the midpoint %08x", mid + 1);
    CHECK(bf16_rne(from_bits(mid - 1)) == p, "below the midpoint %08x", mid - 1);
  }
  CHECK(bf16_rne(from_bits(0x7f800000u)) == 0x7f80u, "+inf");
  CHECK(bf16_rne(from_bits(0xff800000u)) == 0xff80u, "-inf");
  for (uint32_t hi = 0; hi < 65536; ++hi)
    for (uint32_t lo : {0x0001u, 0x7fffu, 0x8000u, 0xffffu, 0x0000u}) {
      const uint32_t u = hi << 16 | lo;
      if ((u & 0x7fffffffu) <= 0x7f800000u) continue;  // not a NaN
      const uint16_t h = bf16_rne(from_bits(u));
      CHECK(bf16_is_nan(h) && (h & 0x8000u) == (u >> 16 & 0x8000u), "NaN %08x -> %04x", u, h);
    }
  printf("bf16 conversions ok\n");
}

static bool f16_is_nan(uint32_t h) { return (h & 0x7fffu) > 0x7c00u; }

static void test_f16() {
  for (uint32_t h = 0; h < 65536; ++h) {
    if (f16_is_nan(h)) continue;
    // the value by the format's definition: (-1)^s 2^(e-15) 1.m, subnormal 2^-14 0.m
    const int e = h >> 10 & 31, m = h & 0x3ff;
    if (e != 31) {
      const double want = (h & 0x8000u ? -1.0 : 1.0) * (e ? ldexp(1024.0 + m, e - 25) : ldexp((double)m, -24));
      CHECK((double)f16_float((uint16_t)h) == want, "f16_float(%04x) = %g, want %g", h, f16_float((uint16_t)h), want);
    } else {
      CHECK(isinf(f16_float((uint16_t)h)), "f16_float(%04x) is no infinity", h);
    }
    CHECK(f16_rne(f16_float((uint16_t)h)) == h, "round trip of %04x -> %04x", h, f16_rne(f16_float((uint16_t)h)));
  }
  for (uint32_t sign : {0u, 0x80000000u}) {
    const uint16_t s16 = (uint16_t)(sign >> 16);
    CHECK(f16_rne(from_bits(sign | 0x477fefffu)) == (s16 | 0x7bffu), "just below 65520 rounds to 65504");
    CHECK(f16_float(s16 | 0x7bffu) == (sign ? -65504.0f : 65504.0f), "0x7bff is 65504");
    CHECK(f16_rne(from_bits(sign | 0x477ff000u)) == (s16 | 0x7c00u), "65520 rounds to infinity");
    // the midpoint of subnormals m and m + 1 (m + 1 = 1024: the smallest normal)
    for (int m = 0; m < 1024; ++m) {
      const float mid = ldexpf((float)(2 * m + 1), -25);
      const uint16_t want = (uint16_t)(s16 | (m & 1 ? m + 1 : m));
      const uint16_t got = f16_rne(sign ? -mid : mid);
      CHECK(got == want, "subnormal midpoint %d: %04x, want %04x", m, got, want);
    }
    for (uint32_t nan : {0x7fc00000u, 0x7f800001u, 0x7fffffffu, 0x7f802000u}) {
      const uint16_t h = f16_rne(from_bits(sign | nan));
      CHECK((h & 0x7c00u) == 0x7c00u && (h & 0x200u) && (h & 0x8000u) == s16, "NaN %08x -> %04x", sign | nan, h);
    }
  }
  printf("f16 conversions ok\n");
}

// An 8 + 8 + 8 bit split of a 24-bit significand is exact: the three planes
// of the image add up to the value, in float arithmetic.
static void test_plane_split() {
  std::vector<float> v;
  for (int e : {-100, 0, 100})
    for (uint32_t sign : {0u, 0x80000000u}) {
      const uint32_t pow2 = sign | (uint32_t)(e + 127) << 23;
      v.push_back(from_bits(pow2));
      v.push_back(from_bits(pow2 - 1));  // 2^e - 1 ulp
      v.push_back(from_bits(pow2 + 1));  // 2^e + 1 ulp
    }
  while (v.size() < 100000 + 18) {
    const uint32_t e = next() % 201 + 27;  // biased exponent of 2^-100 .. 2^100
    v.push_back(from_bits((next() & 0x80000000u) | e << 23 | (next() >> 9)));
  }
  const int kpad = (int)v.size();
  const std::vector<uint16_t> img = bf16_plane_image(v, 1, kpad);
  CHECK(img.size() == 3 * v.size(), "plane image of %zu words", img.size());
  for (int k = 0; k < kpad; ++k) {
    const float h = bf16_float(img[k]), m = bf16_float(img[kpad + k]), lo = bf16_float(img[2 * kpad + k]);
    CHECK(img[k] == bf16_rne(v[k]), "plane 0 of %08x is not its bf16", bits_of(v[k]));
    CHECK(h + m + lo == v[k], "%08x: planes %04x %04x %04x add up to %08x", bits_of(v[k]), img[k], img[kpad + k],
          img[2 * kpad + k], bits_of(h + m + lo));
  }
  printf("bf16 plane split exact on %d values\n", kpad);
}

// The fragment image is the plane image permuted (X6Gemm::wd, internal.h;
// kernels/gemm_bf16.hip's head comment): for 16-unit block u, K-tile t (32 k)
// and plane p the 512 words at ((u * kt + t) * 3 + p) * 512 hold lane l's 8
// words (unit 16 u + (l & 15), k = 32 t + 8 (l >> 4) ..+7) at 8 l; units
// zero-padded to a multiple of kX6DirUnits.
static void test_fragment_image() {
  for (int n : {1, 15, 16, 17, 255, 256, 257})
    for (int kpad : {32, 64, 96}) {
      std::vector<float> wt((size_t)n * kpad);
      for (size_t i = 0; i < wt.size(); ++i)  // distinct, and low significand bits set: three different planes
        wt[i] = from_bits(bits_of((float)(i + 1)) | 0x100u | ((uint32_t)i * 2654435761u >> 24) | 1u);
      const std::vector<uint16_t> planes = bf16_plane_image(wt, n, kpad), img = bf16_fragment_image(wt, n, kpad);
      CHECK(planes.size() == (size_t)n * 3 * kpad, "n %d kpad %d: plane image of %zu words", n, kpad, planes.size());
      CHECK(img.size() == round_up(n, 256) * 3 * kpad, "n %d kpad %d: fragment image of %zu words", n, kpad,
            img.size());
      std::vector<char> addressed(img.size(), 0);
      const int kt = kpad / 32;
      for (int j = 0; j < n; ++j)
        for (int k = 0; k < kpad; ++k)
          for (int p = 0; p < 3; ++p) {
            const int u = j / 16, t = k / 32, l = j % 16 + 16 * (k % 32 / 8), e = k % 8;
            const size_t at = (((size_t)u * kt + t) * 3 + p) * 512 + 8 * (size_t)l + e;
            CHECK(at < img.size() && !addressed[at], "n %d kpad %d: address %zu of (%d, %d, %d)", n, kpad, at, j, k, p);
            addressed[at] = 1;
            const uint16_t want = planes[(size_t)j * 3 * kpad + (size_t)p * kpad + k];
            CHECK(img[at] == want, "n %d kpad %d: (%d, %d) plane %d is %04x, want %04x", n, kpad, j, k, p, img[at],
                  want);
          }
      for (size_t i = 0; i < img.size(); ++i)
        CHECK(addressed[i] || img[i] == 0, "n %d kpad %d: padding word %zu is %04x", n, kpad, i, img[i]);
    }
  printf("fragment image ok\n");
}

// Two scaled fp16 planes: max |u| in [2^14, 2^15), u = hi + lo / 2^11 up to
// the second plane's own rounding (2^-11 relative of a remainder of at most
// 2^-11 |u|, or half a subnormal step 2^-25 of the scaled remainder).
static void test_f16_image() {
  const int n = 5, kpad = 64;
  std::vector<float> wt((size_t)n * kpad);
  for (float &w : wt) w = 0.75f * next_unit();
  wt[17] = -0.75f;
  std::vector<uint16_t> img;
  int shift = -1000;
  CHECK(f16_plane_image(wt, n, kpad, &img, &shift), "finite weights have an image");
  CHECK(shift == 15 && img.size() == (size_t)n * 2 * kpad, "shift %d, %zu words", shift, img.size());
  for (int j = 0; j < n; ++j)
    for (int k = 0; k < kpad; ++k) {
      const double u = ldexp((double)wt[(size_t)j * kpad + k], shift);
      const uint16_t hi = img[(size_t)j * 2 * kpad + k], lo = img[(size_t)j * 2 * kpad + kpad + k];
      CHECK(fabs(u) < 32768.0 && hi == f16_rne((float)u), "(%d, %d): first plane %04x", j, k, hi);
      const double err = fabs(u - ((double)f16_float(hi) + (double)f16_float(lo) / 2048.0));
      CHECK(err <= ldexp(fabs(u), -22) + ldexp(1.0, -36), "(%d, %d): planes are %g from %g", j, k, err, u);
    }
  for (float bad : {INFINITY, -INFINITY, NAN}) {
    std::vector<float> w2 = wt;
    w2[w2.size() - 1] = bad;
    std::vector<uint16_t> none(3, 7);
    int s2 = 123;
    CHECK(!f16_plane_image(w2, n, kpad, &none, &s2), "a weight that is not finite has no image");
    CHECK(none == std::vector<uint16_t>(3, 7) && s2 == 123, "no image: outputs untouched");
  }
  printf("f16 plane image ok\n");
}

static void test_int8_image() {
  const int shapes[][2] = {{1, 1}, {3, 63}, {4, 64}, {5, 65}, {17, 200}};
  for (const auto &sh : shapes)
    for (int align : {64, 128}) {
      const int n = sh[0], k = sh[1], kpad = (int)round_up(k, 64);
      // columns k .. kpad - 1 of the fp32 matrix are no weights: a value that
      // would move the range if it were read
      std::vector<float> wt((size_t)n * kpad, 7.0f);
      float mn = FLT_MAX, mx = -FLT_MAX;
      int row_mn = 0, row_mx = 0;
      for (int j = 0; j < n; ++j)
        for (int c = 0; c < k; ++c) {
          float w = next_unit();
          if (n * k == 1) w = -0.25f;  // one weight: its max is FindMinMax's seed FLT_MIN
          wt[(size_t)j * kpad + c] = w;
          if (w < mn) mn = w, row_mn = j;
          if (w > mx) mx = w, row_mx = j;
        }
      if (mx < FLT_MIN) mx = FLT_MIN, row_mx = -1;
      CHECK(mn < mx, "n %d k %d: min and max differ", n, k);
      const Int8Image im = int8_image(wt, n, k, kpad, align);
      CHECK(im.kpad == (int)round_up(k, align), "n %d k %d align %d: kpad %d", n, k, align, im.kpad);
      CHECK(im.q.size() == (size_t)n * im.kpad && im.colsum.size() == (size_t)n, "n %d k %d: sizes", n, k);
      CHECK(im.scale == (float)((mx - mn) / 255.0), "n %d k %d: scale %g", n, k, im.scale);
      bool has_lo = false, has_hi = row_mx < 0;
      for (int j = 0; j < n; ++j) {
        int32_t sum = 0;
        for (int c = 0; c < im.kpad; ++c) {
          const int q = im.q[(size_t)j * im.kpad + c];
          CHECK(q >= -128 && q <= 127, "n %d k %d: byte %d", n, k, q);
          if (c >= k) CHECK(q == 0, "n %d k %d: padding (%d, %d) is %d", n, k, j, c, q);
          sum += q;
          if (c < k) {
            // within half a step of the weight (and 1e-3 of a step for the float evaluation)
            const double x = (double)wt[(size_t)j * kpad + c] / im.scale + im.zero_point;
            CHECK(fabs(q + 128 - x) <= 0.5 + 1e-3, "n %d k %d: (%d, %d) byte %d for %g steps", n, k, j, c, q, x);
          }
          has_lo = has_lo || (j == row_mn && q == -128);
          has_hi = has_hi || (j == row_mx && q == 127);
        }
        CHECK(im.colsum[j] == sum, "n %d k %d: colsum[%d] %d, row sum %d", n, k, j, im.colsum[j], sum);
      }
      CHECK(has_lo, "n %d k %d: no -128 in the minimum's row %d", n, k, row_mn);
      CHECK(has_hi, "n %d k %d: no 127 in the maximum's row %d", n, k, row_mx);
    }
  printf("int8 image ok\n");
}

static void test_quant_params() {
  float s = -1.0f;
  int32_t zp = -1;
  CHECK(quant_params_from_range(0.0f, 255.0f, &s, &zp) && s == 1.0f && zp == 0, "[0, 255]: %g %d", s, zp);
  CHECK(quant_params_from_range(-128.0f, 127.0f, &s, &zp) && s == 1.0f && zp == 128, "[-128, 127]: %g %d", s, zp);
  CHECK(quant_params_from_range(-2.0f, 508.0f, &s, &zp) && s == 2.0f && zp == 1, "[-2, 508]: %g %d", s, zp);
  // max below FLT_MIN counts as FLT_MIN (FindMinMax's seed)
  CHECK(quant_params_from_range(-255.0f, -1.0f, &s, &zp) && s == 1.0f && zp == 255, "[-255, -1]: %g %d", s, zp);
  s = 5.0f, zp = 5;
  CHECK(!quant_params_from_range(1.0f, 1.0f, &s, &zp) && s == 5.0f && zp == 5, "[1, 1] has no scale");
  printf("range parameters ok\n");
}

static void test_transpose() {
  const int in = 5, out = 3, kpad = 8;
  std::vector<float> w((size_t)in * out);
  for (size_t i = 0; i < w.size(); ++i) w[i] = (float)(i + 1);
  const std::vector<float> wt = transpose_padded(w, in, out, kpad);
  CHECK(wt.size() == (size_t)out * kpad, "%zu elements", wt.size());
  for (int j = 0; j < out; ++j)
    for (int k = 0; k < kpad; ++k)
      CHECK(bits_of(wt[(size_t)j * kpad + k]) == (k < in ? bits_of(w[(size_t)k * out + j]) : 0u), "(%d, %d)", j, k);
  printf("transpose ok\n");
}

static void test_relayout() {
  struct Case {
    int nseg, din, din_pad, n, n_pad;
  };
  for (const Case &c : {Case{1, 5, 5, 5, 32}, Case{3, 5, 32, 7, 32}, Case{2, 7, 32, 3, 4}}) {
    const int kpad = (int)round_up(c.nseg * c.din, 64), kpad_pad = (int)round_up(c.nseg * c.din_pad, 64);
    // what lies behind the old matrix's true columns must not travel
    std::vector<float> old((size_t)c.n * kpad, -3.0f);
    for (int j = 0; j < c.n; ++j)
      for (int k = 0; k < c.nseg * c.din; ++k) old[(size_t)j * kpad + k] = (float)(j * kpad + k + 1);
    const std::vector<float> wt = relayout_padded(old, c.n, kpad, c.nseg, c.din, c.n_pad, kpad_pad, c.din_pad);
    CHECK(wt.size() == (size_t)c.n_pad * kpad_pad, "nseg %d: %zu elements", c.nseg, wt.size());
    std::vector<char> is_true(wt.size(), 0);
    for (int j = 0; j < c.n; ++j)
      for (int s = 0; s < c.nseg; ++s)
        for (int col = 0; col < c.din; ++col) {
          const size_t at = (size_t)j * kpad_pad + (size_t)s * c.din_pad + col;
          is_true[at] = 1;
          CHECK(wt[at] == old[(size_t)j * kpad + s * c.din + col], "nseg %d: (%d, %d, %d) is %g", c.nseg, j, s, col,
                wt[at]);
        }
    for (size_t i = 0; i < wt.size(); ++i)
      CHECK(is_true[i] || bits_of(wt[i]) == 0u, "nseg %d: padding element %zu is %g", c.nseg, i, wt[i]);
    const float fills[3] = {0.0f, 1.0f, 0.0f};  // bias, BatchNorm scale, BatchNorm offset
    for (float fill : fills) {
      std::vector<float> v(c.n);
      for (int j = 0; j < c.n; ++j) v[j] = 0.5f + j;
      const std::vector<float> p = padded_vector(v, c.n_pad, fill);
      CHECK(p.size() == (size_t)c.n_pad, "nseg %d: padded vector of %zu", c.nseg, p.size());
      for (int j = 0; j < c.n_pad; ++j)
        CHECK(bits_of(p[j]) == bits_of(j < c.n ? v[j] : fill), "nseg %d fill %g: entry %d is %g", c.nseg, fill, j,
              p[j]);
    }
  }
  printf("re-layout ok\n");
}

int main() {
  CHECK(round_up(0, 4) == 0 && round_up(1, 4) == 4 && round_up(4, 4) == 4 && round_up(257, 256) == 512, "round_up");
  test_bf16();
  test_f16();
  test_plane_split();
  test_fragment_image();
  test_f16_image();
  test_int8_image();
  test_quant_params();
  test_transpose();
  test_relayout();
  printf("PASSED\n");
  return 0;
}
