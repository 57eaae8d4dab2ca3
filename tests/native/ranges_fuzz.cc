// ranges_fuzz.cc -- the configuration key gpu_int8_ranges under
// AddressSanitizer / UndefinedBehaviorSanitizer (make sanitize; host code
// only, catears_amd/csrc/model_io.cc alone): catears::read_int8_ranges fed a
// valid VEC0 of (min, max) pairs, every truncation of it, an odd and an empty
// list, headers declaring billions of elements, and seeded random
// corruptions.  Every failure must name the ranges file; nothing may crash.
//
//   ranges_fuzz <scratch dir> [random corruptions]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "model_io.h"

using catears::Config;
using catears::read_int8_ranges;

static int g_failed = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      printf("FAILED %s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, catears::last_error()); \
      ++g_failed;                                                       \
    }                                                                   \
  } while (0)

static void put(const std::string &path, const std::vector<uint8_t> &bytes) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) abort();
  if (!bytes.empty() && fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size()) abort();
  fclose(f);
}

// Vector<float>::Write (src/vector.cc): "VEC0", section size, dim, payload
static std::vector<uint8_t> vec0(const std::vector<float> &v) {
  std::vector<uint8_t> out(12 + 4 * v.size());
  const int32_t dim = (int32_t)v.size(), size = 4 + 4 * dim;
  memcpy(&out[0], "VEC0", 4);
  memcpy(&out[4], &size, 4);
  memcpy(&out[8], &dim, 4);
  if (!v.empty()) memcpy(&out[12], v.data(), 4 * v.size());
  return out;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1], conf = dir + "/am_int8.conf", file = dir + "/ranges.vec0";
  const int randoms = argc > 2 ? atoi(argv[2]) : 2000;
  {
    const std::string text = "# test\nnnet = x.nn02\nGPU_INT8_RANGES = ranges.vec0\n";
    put(conf, std::vector<uint8_t>(text.begin(), text.end()));
  }
  Config cf;
  EXPECT(cf.read(conf) == CE_GPU_OK);
  std::vector<float> good;
  for (int i = 0; i < 7; ++i) good.push_back(-1.5f * (i + 1)), good.push_back(2.25f * (i + 1));
  const std::vector<uint8_t> image = vec0(good);

  std::vector<float> got;
  std::string path;
  put(file, image);
  EXPECT(read_int8_ranges(cf, &got, &path) == CE_GPU_OK && got == good && path == file);

  // key absent: nothing read, nothing wrong
  {
    const std::string plain = dir + "/am_plain.conf", text = "nnet = x.nn02\n";
    put(plain, std::vector<uint8_t>(text.begin(), text.end()));
    Config none;
    EXPECT(none.read(plain) == CE_GPU_OK);
    EXPECT(read_int8_ranges(none, &got, &path) == CE_GPU_OK && got.empty() && path.empty());
  }
  // file missing
  remove(file.c_str());
  EXPECT(read_int8_ranges(cf, &got, &path) != CE_GPU_OK && strstr(catears::last_error(), "ranges.vec0"));

  // every truncation fails and names the file
  for (size_t n = 0; n < image.size(); ++n) {
    put(file, std::vector<uint8_t>(image.begin(), image.begin() + n));
    const int rc = read_int8_ranges(cf, &got, &path);
    EXPECT(rc != CE_GPU_OK && strstr(catears::last_error(), "ranges.vec0"));
  }
  // one value too few, and none at all: CE_GPU_EINVAL with the file name
  for (size_t n : {good.size() - 1, (size_t)0}) {
    put(file, vec0(std::vector<float>(good.begin(), good.begin() + n)));
    const int rc = read_int8_ranges(cf, &got, &path);
    EXPECT(rc == CE_GPU_EINVAL && got.empty() && strstr(catears::last_error(), "ranges.vec0") &&
           strstr(catears::last_error(), "pairs"));
  }
  // headers declaring sections far beyond the file
  for (int32_t huge : {0x7fffffff, 0x40000000, -1, -2147483647 - 1}) {
    std::vector<uint8_t> bad = image;
    memcpy(&bad[8], &huge, 4);
    put(file, bad);
    EXPECT(read_int8_ranges(cf, &got, &path) != CE_GPU_OK);
    bad = image;
    memcpy(&bad[4], &huge, 4);
    put(file, bad);
    EXPECT(read_int8_ranges(cf, &got, &path) != CE_GPU_OK);
  }
  // seeded random corruptions: any status, but pairs whenever it is OK
  uint32_t seed = 12345;
  auto next = [&seed]() { return seed = seed * 1664525u + 1013904223u; };
  int ok = 0;
  for (int it = 0; it < randoms; ++it) {
    std::vector<uint8_t> bad = image;
    const int edits = 1 + next() % 4;
    for (int e = 0; e < edits; ++e) bad[next() % (it % 3 ? 12 : bad.size())] = (uint8_t)(next() >> 24);
    if (it % 5 == 0) bad.resize(next() % (bad.size() + 1));
    put(file, bad);
    const int rc = read_int8_ranges(cf, &got, &path);
    if (rc == CE_GPU_OK) {
      ++ok;
      EXPECT(!got.empty() && got.size() % 2 == 0);
    } else {
      EXPECT(got.empty() || rc != CE_GPU_EINVAL);
    }
  }
  printf("%d random corruptions, %d still valid files\n", randoms, ok);
  if (g_failed) {
    printf("%d checks FAILED\n", g_failed);
    return 1;
  }
  printf("PASSED\n");
  return 0;
}
