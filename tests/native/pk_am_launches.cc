// pk_am_launches.cc -- pk_dropin's `am` mode with a report of which GEMM
// kernels the drop-in's calls took: the streaming AcousticModel path (one
// frame per Process call, EndOfStream at the end), then one line on stdout
//
//   bf16_latency_launches <n> i8_latency_launches <n>
//
// from the library's process-wide launch counters
// (ce_gpu_debug_bf16_latency_launches, ce_gpu_debug_i8_latency_launches).
// tests/test_gpu_bf16_latency.py reads it to see that gpu_latency_mode reaches
// the plain bf16 GEMMs of a gpu_gemm = bf16 model.
//
//   pk_am_launches <am.conf> <feats.f32> <rows> <out.f32>
// The output file starts with two int32: rows, cols.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "am.h"
#include "catears_gpu.h"
#include "catears_runtime.h"
#include "configuration.h"
#include "matrix.h"

using namespace pocketkaldi;

static std::vector<float> load(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<float> v(n / sizeof(float));
  if (n && fread(v.data(), 1, n, f) != (size_t)n) exit(2);
  fclose(f);
  return v;
}

static void append_rows(std::vector<float> *all, const Matrix<float> &m, int *cols) {
  for (int r = 0; r < m.NumRows(); ++r) {
    const SubVector<float> row = m.Row(r);
    all->insert(all->end(), row.Data(), row.Data() + row.Dim());
    *cols = row.Dim();
  }
}

static int run(int argc, char **argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: pk_am_launches <am.conf> <feats.f32> <rows> <out.f32>\n");
    return 1;
  }
  Configuration conf;
  Status st = conf.Read(argv[1]);
  AcousticModel am;
  if (st.ok()) st = am.Read(conf);
  if (!st.ok()) {
    fprintf(stderr, "%s\n", st.what().c_str());
    return 3;
  }
  const int rows = atoi(argv[3]);
  const std::vector<float> feats = load(argv[2]);
  const int dim = rows ? (int)(feats.size() / rows) : 0;
  int64_t b16_0 = 0, i8_0 = 0, b16_1 = 0, i8_1 = 0;
  ce_gpu_debug_bf16_latency_launches(&b16_0);
  ce_gpu_debug_i8_latency_launches(&i8_0);
  AcousticModel::Instance inst;
  std::vector<float> all;
  int cols = am.num_pdfs();
  Matrix<float> log_prob;
  for (int t = 0; t < rows; ++t) {
    SubVector<float> frame(const_cast<float *>(&feats[(size_t)t * dim]), dim);
    am.Process(&inst, frame, &log_prob);
    append_rows(&all, log_prob, &cols);
  }
  am.EndOfStream(&inst, &log_prob);
  append_rows(&all, log_prob, &cols);
  ce_gpu_debug_bf16_latency_launches(&b16_1);
  ce_gpu_debug_i8_latency_launches(&i8_1);
  FILE *f = fopen(argv[4], "wb");
  if (!f) return 2;
  const int32_t hdr[2] = {cols ? (int32_t)(all.size() / cols) : 0, cols};
  fwrite(hdr, 4, 2, f);
  fwrite(all.data(), sizeof(float), all.size(), f);
  fclose(f);
  printf("bf16_latency_launches %lld i8_latency_launches %lld\n", (long long)(b16_1 - b16_0), (long long)(i8_1 - i8_0));
  return 0;
}

int main(int argc, char **argv) {
  try {
    return run(argc, argv);
  } catch (const catears::host::DeviceError &e) {
    fprintf(stderr, "DeviceError: %s\n", e.what());
    return 3;
  }
}
