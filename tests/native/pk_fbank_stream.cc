// pk_fbank_stream.cc -- the drop-in Fbank::Process and CMVN with the
// library's allocation counters (ce_gpu_debug_counters) read around the
// calls: tests/test_gpu_dropin_plans.py checks that a lane's reusable plan
// leaves the counters alone once it is warm and moves them by one growth
// when a call exceeds its capacity.
//
//   pk_fbank_stream fbank <pcm.f32> <chunk> <pieces> <out.f32>
//     streams the first `pieces` pieces of `chunk` samples (pieces = 0: the
//     whole file, the last piece short) through one Fbank::Instance;
//   pk_fbank_stream cmvn <feats.f32> <rows_a> <rows_b> <stats.vec0> <out_a.f32> <out_b.f32>
//     constructs CMVN over the first rows_a rows, then over the first rows_b.
//   pk_fbank_stream time <pcm.f32> <chunk> <pieces> <am.conf> <am_threads>
//     (tools/latency.py --fbank-stream) the host time of every Fbank::Process
//     call but the first over `pieces` pieces, alone (am_threads = 0) or
//     beside am_threads threads that each stream frames through
//     AcousticModel::Process on lanes of their own; one JSON line.
//
// stdout, one line each, "<label> <device allocations> <device releases>":
//   start   the runtime exists (lane 0 and its plan), nothing was called;
//   first   after the first call;
//   last    after the last call.
// An output file starts with two int32: rows, cols.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "am.h"
#include "catears_gpu.h"
#include "configuration.h"
#include "catears_runtime.h"
#include "cmvn.h"
#include "fbank.h"
#include "matrix.h"
#include "util.h"
#include "vector.h"

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

static void save(const char *path, const float *data, int rows, int cols) {
  FILE *f = fopen(path, "wb");
  if (!f) exit(2);
  const int32_t hdr[2] = {rows, cols};
  fwrite(hdr, 4, 2, f);
  fwrite(data, sizeof(float), (size_t)rows * cols, f);
  fclose(f);
}

static void counters(const char *label) {
  int64_t a = 0, f = 0;
  ce_gpu_debug_counters(&a, &f);
  printf("%s %lld %lld\n", label, (long long)a, (long long)f);
}

static std::vector<float> cmvn_rows(const Vector<float> &stats, const std::vector<float> &feats, int rows) {
  Matrix<float> raw;
  raw.Resize(rows, 40, Matrix<float>::kUndefined);
  for (int r = 0; r < rows; ++r) memcpy(raw.Row(r).Data(), &feats[(size_t)r * 40], sizeof(float) * 40);
  CMVN cmvn(stats, raw);
  std::vector<float> out((size_t)rows * 40);
  for (int t = 0; t < rows; ++t) {
    SubVector<float> row(&out[(size_t)t * 40], 40);
    cmvn.GetFrame(t, &row);
  }
  return out;
}

static int run(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "fbank" && argc == 6) {
    const std::vector<float> pcm = load(argv[2]);
    const size_t chunk = (size_t)atoi(argv[3]);
    const int pieces = atoi(argv[4]);
    if (chunk == 0) return 1;
    const size_t end = pieces > 0 ? std::min(pcm.size(), chunk * (size_t)pieces) : pcm.size();
    catears::host::Runtime::Get();
    counters("start");
    Fbank fbank;
    Fbank::Instance inst;
    std::vector<float> all;
    bool first = true;
    for (size_t at = 0; at < end; at += chunk) {
      const int n = (int)std::min(chunk, end - at);
      Vector<float> wave(n, Vector<float>::kUndefined);
      memcpy(wave.Data(), &pcm[at], sizeof(float) * n);
      Matrix<float> feats;
      fbank.Process(&inst, wave, &feats);
      for (int r = 0; r < feats.NumRows(); ++r) {
        const SubVector<float> row = feats.Row(r);
        all.insert(all.end(), row.Data(), row.Data() + row.Dim());
      }
      if (first) counters("first");
      first = false;
    }
    counters("last");
    save(argv[5], all.data(), (int)(all.size() / 40), 40);
    return 0;
  }
  if (mode == "cmvn" && argc == 8) {
    const std::vector<float> feats = load(argv[2]);
    const int rows_a = atoi(argv[3]), rows_b = atoi(argv[4]);
    if (rows_a < 0 || rows_b < 0 || (size_t)std::max(rows_a, rows_b) * 40 > feats.size()) return 1;
    Vector<float> stats;
    util::ReadableFile fd;
    Status st = fd.Open(argv[5]);
    if (st.ok()) st = stats.Read(&fd);
    if (!st.ok()) {
      fprintf(stderr, "%s\n", st.what().c_str());
      return 3;
    }
    catears::host::Runtime::Get();
    counters("start");
    const std::vector<float> a = cmvn_rows(stats, feats, rows_a);
    counters("first");
    const std::vector<float> b = cmvn_rows(stats, feats, rows_b);
    counters("last");
    save(argv[6], a.data(), rows_a, 40);
    save(argv[7], b.data(), rows_b, 40);
    return 0;
  }
  if (mode == "time" && argc == 7) {
    const std::vector<float> pcm = load(argv[2]);
    const size_t chunk = (size_t)atoi(argv[3]);
    const int pieces = atoi(argv[4]), am_threads = atoi(argv[6]);
    if (chunk == 0 || pieces < 2 || am_threads < 0 || pcm.size() < chunk * (size_t)pieces) return 1;
    Configuration conf;
    AcousticModel am;
    if (am_threads > 0) {
      Status st = conf.Read(argv[5]);
      if (st.ok()) st = am.Read(conf);
      if (!st.ok()) {
        fprintf(stderr, "%s\n", st.what().c_str());
        return 3;
      }
    }
    catears::host::Runtime::Get();
    // the AM lanes: every thread feeds frames to an Instance of its own for
    // as long as the fbank stream runs
    std::atomic<bool> stop{false};
    std::atomic<int> warm{0};
    std::atomic<long long> am_batches{0};
    std::vector<std::thread> lanes;
    for (int k = 0; k < am_threads; ++k)
      lanes.emplace_back([&, k]() {
        AcousticModel::Instance inst;
        std::vector<float> f(40);
        Matrix<float> log_prob;
        bool counted = false;
        for (long long t = 0; !stop.load(std::memory_order_relaxed); ++t) {
          for (int d = 0; d < 40; ++d) f[d] = 10.0f + (float)((t * 7 + d * 13 + k) % 17) * 0.5f;
          SubVector<float> frame(f.data(), 40);
          am.Process(&inst, frame, &log_prob);
          if (log_prob.NumRows() > 0) {
            am_batches.fetch_add(1, std::memory_order_relaxed);
            if (!counted) warm.fetch_add(1), counted = true;
          }
        }
      });
    while (warm.load() < am_threads) std::this_thread::yield();
    Fbank fbank;
    Fbank::Instance inst;
    std::vector<double> us;
    int64_t a0 = 0, f0 = 0, a1 = 0, f1 = 0;
    long long frames = 0, batches0 = 0;
    for (int i = 0; i < pieces; ++i) {
      Vector<float> wave((int)chunk, Vector<float>::kUndefined);
      memcpy(wave.Data(), &pcm[(size_t)i * chunk], sizeof(float) * chunk);
      Matrix<float> feats;
      if (i == 1) {  // the first call is the warm-up
        ce_gpu_debug_counters(&a0, &f0);
        batches0 = am_batches.load();
      }
      const auto t0 = std::chrono::steady_clock::now();
      fbank.Process(&inst, wave, &feats);
      const auto t1 = std::chrono::steady_clock::now();
      if (i >= 1) us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
      frames += feats.NumRows();
    }
    const long long batches = am_batches.load() - batches0;
    ce_gpu_debug_counters(&a1, &f1);
    stop.store(true);
    for (std::thread &t : lanes) t.join();
    std::sort(us.begin(), us.end());
    auto pct = [&](double q) { return us[(size_t)(q * (us.size() - 1) + 0.5)]; };
    double sum = 0.0;
    for (double v : us) sum += v;
    printf("{\"chunk\": %zu, \"calls\": %zu, \"am_threads\": %d, \"frames\": %lld, \"p10_us\": %.1f, \"p50_us\": %.1f, "
           "\"p90_us\": %.1f, \"mean_us\": %.1f, \"am_batches_meanwhile\": %lld, \"device_allocs\": %lld, "
           "\"device_frees\": %lld}\n",
           chunk, us.size(), am_threads, frames, pct(0.1), pct(0.5), pct(0.9), sum / us.size(), batches,
           (long long)(a1 - a0), (long long)(f1 - f0));
    return 0;
  }
  fprintf(stderr, "usage: pk_fbank_stream fbank <pcm.f32> <chunk> <pieces> <out.f32>\n"
                  "       pk_fbank_stream cmvn <feats.f32> <rows_a> <rows_b> <stats.vec0> <out_a.f32> <out_b.f32>\n"
                  "       pk_fbank_stream time <pcm.f32> <chunk> <pieces> <am.conf> <am_threads>\n");
  return 1;
}

int main(int argc, char **argv) {
  try {
    return run(argc, argv);
  } catch (const catears::host::DeviceError &e) {
    fprintf(stderr, "DeviceError: %s\n", e.what());
    return 3;
  }
}
