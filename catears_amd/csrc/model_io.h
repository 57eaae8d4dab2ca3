// model_io.h -- host-only model readers of libcatears_hip: the reference's
// binary sections (VEC0 / MAT0 / NN02), its key = value configuration files,
// and the thread-local error record every C-ABI entry reports through.  No
// HIP here: tests/native/parse_fuzz.cc builds this file alone under
// AddressSanitizer / UndefinedBehaviorSanitizer and feeds it truncated and
// corrupted model images.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <map>
#include <string>
#include <vector>

#include "catears_gpu.h"

namespace catears {

// Records `msg` as this thread's last error and returns `code`.
int fail(int code, const std::string &msg);
const char *last_error();
std::string fmt(const char *f, ...) __attribute__((format(printf, 1, 2)));

// Little-endian binary reader with the reference's error strings
// (src/util.cc:123-153).  Every section length read from the file is checked
// against the bytes the file still holds before anything is allocated for
// it: a corrupt header (a VEC0 dim or MAT0 shape in the billions) fails as
// the truncated file it is -- "IOError: failed to read: <file>" -- instead of
// the reference's posix_memalign abort / std::bad_alloc, which must not cross
// the C-ABI.
struct Reader {
  FILE *f = nullptr;
  std::string name;
  int64_t size = 0;  // bytes in the file or image
  ~Reader();
  int open(const std::string &path);
  // The same over an in-memory image (ce_gpu_model_load_mem).
  int open_mem(const void *buf, size_t n, const char *label);
  int64_t remaining() const;
  int read(void *dst, size_t n);
  int i32(int32_t *v) { return read(v, 4); }
  int tag(const char *expect);
  // fails with the truncated-file error unless `n` more bytes are there
  int need(int64_t n);
  // Vector<Real>::Read (src/vector.cc:267-300), Real of size 4
  template <typename T>
  int vec(std::vector<T> *out) {
    static_assert(sizeof(T) == 4, "VEC0 payloads here are 4-byte");
    int32_t dim = 0;
    int rc = vec_head(&dim);
    if (rc != CE_GPU_OK) return rc;
    out->resize(dim);
    return read(out->data(), (size_t)dim * 4);
  }
  // Matrix<float>::Read (src/matrix.cc:159-191)
  int mat(std::vector<float> *out, int *rows, int *cols);

 private:
  // "VEC0", section size, dim: checked, and the payload known to be there
  int vec_head(int32_t *dim);
};

// Configuration::Read (src/configuration.cc:14-50): key = value, '#' comments,
// keys case-insensitive, paths relative to the config file's directory.
struct Config {
  std::string file;
  std::map<std::string, std::string> kv;
  int read(const std::string &path);
  int get(const std::string &key, std::string *v) const;
  int path(const std::string &key, std::string *v) const;
  int integer(const std::string &key, int *v) const;
};

// The configuration key gpu_int8_ranges = <path> (this implementation's own;
// resolved like nnet / prior): a VEC0 of min0 max0 min1 max1 ..., the
// h_ranges of ce_gpu_model_quantize_static.  Key absent: *ranges empty, OK.
// A file that is not a non-empty list of pairs fails with CE_GPU_EINVAL and
// the file name in the message; *path receives the resolved file name.
int read_int8_ranges(const Config &cf, std::vector<float> *ranges, std::string *path);

// ce_gpu_gemm_mode_from_name: fp32, bf16x6, bf16x6p, f16x3, bf16 -> the
// CE_GPU_GEMM_* number; false for any other name (or NULL).
bool gemm_mode_from_name(const char *name, int *mode);

// The configuration key gpu_gemm = <name> (this implementation's own): the
// GEMM mode the loaded model is switched to.  Key absent: *mode = -1, OK.  A
// name gemm_mode_from_name does not know fails with CE_GPU_EINVAL and the key
// and value in the message.
int read_gpu_gemm(const Config &cf, int *mode);

// The configuration key gpu_pad_widths = 0 | 1 (this implementation's own):
// 1 re-lays the loaded model with ce_gpu_model_pad_widths before gpu_gemm is
// applied.  Key absent: *pad = 0, OK.  Any other value fails with
// CE_GPU_EINVAL and the key and value in the message; so does the value 1
// beside gpu_int8_ranges (a padded model takes no int8 form), naming both keys.
int read_gpu_pad_widths(const Config &cf, int *pad);

// The configuration key gpu_row_ops = 0 | 1 (this implementation's own): 1
// admits the loaded model's row steps to the matrix-core programs with
// ce_gpu_model_admit_row_ops, before gpu_pad_widths and gpu_gemm are applied.
// Absent: *admit = 0.  Any other value: CE_GPU_EINVAL with "gpu_row_ops =
// <value>" in the text.  Beside gpu_int8_ranges it is accepted and has no
// effect, like gpu_gemm.
int read_gpu_row_ops(const Config &cf, int *admit);

// Layer ids (src/nnet.h:21-30).
enum LayerId { kLinear = 0, kReLU = 1, kNormalize = 2, kSoftmax = 3, kSplice = 6, kBatchNorm = 7,
               kLogSoftmax = 8, kNarrow = 9 };

struct RawLayer {
  int id = -1;
  std::vector<float> w, b, scale, offset;  // linear: w is in x out
  int rows = 0, cols = 0;
  std::vector<int32_t> idx;  // splice
  int left = 0, right = 0;   // narrow
};

// Nnet::Read / ReadLayer (src/nnet.cc:221-293): the NN02 header's left /
// right context in *hl / *hr, the layers in file order.
int read_nnet(Reader &rd, std::vector<RawLayer> *layers, int *hl, int *hr);

}  // namespace catears
