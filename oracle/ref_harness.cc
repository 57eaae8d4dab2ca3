// ref_harness.cc -- TEST INFRASTRUCTURE.  A C-ABI shim over the reference's hot
// path, compiled from the reference's own sources where they lie:
//   * pocketkaldi::SRFFT        (srfft.cc)
//   * gemmlowp EightBitIntGemm  (gemmlowp/eight_bit_int_gemm/eight_bit_int_gemm.cc)
//   * Fbank, CMVN, Quantize, MatMat_U8U8F32, Nnet and AcousticModel
//     (fbank.cc, cmvn.cc, matrix.cc, nnet.cc, am.cc and what they link)
// matrix.cc includes <cblas.h> for one routine, cblas_sgemm (MatMat).  Where no
// BLAS is installed, oracle/blas_standin/cblas.h declares it and this file
// defines it (below).  The fp32 summation order of a Linear layer is therefore
// OURS: the reference does not pin one, it is whatever the linked BLAS does.
// Everything else the entries below return is the reference's own arithmetic.
// Built by oracle/Makefile into oracle/_ref/libref.so; only tests load it.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include <cblas.h>

#include "am.h"
#include "cmvn.h"
#include "configuration.h"
#include "eight_bit_int_gemm/eight_bit_int_gemm.h"
#include "fbank.h"
#include "matrix.h"
#include "nnet.h"
#include "srfft.h"
#include "vector.h"

using pocketkaldi::Matrix;
using pocketkaldi::SubVector;
using pocketkaldi::Vector;

// The one BLAS routine matrix.cc calls (MatMat, row-major, no transposes).
// c = alpha * a b + beta * c with each element summed over k = 0, 1, 2, ... in
// one float accumulator: a plain loop, the order of the oracle's orc_sgemm.
// Any other argument combination is not the reference's call: abort.
extern "C" void cblas_sgemm(enum CBLAS_ORDER order, enum CBLAS_TRANSPOSE trans_a,
                            enum CBLAS_TRANSPOSE trans_b, int m, int n, int k, float alpha, const float *a,
                            int lda, const float *b, int ldb, float beta, float *c, int ldc) {
  if (order != CblasRowMajor || trans_a != CblasNoTrans || trans_b != CblasNoTrans || alpha != 1.0f ||
      beta != 0.0f || m < 0 || n < 0 || k < 0 || lda < k || ldb < n || ldc < n)
    abort();
  for (int i = 0; i < m; ++i) {
    for (int j = 0; j < n; ++j) {
      float acc = 0.0f;
      for (int p = 0; p < k; ++p) acc += a[(long)i * lda + p] * b[(long)p * ldb + j];
      c[(long)i * ldc + j] = acc;
    }
  }
}

namespace {

// rows x cols floats into a reference Matrix (stride == cols)
void fill(Matrix<float> *m, const float *x, int rows, int cols) {
  m->Resize(rows, cols);
  for (int r = 0; r < rows; ++r) memcpy(m->Row(r).Data(), x + (long)r * cols, sizeof(float) * cols);
}

// Appends m's rows to out (row width `cols`) from row `at` on; returns the new
// row count, or -1 when they do not fit `cap` rows or have another width.
int append(const Matrix<float> &m, float *out, int at, int cap, int cols) {
  if (m.NumRows() == 0) return at;
  if (m.NumCols() != cols || at + m.NumRows() > cap) return -1;
  for (int r = 0; r < m.NumRows(); ++r)
    memcpy(out + (long)(at + r) * cols, m.Row(r).Data(), sizeof(float) * cols);
  return at + m.NumRows();
}

}  // namespace

extern "C" {

void *ref_srfft_new(int real_len) { return new pocketkaldi::SRFFT(real_len); }

void ref_srfft_free(void *f) { delete static_cast<pocketkaldi::SRFFT *>(f); }

// Forward real FFT in place (src/srfft.cc:370-459); buf holds >= real_len floats.
void ref_srfft_forward(void *f, float *data, int real_len, float *buf) {
  static_cast<pocketkaldi::SRFFT *>(f)->Compute(data, real_len, true, buf, real_len);
}

// n forward transforms back to back (timing, tools/cpu_calibrate.py)
void ref_srfft_forward_n(void *f, float *data, int n, int real_len, float *buf) {
  for (int i = 0; i < n; ++i)
    static_cast<pocketkaldi::SRFFT *>(f)->Compute(data + (long)i * real_len, real_len, true, buf, real_len);
}

// gemmlowp called with the harness's own restatement of MatMat_U8U8F32's
// argument convention (src/matrix.cc:389-420); ref_matmat_u8u8f32 below goes
// through matrix.cc itself.  Row-major A (m x k), B (k x n), C (m x n).
void ref_gemm_u8u8f32(int m, int n, int k, const uint8_t *a, float sa, int32_t zpa,
                      const uint8_t *b, float sb, int32_t zpb, float *c) {
  gemmlowp::eight_bit_int_gemm::EightBitIntGemm(
      true, true, true, m, n, k, a, -zpa, k, b, -zpb, n, c, sa * sb, n,
      gemmlowp::eight_bit_int_gemm::BitDepthSetting::A8B8);
}

// CMVN::GetFrame for frames 0 .. T-1 (src/cmvn.cc); gstats: 41 floats, feats
// and out: T x 40.
void ref_cmvn(const float *gstats, const float *feats, int T, float *out) {
  if (T <= 0) return;
  Vector<float> g(41);
  memcpy(g.Data(), gstats, sizeof(float) * 41);
  Matrix<float> raw;
  fill(&raw, feats, T, 40);
  pocketkaldi::CMVN cmvn(g, raw);
  for (int t = 0; t < T; ++t) {
    SubVector<float> row(out + (long)t * 40, 40);
    cmvn.GetFrame(t, &row);
  }
}

// One Fbank::Process call on a fresh Instance (src/fbank.cc:265-314).  out
// holds cap x 40 floats; returns the frame count, -1 if it exceeds cap.
int ref_fbank(const float *wave, long n, float *out, int cap) {
  pocketkaldi::Fbank fbank;
  pocketkaldi::Fbank::Instance inst;
  Matrix<float> feats;
  SubVector<float> w(const_cast<float *>(wave), (int)n);
  fbank.Process(&inst, w, &feats);
  return append(feats, out, 0, cap, 40);
}

// One Fbank::Instance fed the wave in pieces of piece_sizes[0], [1], ... (the
// list is cycled; every size > 0) until the n samples are used up.
int ref_fbank_stream(const float *wave, long n, const int *piece_sizes, int n_pieces, float *out, int cap) {
  pocketkaldi::Fbank fbank;
  pocketkaldi::Fbank::Instance inst;
  int rows = 0;
  long at = 0;
  for (int p = 0; at < n; ++p) {
    long len = piece_sizes[p % n_pieces];
    if (len <= 0) return -1;
    if (len > n - at) len = n - at;
    Matrix<float> feats;
    SubVector<float> w(const_cast<float *>(wave) + at, (int)len);
    fbank.Process(&inst, w, &feats);
    rows = append(feats, out, rows, cap, 40);
    if (rows < 0) return -1;
    at += len;
  }
  return rows;
}

// pocketkaldi::Quantize (src/matrix.cc:366-387): rows x cols floats to bytes,
// scale and zero point.
void ref_quantize(const float *x, int rows, int cols, uint8_t *q, float *scale, int32_t *zero_point) {
  Matrix<float> src;
  fill(&src, x, rows, cols);
  Matrix<uint8_t> dest;
  pocketkaldi::QuantizationParams prm;
  pocketkaldi::Quantize(src, &dest, &prm);
  for (int r = 0; r < rows; ++r) memcpy(q + (long)r * cols, dest.Data() + (long)r * dest.Stride(), cols);
  *scale = prm.scale;
  *zero_point = prm.zero_point;
}

// MatMat_U8U8F32 of src/matrix.cc.  Row-major A (m x k), B (k x n), C (m x n).
void ref_matmat_u8u8f32(int m, int n, int k, const uint8_t *a, float sa, int32_t zpa,
                        const uint8_t *b, float sb, int32_t zpb, float *c) {
  Matrix<uint8_t> A(m, k), B(k, n);
  for (int r = 0; r < m; ++r) memcpy(A.Data() + (long)r * A.Stride(), a + (long)r * k, k);
  for (int r = 0; r < k; ++r) memcpy(B.Data() + (long)r * B.Stride(), b + (long)r * n, n);
  Matrix<float> C(m, n);
  pocketkaldi::QuantizationParams pa = {sa, zpa}, pb = {sb, zpb};
  pocketkaldi::MatMat_U8U8F32(A, pa, B, pb, &C);
  for (int r = 0; r < m; ++r) memcpy(c + (long)r * n, C.Row(r).Data(), sizeof(float) * n);
}

// Nnet::Read of the NN02 file, then Nnet::Propagate of x (rows x cols).  out
// holds cap floats.  Returns 0; -1: the file does not open or parse; -2: the
// output does not fit.  contexts[0..1]: the file's left and right context.
int ref_nnet_propagate(const char *nnet_path, const float *x, int rows, int cols, float *out, long cap,
                       int *out_rows, int *out_cols, int *contexts) {
  pocketkaldi::util::ReadableFile fd;
  if (!fd.Open(nnet_path).ok()) return -1;
  pocketkaldi::Nnet nnet;
  if (!nnet.Read(&fd).ok()) return -1;
  fd.Close();
  contexts[0] = nnet.left_context();
  contexts[1] = nnet.right_context();
  Matrix<float> in, y;
  fill(&in, x, rows, cols);
  nnet.Propagate(in, &y);
  *out_rows = y.NumRows();
  *out_cols = y.NumCols();
  if ((long)y.NumRows() * y.NumCols() > cap) return -2;
  return append(y, out, 0, y.NumRows(), y.NumCols()) < 0 ? -2 : 0;
}

// AcousticModel::Read of the config, Process for each of the T frames (40
// floats each), then EndOfStream (src/am.cc:115-164); the batches' rows are
// concatenated into out (cap floats, rows of num_pdfs).  Returns the row
// count; -1: the model does not read; -2: the rows do not fit.  tid2pdf holds
// tid_cap entries; *tid_n is the map's length (copied only if it fits).
int ref_am(const char *conf_path, const float *feats, int T, float *out, long cap_floats, int *num_pdfs,
           int32_t *tid2pdf, int tid_cap, int *tid_n) {
  pocketkaldi::Configuration conf;
  if (!conf.Read(conf_path).ok()) return -1;
  pocketkaldi::AcousticModel am;
  if (!am.Read(conf).ok()) return -1;
  *num_pdfs = am.num_pdfs();
  if (am.num_pdfs() <= 0) return -1;
  const int cap = (int)(cap_floats / am.num_pdfs());
  const Vector<int32_t> &map = am.TransitionPdfIdMap();
  *tid_n = map.Dim();
  if (map.Dim() <= tid_cap) memcpy(tid2pdf, map.Data(), sizeof(int32_t) * map.Dim());
  pocketkaldi::AcousticModel::Instance inst;
  int rows = 0;
  for (int t = 0; t <= T && rows >= 0; ++t) {
    Matrix<float> log_prob;
    if (t < T) {
      SubVector<float> frame(const_cast<float *>(feats) + (long)t * 40, 40);
      am.Process(&inst, frame, &log_prob);
    } else {
      am.EndOfStream(&inst, &log_prob);
    }
    rows = append(log_prob, out, rows, cap, am.num_pdfs());
  }
  return rows < 0 ? -2 : rows;
}

}  // extern "C"
