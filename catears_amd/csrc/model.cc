// model.cc -- the model object of libcatears_hip: an NN02 layer list
// (model_io.cc) turned into a device program of fused steps, the weight
// images each GEMM mode reads (weight_images.cc, uploaded here), and every
// ce_gpu_model_* entry: loading, the GEMM mode, padded widths, admitted row
// steps and the int8 forms.  What runs the program is nnet_programs.cc.
#include <float.h>
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "internal.h"
#include "model_io.h"
#include "nnet_programs.h"

using namespace catears;

namespace {

// Default matrix-core form of the fp32 program: bf16x6.  Another mode is a
// per-model choice through ce_gpu_model_set_gemm; the experiments library
// also takes CATEARS_NNET_GEMM (0 fp32, 1 bf16x6, 2 f16x3, 3 bf16x6p, 4 bf16,
// the ce_gpu_model_set_gemm numbers) for the tools.
int default_gemm() {
  static const int g = CE_KNOB("CATEARS_NNET_GEMM", (int)CE_GPU_GEMM_BF16X6);
  return g >= CE_GPU_GEMM_FP32 && g <= CE_GPU_GEMM_BF16 ? g : -1;
}

template <typename T>
int upload(DevBuf *out, const std::vector<T> &v) {
  return out->upload(v.data(), v.size() * sizeof(T));
}

// The first n floats of a device vector or matrix.
int download(const DevBuf &b, size_t n, std::vector<float> *out) {
  out->resize(n);
  if (n) CE_HIP(hipMemcpy(out->data(), b.ptr, (size_t)n * 4, hipMemcpyDeviceToHost));
  return CE_GPU_OK;
}

// Every image of one Linear's weights from its n x kpad fp32 matrix (g->n and
// g->kpad set): wt, the bf16x6 planes, the fragment image, the f16x3 planes
// with their shift.  *f16_ok: the f16x3 image exists (finite weights).
int upload_weight_images(const std::vector<float> &wt, GemmLayer *g, bool *f16_ok) {
  CE_TRY(upload(&g->wt, wt));
  CE_TRY(upload(&g->wsplit, bf16_plane_image(wt, g->n, g->kpad)));
  if (g->kpad % 32 == 0) CE_TRY(upload(&g->wdir, bf16_fragment_image(wt, g->n, g->kpad)));
  std::vector<uint16_t> f16;
  *f16_ok = f16_plane_image(wt, g->n, g->kpad, &f16, &g->w_shift);
  return *f16_ok ? upload(&g->wf16, f16) : CE_GPU_OK;
}

// The program-shape rule of the plane modes and the mode a model loads in.
// bf16x6 program: every step a Linear with its ReLU / BatchNorm fused, a
// K-tile of 32 inside one splice segment after the first layer (whose
// spliced block is written padded), output widths multiples of 4.
// m->x3_ok on entry: every weight matrix has its f16x3 image.
// A row step of its own puts the program outside, unless the model was
// admitted (ce_gpu_model_admit_row_ops): the rule then looks at the GEMM
// steps only, and the model takes CE_GPU_GEMM_BF16X6 and CE_GPU_GEMM_BF16
// but neither plane mode.
int settle_gemm_mode(ce_gpu_model *m) {
  m->x6_ok = true;
  const bool row_steps = has_row_steps(m);
  for (size_t i = 0; i < m->steps.size(); ++i) {
    const Step &st = m->steps[i];
    if (!st.is_gemm) {
      if (!m->row_ops_admitted) m->x6_ok = false;
      continue;
    }
    if (st.gemm.n % 4 != 0 || (i > 0 && st.gemm.din % 32 != 0) || st.gemm.kpad % 32 != 0) m->x6_ok = false;
  }
  m->x3_ok = m->x3_ok && m->x6_ok && !row_steps;
  const int want = default_gemm();
  if (want < 0) return fail(CE_GPU_EINVAL, "default GEMM mode: not one of 0 fp32, 1 bf16x6, 2 f16x3, 3 bf16x6p, 4 bf16");
  m->gemm = want == CE_GPU_GEMM_F16X3 && m->x3_ok   ? CE_GPU_GEMM_F16X3
            : want == CE_GPU_GEMM_BF16X6_PLANES && m->x6_ok && !row_steps ? CE_GPU_GEMM_BF16X6_PLANES
            : want == CE_GPU_GEMM_BF16 && m->x6_ok ? CE_GPU_GEMM_BF16
            : want != CE_GPU_GEMM_FP32 && m->x6_ok ? CE_GPU_GEMM_BF16X6
                                                    : CE_GPU_GEMM_FP32;
  return CE_GPU_OK;
}

// Turns the layer list into fused device steps.  The reference's converter
// always emits Splice immediately followed by Narrow(-min(idx,0), max(idx,0))
// (tool/convert_am.py:272-285); under that shape the output of a chunk does
// not depend on where the chunk boundaries are, which is what lets the GPU run
// whole utterances.  Other shapes are rejected with CE_GPU_ENOTSUP.
int build_program(const std::vector<RawLayer> &layers, int left, int right, ce_gpu_model *m) {
  m->x3_ok = true;           // cleared by a weight matrix the f16 planes cannot hold
  std::vector<int> pending;  // splice offsets waiting for their Linear
  bool have_pending = false, gemm_open = false;
  int width = -1, sum_l = 0, sum_r = 0, pend_l = 0, pend_r = 0;
  for (size_t i = 0; i < layers.size(); ++i) {
    const RawLayer &L = layers[i];
    switch (L.id) {
      case kSplice: {
        if (have_pending) return fail(CE_GPU_ENOTSUP, "two Splice layers without a Linear between them");
        if (L.idx.empty() || L.idx.size() > 8) return fail(CE_GPU_ENOTSUP, "Splice needs 1..8 indices");
        int lo = 0, hi = 0;
        for (int v : L.idx) lo = std::min(lo, v), hi = std::max(hi, v);
        if (i + 1 >= layers.size() || layers[i + 1].id != kNarrow || layers[i + 1].left != -lo ||
            layers[i + 1].right != hi)
          return fail(CE_GPU_ENOTSUP, "Splice must be followed by Narrow(-min(idx,0), max(idx,0))");
        pending.assign(L.idx.begin(), L.idx.end());
        have_pending = true;
        pend_l = -lo;
        pend_r = hi;
        gemm_open = false;
        ++i;  // the Narrow
        sum_l += -lo;
        sum_r += hi;
        if (!(i + 1 < layers.size() && layers[i + 1].id == kLinear))
          return fail(CE_GPU_ENOTSUP, "Splice/Narrow must feed a Linear layer");
        break;
      }
      case kNarrow:
        if (L.left != 0 || L.right != 0) return fail(CE_GPU_ENOTSUP, "Narrow without a preceding Splice");
        break;
      case kLinear: {
        Step st;
        GemmLayer &g = st.gemm;
        const int in = L.rows, out = L.cols;
        if ((int)L.b.size() != out)
          return fail(CE_GPU_ECORRUPT, "Corruption: Linear bias size does not match W");
        g.nseg = have_pending ? (int)pending.size() : 1;
        g.in_left = sum_l - (have_pending ? pend_l : 0);
        g.in_right = sum_r - (have_pending ? pend_r : 0);
        if (in % g.nseg != 0) return fail(CE_GPU_ECORRUPT, "Corruption: Linear input does not match Splice");
        g.din = in / g.nseg;
        for (int s = 0; s < g.nseg; ++s) g.off[s] = have_pending ? pending[s] : 0;
        if (width >= 0 && g.din != width)
          return fail(CE_GPU_ECORRUPT, fmt("Corruption: layer %zu expects width %d, got %d", i, g.din, width));
        if (m->steps.empty()) m->input_dim = g.din;
        g.k = in;
        g.kpad = (int)round_up(in, gemm_k_align());
        g.n = out;
        g.din_true = g.din;
        g.n_true = out;
        bool f16_ok = false;
        CE_TRY(upload_weight_images(transpose_padded(L.w, in, out, g.kpad), &g, &f16_ok));
        if (!f16_ok) m->x3_ok = false;
        CE_TRY(upload(&g.bias, L.b));
        m->num_params += (int64_t)in * out + out;
        m->max_width = std::max(m->max_width, out);
        ++m->num_linear;
        m->steps.push_back(std::move(st));
        have_pending = false;
        gemm_open = true;
        width = out;
        break;
      }
      case kReLU:
      case kBatchNorm: {
        if (width < 0) return fail(CE_GPU_ENOTSUP, "the first layer must be a (spliced) Linear");
        if (L.id == kBatchNorm && ((int)L.scale.size() != width || (int)L.offset.size() != width))
          return fail(CE_GPU_ECORRUPT, "Corruption: BatchNorm size does not match its input");
        GemmLayer &g = m->steps.back().gemm;
        const bool bn_free = L.id != kBatchNorm || !g.bn_scale.ptr;
        if (gemm_open && m->steps.back().is_gemm && g.npost < 4 && bn_free) {
          g.post[g.npost++] = L.id == kReLU ? kPostRelu : kPostBatchNorm;
          if (L.id == kBatchNorm) {
            CE_TRY(upload(&g.bn_scale, L.scale));
            CE_TRY(upload(&g.bn_offset, L.offset));
            m->num_params += 2 * width;
          }
        } else {
          Step st;
          st.is_gemm = false;
          st.row.kind = L.id == kReLU ? kRowRelu : kRowBatchNorm;
          st.row.dim = width;
          if (L.id == kBatchNorm) {
            CE_TRY(upload(&st.row.scale, L.scale));
            CE_TRY(upload(&st.row.offset, L.offset));
          }
          m->steps.push_back(std::move(st));
          gemm_open = false;
        }
        break;
      }
      case kLogSoftmax:
      case kSoftmax:
      case kNormalize: {
        if (width < 0) return fail(CE_GPU_ENOTSUP, "the first layer must be a (spliced) Linear");
        if (L.id == kLogSoftmax && i + 1 == layers.size()) {
          m->final_log_softmax = true;
        } else {
          Step st;
          st.is_gemm = false;
          st.row.kind = L.id == kLogSoftmax ? kRowLogSoftmax : (L.id == kSoftmax ? kRowSoftmax : kRowNormalize);
          st.row.dim = width;
          m->steps.push_back(std::move(st));
        }
        gemm_open = false;
        break;
      }
      default:
        return fail(CE_GPU_ECORRUPT, "Corruption: unexpected layer");
    }
  }
  if (m->steps.empty() || !m->steps.front().is_gemm)
    return fail(CE_GPU_ENOTSUP, "the nnet must start with a (spliced) Linear layer");
  m->net_left = sum_l;
  m->net_right = sum_r;
  if (left < 0 && right < 0) {
    m->left = sum_l;
    m->right = sum_r;
  } else if (sum_l != left || sum_r != right)
    return fail(CE_GPU_ECORRUPT, fmt("Corruption: config context (%d, %d) differs from the nnet's (%d, %d)",
                                     left, right, sum_l, sum_r));
  m->num_pdfs = width;
  return settle_gemm_mode(m);
}

// The int8 form of one Linear at quantize time: the int8 image of its weight
// matrix (read back from the device) and how the layer's quantized input is
// addressed.
int quantize_weights(Step &st) {
  GemmLayer &g = st.gemm;
  I8Layer &L = st.i8;
  std::vector<float> wt;
  CE_TRY(download(g.wt, (size_t)g.n * g.kpad, &wt));
  const int ka = i8_k_align();
  const Int8Image im = int8_image(wt, g.n, g.k, g.kpad, ka);
  L.w_zp = im.zero_point;
  L.w_scale = im.scale;
  L.n = g.n;
  L.k = g.k;
  L.kpad = im.kpad;
  CE_TRY(upload(&L.wq, im.q));
  CE_TRY(upload(&L.colsum, im.colsum));
  L.in_width = g.din;
  L.in_left = g.in_left;
  L.in_right = g.in_right;
  L.spliced = g.din % ka != 0;
  if (L.spliced) {
    L.a_din = L.kpad;
    L.a_nseg = 1;
    for (int i = 0; i < 8; ++i) L.a_off[i] = 0;
  } else {
    L.a_din = g.din;
    L.a_nseg = g.nseg;
    for (int i = 0; i < 8; ++i) L.a_off[i] = g.off[i];
  }
  L.bias = g.bias.as<float>();
  L.bn_scale = g.bn_scale.as<float>();
  L.bn_offset = g.bn_offset.as<float>();
  for (int i = 0; i < 4; ++i) L.post[i] = g.post[i];
  L.npost = g.npost;
  return CE_GPU_OK;
}

// Nnet::Read into a device program; `rd` is positioned at the NN02 tag.
// left/right < 0: take the context from the network's Narrow layers.
int read_program(ce_gpu_ctx *ctx, Reader &rd, int left, int right, ce_gpu_model *m) {
  CE_HIP(hipSetDevice(ctx->device));
  if ((left < 0) != (right < 0)) return fail(CE_GPU_EINVAL, "negative context");
  m->left = left;
  m->right = right;
  std::vector<RawLayer> layers;
  int hl = 0, hr = 0;
  CE_TRY(read_nnet(rd, &layers, &hl, &hr));
  return build_program(layers, left, right, m);
}

// Prior probabilities -> device log prior (ApplyLog, src/am.cc:40-44).
int set_prior(ce_gpu_model *m, const float *prior, int dim) {
  if (dim != m->num_pdfs)
    return fail(CE_GPU_ECORRUPT, fmt("Corruption: prior has %d entries, nnet outputs %d", dim, m->num_pdfs));
  std::vector<float> lp(prior, prior + dim);
  for (float &v : lp) v = logf(v);
  return upload(&m->log_prior, lp);
}

int load_model(ce_gpu_ctx *ctx, const std::string &nnet, const std::string &prior, int left, int right,
               const std::string &tid2pdf, ce_gpu_model **out) {
  std::unique_ptr<ce_gpu_model> m(new (std::nothrow) ce_gpu_model());
  if (!m) return fail(CE_GPU_ENOMEM, "out of host memory");
  if (left < 0 || right < 0) return fail(CE_GPU_EINVAL, "negative context");
  {
    Reader rd;
    CE_TRY(rd.open(nnet));
    CE_TRY(read_program(ctx, rd, left, right, m.get()));
  }
  Reader rp;
  CE_TRY(rp.open(prior));
  std::vector<float> pr;
  CE_TRY(rp.vec(&pr));
  CE_TRY(set_prior(m.get(), pr.data(), (int)pr.size()));
  if (!tid2pdf.empty()) {
    Reader rt;
    CE_TRY(rt.open(tid2pdf));
    CE_TRY(rt.vec(&m->tid2pdf));
  }
  *out = m.release();
  return CE_GPU_OK;
}

}  // namespace

// =================================================================== ABI ==

extern "C" {

int ce_gpu_model_load(ce_gpu_ctx *ctx, const char *nnet_path, const char *prior_path, int left_context,
                      int right_context, ce_gpu_model **out) {
  if (!ctx || !nnet_path || !prior_path || !out) return fail(CE_GPU_EINVAL, "NULL argument");
  *out = nullptr;
  return load_model(ctx, nnet_path, prior_path, left_context, right_context, "", out);
}

int ce_gpu_model_load_config(ce_gpu_ctx *ctx, const char *config_path, ce_gpu_model **out) {
  if (!ctx || !config_path || !out) return fail(CE_GPU_EINVAL, "NULL argument");
  *out = nullptr;
  Config cf;
  CE_TRY(cf.read(config_path));
  std::string nnet, prior, tid2pdf;
  int left = 0, right = 0, chunk = 0, num_pdfs = 0;
  CE_TRY(cf.path("nnet", &nnet));
  CE_TRY(cf.path("prior", &prior));
  CE_TRY(cf.integer("left_context", &left));
  CE_TRY(cf.integer("right_context", &right));
  CE_TRY(cf.integer("chunk_size", &chunk));
  CE_TRY(cf.integer("num_pdfs", &num_pdfs));
  CE_TRY(cf.path("tid2pdf", &tid2pdf));
  // gpu_gemm: the GEMM mode from the config; a bad name fails before any upload
  int gemm = -1;
  CE_TRY(read_gpu_gemm(cf, &gemm));
  // gpu_pad_widths: the re-layout onto padded widths, before gpu_gemm
  int pad = 0;
  CE_TRY(read_gpu_pad_widths(cf, &pad));
  // gpu_row_ops: the row steps admitted to the matrix-core programs, before both
  int row_ops = 0;
  CE_TRY(read_gpu_row_ops(cf, &row_ops));
  ce_gpu_model *m = nullptr;
  CE_TRY(load_model(ctx, nnet, prior, left, right, tid2pdf, &m));
  m->chunk = chunk;
  std::unique_ptr<ce_gpu_model> own(m);
  if (row_ops) {
    const int rc = ce_gpu_model_admit_row_ops(ctx, m);
    if (rc != CE_GPU_OK) return fail(rc, cf.file + ": gpu_row_ops = 1: " + last_error());
  }
  if (pad) {
    const int rc = ce_gpu_model_pad_widths(ctx, m);
    if (rc != CE_GPU_OK) return fail(rc, cf.file + ": gpu_pad_widths = 1: " + last_error());
  }
  if (gemm >= 0) {
    const int rc = ce_gpu_model_set_gemm(m, gemm);
    if (rc != CE_GPU_OK) return fail(rc, cf.file + ": gpu_gemm = " + cf.kv["gpu_gemm"] + ": " + last_error());
  }
  // gpu_int8_ranges: static int8 from the config (model_io.cc)
  std::string ranges_path;
  std::vector<float> ranges;
  CE_TRY(read_int8_ranges(cf, &ranges, &ranges_path));
  if (!ranges.empty()) {
    const int rc = ce_gpu_model_quantize_static(ctx, m, ranges.data(), (int)(ranges.size() / 2));
    if (rc != CE_GPU_OK) return fail(rc, ranges_path + ": " + last_error());
  }
  own.release();
  *out = m;
  return CE_GPU_OK;
}

int ce_gpu_model_load_mem(ce_gpu_ctx *ctx, const void *nnet, int64_t nbytes, const float *h_prior,
                          int prior_dim, int left_context, int right_context, ce_gpu_model **out) {
  if (!ctx || !out || !nnet || nbytes <= 0 || (prior_dim > 0 && !h_prior))
    return fail(CE_GPU_EINVAL, "bad argument");
  *out = nullptr;
  std::unique_ptr<ce_gpu_model> m(new (std::nothrow) ce_gpu_model());
  if (!m) return fail(CE_GPU_ENOMEM, "out of host memory");
  Reader rd;
  CE_TRY(rd.open_mem(nnet, (size_t)nbytes, "<nnet image>"));
  CE_TRY(read_program(ctx, rd, left_context, right_context, m.get()));
  if (h_prior) CE_TRY(set_prior(m.get(), h_prior, prior_dim));
  *out = m.release();
  return CE_GPU_OK;
}

int ce_gpu_nnet_check_mem(const void *nnet, int64_t nbytes, int *num_layers, int *left, int *right) {
  if (!nnet || nbytes <= 0) return fail(CE_GPU_EINVAL, "bad argument");
  Reader rd;
  CE_TRY(rd.open_mem(nnet, (size_t)nbytes, "<nnet image>"));
  std::vector<RawLayer> layers;
  int hl = 0, hr = 0;
  CE_TRY(read_nnet(rd, &layers, &hl, &hr));
  if (num_layers) *num_layers = (int)layers.size();
  if (left) *left = hl;
  if (right) *right = hr;
  return CE_GPU_OK;
}

int ce_gpu_model_info(const ce_gpu_model *m, int *left_context, int *right_context, int *input_dim,
                      int *num_pdfs, int *num_linear, int64_t *num_params) {
  if (!m) return fail(CE_GPU_EINVAL, "model is NULL");
  if (left_context) *left_context = m->left;
  if (right_context) *right_context = m->right;
  if (input_dim) *input_dim = m->input_dim;
  if (num_pdfs) *num_pdfs = m->num_pdfs;
  if (num_linear) *num_linear = m->num_linear;
  if (num_params) *num_params = m->num_params;
  return CE_GPU_OK;
}

int ce_gpu_model_tid2pdf(const ce_gpu_model *m, int32_t *h_out, int capacity, int *size) {
  if (!m) return fail(CE_GPU_EINVAL, "model is NULL");
  const int n = (int)m->tid2pdf.size();
  if (size) *size = n;
  if (h_out && capacity > 0) memcpy(h_out, m->tid2pdf.data(), sizeof(int32_t) * std::min(n, capacity));
  return CE_GPU_OK;
}

int ce_gpu_model_destroy(ce_gpu_model *m) {
  delete m;
  return CE_GPU_OK;
}

int ce_gpu_model_set_gemm(ce_gpu_model *m, int mode) {
  if (!m) return fail(CE_GPU_EINVAL, "NULL model");
  if (mode != CE_GPU_GEMM_FP32 && mode != CE_GPU_GEMM_BF16X6 && mode != CE_GPU_GEMM_F16X3 &&
      mode != CE_GPU_GEMM_BF16X6_PLANES && mode != CE_GPU_GEMM_BF16)
    return fail(CE_GPU_EINVAL, "unknown GEMM mode");
  if (mode != CE_GPU_GEMM_FP32 && !m->x6_ok)
    return fail(CE_GPU_ENOTSUP, "this nnet program cannot run on split planes (unfused row op or widths)");
  if ((mode == CE_GPU_GEMM_F16X3 || mode == CE_GPU_GEMM_BF16X6_PLANES) && has_row_steps(m))
    return fail(CE_GPU_ENOTSUP, "this nnet program has a row step of its own: GEMM modes fp32, bf16x6 and bf16 only");
  if (mode == CE_GPU_GEMM_F16X3 && !m->x3_ok)
    return fail(CE_GPU_ENOTSUP, "a weight matrix is not finite: no f16x3 image");
  m->gemm = mode;
  return CE_GPU_OK;
}

int ce_gpu_model_get_gemm(const ce_gpu_model *m, int *mode) {
  if (!m || !mode) return fail(CE_GPU_EINVAL, "NULL argument");
  *mode = m->gemm;
  return CE_GPU_OK;
}

int ce_gpu_gemm_mode_from_name(const char *name, int *mode) {
  if (!name || !mode) return fail(CE_GPU_EINVAL, "NULL argument");
  if (!gemm_mode_from_name(name, mode)) return fail(CE_GPU_EINVAL, std::string("unknown GEMM mode name: ") + name);
  return CE_GPU_OK;
}

int ce_gpu_model_pad_widths(ce_gpu_ctx *ctx, ce_gpu_model *m) {
  if (!ctx || !m) return fail(CE_GPU_EINVAL, "NULL argument");
  if (m->int8) return fail(CE_GPU_EINVAL, "model_pad_widths: the model is quantized");
  if (m->x6_ok) return CE_GPU_OK;  // already inside the plane modes' envelope (or padded)
  if (!m->row_ops_admitted && has_row_steps(m))
    return fail(CE_GPU_ENOTSUP, "model_pad_widths: the program has an unfused row op");
  CE_HIP(hipSetDevice(ctx->device));
  CE_HIP(hipStreamSynchronize(ctx->stream));
  // the new layers are built beside the old ones: a failure leaves the model as it was
  const size_t nl = m->steps.size(), last_gemm = last_gemm_step(m);
  std::vector<GemmLayer> pad(nl);
  bool f16_all = true;
  int prev_n = 0, max_width = 0;
  for (size_t i = 0; i < nl; ++i) {
    // an admitted model's row steps stay as they are: dim and the BatchNorm
    // vectors at the true width, on rows whose leading dimension is padded
    if (!m->steps[i].is_gemm) continue;
    const GemmLayer &g = m->steps[i].gemm;
    GemmLayer &p = pad[i];
    p.n = (int)round_up(g.n, i == last_gemm ? 4 : 32);
    p.din = i == 0 ? g.din : prev_n;
    p.din_true = g.din;
    p.n_true = g.n;
    p.nseg = g.nseg;
    for (int s = 0; s < 8; ++s) p.off[s] = g.off[s];
    p.k = p.nseg * p.din;
    p.kpad = (int)round_up(p.k, gemm_k_align());
    for (int q = 0; q < 4; ++q) p.post[q] = g.post[q];
    p.npost = g.npost;
    p.in_left = g.in_left;
    p.in_right = g.in_right;
    std::vector<float> old;
    CE_TRY(download(g.wt, (size_t)g.n * g.kpad, &old));
    bool f16_ok = false;
    CE_TRY(upload_weight_images(relayout_padded(old, g.n, g.kpad, g.nseg, g.din, p.n, p.kpad, p.din), &p, &f16_ok));
    f16_all = f16_all && f16_ok;
    // a padded unit: bias 0, BatchNorm scale 1 and offset 0 -- +0 after any post chain
    std::vector<float> v;
    CE_TRY(download(g.bias, g.n, &v));
    CE_TRY(upload(&p.bias, padded_vector(v, p.n, 0.0f)));
    if (g.bn_scale.ptr) {
      CE_TRY(download(g.bn_scale, g.n, &v));
      CE_TRY(upload(&p.bn_scale, padded_vector(v, p.n, 1.0f)));
      CE_TRY(download(g.bn_offset, g.n, &v));
      CE_TRY(upload(&p.bn_offset, padded_vector(v, p.n, 0.0f)));
    }
    prev_n = p.n;
    max_width = std::max(max_width, p.n);
  }
  for (size_t i = 0; i < nl; ++i)
    if (m->steps[i].is_gemm) m->steps[i].gemm = std::move(pad[i]);
  m->max_width = max_width;
  m->padded = true;
  m->x3_ok = f16_all;
  return settle_gemm_mode(m);
}

int ce_gpu_model_padded_widths(const ce_gpu_model *m, int *h_true, int *h_padded, int capacity, int *count) {
  if (!m || !count) return fail(CE_GPU_EINVAL, "NULL argument");
  int n = 0;
  for (const Step &st : m->steps) {
    if (!st.is_gemm) continue;
    if (n < capacity) {
      if (h_true) h_true[n] = st.gemm.n_true;
      if (h_padded) h_padded[n] = st.gemm.n;
    }
    ++n;
  }
  *count = n;
  return CE_GPU_OK;
}

int ce_gpu_model_admit_row_ops(ce_gpu_ctx *ctx, ce_gpu_model *m) {
  if (!ctx || !m) return fail(CE_GPU_EINVAL, "NULL argument");
  if (m->int8) return fail(CE_GPU_EINVAL, "model_admit_row_ops: the model is quantized (the int8 programs run row steps as they are)");
  if (m->row_ops_admitted || !has_row_steps(m)) return CE_GPU_OK;
  m->row_ops_admitted = true;
  return settle_gemm_mode(m);
}

int ce_gpu_model_quantize(ce_gpu_ctx *ctx, ce_gpu_model *m) {
  if (!ctx || !m) return fail(CE_GPU_EINVAL, "NULL argument");
  if (m->padded) return fail(CE_GPU_EINVAL, "model_quantize: the model is on padded widths (ce_gpu_model_pad_widths)");
  if (m->int8_static) return fail(CE_GPU_EINVAL, "model_quantize: the model is static int8");
  if (m->int8) return CE_GPU_OK;
  CE_HIP(hipSetDevice(ctx->device));
  for (Step &st : m->steps)
    if (st.is_gemm) CE_TRY(quantize_weights(st));
  m->int8 = true;
  return CE_GPU_OK;
}

int ce_gpu_quant_params_from_range(float min, float max, float *scale, int32_t *zero_point) {
  if (!scale || !zero_point) return fail(CE_GPU_EINVAL, "NULL argument");
  if (!std::isfinite(min) || !std::isfinite(max) || min > max)
    return fail(CE_GPU_EINVAL, fmt("quant_params_from_range: bad range [%g, %g]", (double)min, (double)max));
  if (!quant_params_from_range(min, max, scale, zero_point))
    return fail(CE_GPU_EINVAL, fmt("quant_params_from_range: [%g, %g] has no positive finite scale", (double)min,
                                   (double)(max < FLT_MIN ? FLT_MIN : max)));
  return CE_GPU_OK;
}

int ce_gpu_model_calibrate(ce_gpu_ctx *ctx, const ce_gpu_model *m, const ce_gpu_plan *p, const float *d_feats,
                           int accumulate, float *h_ranges) {
  if (!ctx || !m || !p || !h_ranges) return fail(CE_GPU_EINVAL, "NULL argument");
  if (m->int8) return fail(CE_GPU_EINVAL, "model_calibrate: the model is already quantized");
  if (!p->has_model || p->left != m->left || p->right != m->right)
    return fail(CE_GPU_EINVAL, "plan was not built for this model's context");
  if (m->left != m->net_left || m->right != m->net_right)
    return fail(CE_GPU_EINVAL, "model context differs from its network's");
  if (!p->chunks.empty() && !d_feats) return fail(CE_GPU_EINVAL, "NULL argument");
  const int n = m->num_linear;
  if (!accumulate)
    for (int i = 0; i < n; ++i) h_ranges[2 * i] = FLT_MAX, h_ranges[2 * i + 1] = FLT_MIN;  // FindMinMax's seeds
  if (p->chunks.empty()) return CE_GPU_OK;
  CE_HIP(hipSetDevice(ctx->device));
  const size_t r_bytes = round_up((size_t)n * 8, 256);
  DevBuf work;
  CE_TRY(work.alloc(r_bytes + i8_params_scratch_bytes()));
  CalibTap tap;
  tap.ranges = work.as<float>();
  tap.part = static_cast<char *>(work.ptr) + r_bytes;
  CE_HIP(hipMemcpyAsync(tap.ranges, h_ranges, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  for (const ce_gpu_plan::Chunk &c : p->chunks) {
    const float *y = nullptr;
    int ldy = 0;
    tap.linear = 0;
    tap.row_edge = p->d_row_edge.as<uint32_t>() + c.map_base;
    CE_TRY(run_steps(ctx, m, d_feats, m->input_dim, c.rows, p->d_row_src.as<int>() + c.map_base, tap.row_edge, &y,
                     &ldy, nullptr, &tap));
  }
  CE_HIP(hipMemcpyAsync(h_ranges, tap.ranges, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  CE_HIP(hipStreamSynchronize(ctx->stream));
  return CE_GPU_OK;
}

int ce_gpu_model_quantize_static(ce_gpu_ctx *ctx, ce_gpu_model *m, const float *h_ranges, int n_ranges) {
  if (!ctx || !m || !h_ranges) return fail(CE_GPU_EINVAL, "NULL argument");
  if (m->padded)
    return fail(CE_GPU_EINVAL, "model_quantize_static: the model is on padded widths (ce_gpu_model_pad_widths)");
  if (m->int8) return fail(CE_GPU_EINVAL, "model_quantize_static: the model is already quantized");
  if (n_ranges != m->num_linear)
    return fail(CE_GPU_EINVAL, fmt("model_quantize_static: %d ranges for %d Linear layers", n_ranges, m->num_linear));
  struct HostQP {
    float scale;
    int32_t zp;
  };
  std::vector<HostQP> qp(n_ranges);
  for (int i = 0; i < n_ranges; ++i)
    CE_TRY(ce_gpu_quant_params_from_range(h_ranges[2 * i], h_ranges[2 * i + 1], &qp[i].scale, &qp[i].zp));
  CE_HIP(hipSetDevice(ctx->device));
  DevBuf d_qp;
  CE_TRY(upload(&d_qp, qp));
  for (Step &st : m->steps)
    if (st.is_gemm) CE_TRY(quantize_weights(st));
  // nothing below fails: the model changes only now
  m->i8_qp = std::move(d_qp);
  int i = 0;
  m->qp_scale.clear();
  m->qp_zp.clear();
  for (Step &st : m->steps) {
    if (!st.is_gemm) continue;
    st.i8.qp = m->i8_qp.as<HostQP>() + i;
    m->qp_scale.push_back(qp[i].scale);
    m->qp_zp.push_back(qp[i].zp);
    ++i;
  }
  m->int8 = true;
  m->int8_static = true;
  return CE_GPU_OK;
}

int ce_gpu_model_quant_params(const ce_gpu_model *m, float *h_scale, int32_t *h_zero_point, int capacity, int *count) {
  if (!m || !count) return fail(CE_GPU_EINVAL, "NULL argument");
  const int n = m->int8_static ? (int)m->qp_scale.size() : 0;
  *count = n;
  for (int i = 0; i < std::min(n, std::max(capacity, 0)); ++i) {
    if (h_scale) h_scale[i] = m->qp_scale[i];
    if (h_zero_point) h_zero_point[i] = m->qp_zp[i];
  }
  return CE_GPU_OK;
}

}  // extern "C"
