// nnet_programs.cc -- what the GPU runs for one chunk of packed rows: one
// host-side program per GEMM mode (run_steps dispatches on the model), each
// with one Layout that says where its buffers lie in the context's
// workspaces.  A program sizes and addresses its buffers through its layout
// function only; reserve_packed_rows takes the largest of the same functions
// over the programs a model can be switched to.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <vector>

#include "internal.h"
#include "nnet_programs.h"

namespace catears {

int diag_skip() {
  static const int v = CE_KNOB("CATEARS_SKIP", 0);
  return v;
}

// ------------------------------------------------------------ workspace --

static int ensure_workspace(ce_gpu_ctx *ctx, size_t floats) {
  if (ctx->workspace_floats >= floats) return CE_GPU_OK;
  CE_HIP(hipStreamSynchronize(ctx->stream));  // old buffer may still be in use
  CE_TRY(ctx->workspace.alloc(floats * sizeof(float)));
  ctx->workspace_floats = floats;
  return CE_GPU_OK;
}

int ensure_scratch(ce_gpu_ctx *ctx, size_t bytes) {
  if (ctx->scratch.bytes >= bytes) return CE_GPU_OK;
  CE_HIP(hipStreamSynchronize(ctx->stream));
  return ctx->scratch.alloc(bytes);
}

// the latency GEMMs' slice partials (one window of rows), 4-byte words
static int ensure_lat_part(ce_gpu_ctx *ctx, size_t words) {
#ifdef CATEARS_EXPERIMENTS
  // the split-K fix-up's tickets (CATEARS_LAT_FIXUP, measured slower:
  // DESIGN.md §8 round 6), zeroed once: every fix-up launch leaves them zero
  if (!ctx->lat_tickets.ptr) {
    CE_TRY(ctx->lat_tickets.upload(std::vector<unsigned>(kX6LatTickets, 0u).data(), kX6LatTickets * sizeof(unsigned)));
  }
#endif
  if (ctx->lat_part.bytes >= words * 4) return CE_GPU_OK;
  CE_HIP(hipStreamSynchronize(ctx->stream));
  return ctx->lat_part.alloc(words * 4);
}

static int ensure_overflow_word(ce_gpu_ctx *ctx) {
  if (ctx->overflow.ptr) return CE_GPU_OK;
  CE_TRY(ctx->overflow.alloc(256));
  CE_HIP(hipMemsetAsync(ctx->overflow.ptr, 0, 256, ctx->stream));
  return CE_GPU_OK;
}

// What one program needs of the context for one row count, and where its
// buffers lie.  Offsets a program does not use stay 0.
struct Layout {
  // ctx->workspace: two ping-pong activation blocks at 0 and `blk`; the
  // operand-chain programs' fp32 output at `out`; plain bf16's fp32 block
  // ahead of row steps at `f32`
  size_t ws_floats = 0, blk = 0, out = 0, f32 = 0;
  // ctx->scratch.  fp32: the first layer's spliced block.  int8: operand
  // buffers at 0 (and `xq_stride`, static), row-sum buffers at `rowsum` +
  // i * `rowsum_stride`, the dynamic program's parameters and min / max
  // partials at `params` and `part`
  size_t scratch_bytes = 0, xq_stride = 0, rowsum = 0, rowsum_stride = 0, params = 0, part = 0;
  size_t lat_words = 0;   // ctx->lat_part (latency mode)
  bool overflow = false;  // ctx->overflow (f16x3)
};

static int ensure_layout(ce_gpu_ctx *ctx, const Layout &L) {
  if (L.overflow) CE_TRY(ensure_overflow_word(ctx));
  CE_TRY(ensure_workspace(ctx, L.ws_floats));
  if (L.scratch_bytes) CE_TRY(ensure_scratch(ctx, L.scratch_bytes));
  if (L.lat_words) CE_TRY(ensure_lat_part(ctx, L.lat_words));
  return CE_GPU_OK;
}

static void cover(Layout *all, const Layout &L) {
  all->ws_floats = std::max(all->ws_floats, L.ws_floats);
  all->scratch_bytes = std::max(all->scratch_bytes, L.scratch_bytes);
  all->lat_words = std::max(all->lat_words, L.lat_words);
  all->overflow = all->overflow || L.overflow;
}

// ---------------------------------------------------------------- knobs --

// CATEARS_SPLICE_FIRST=0 (experiments library) keeps the gather loader for
// narrow segments (A/B).
static bool splice_first_layer() {
  static const bool on = CE_KNOB("CATEARS_SPLICE_FIRST", 1) != 0;
  return on;
}

static int x6_variant_env() {
  static const int v = CE_KNOB("CATEARS_X6_VARIANT", 0);
  return v;
}

// bf16x6 with fp32 operands in HBM (gemm_bf16x6f_kernel: the split into
// planes happens on the way into LDS): the layers chain fp32 activations as
// the fp32 program does, the weights are the fp32 `wt` matrices.  4 B per
// operand element through L2 instead of the planes' 6; measured +3 % over
// the plane kernels (tools/ab.sh).
// Default; CATEARS_X6_F32IN=0 selects the plane-operand kernels (the
// ChainX6 program: planes written by each epilogue, bit-identical results).
static bool x6_f32in() {
  static const bool v = CE_KNOB("CATEARS_X6_F32IN", 1) != 0;
  return v;
}

// CATEARS_X6_FIRST=0 keeps the round-3 splice_pad launch before the first
// layer's throughput GEMM (bit-identical; the default gathers in its loader)
static bool x6_first_direct() {
  static const bool v = CE_KNOB("CATEARS_X6_FIRST", 1) != 0;
  return v && (x6_variant_env() == 0 || x6_variant_env() == 300);
}

// CATEARS_X6_CHAIN: the layers hand each other their outputs as bf16 planes
// (the direct-weight kernel's OUT16 epilogue, read by its PIN loader), so
// each activation is split once, in the epilogue that produces it, instead of
// by every unit tile of the next layer that reads it.  Bit-identical to the
// fp32 chain (tests/test_gpu_x6_variants.py).
// 2: only the output layer reads planes (its 14 unit tiles would each split
// the same activations), written by the layer before it.
static int x6_plane_chain_env() {
  static const int v = CE_KNOB("CATEARS_X6_CHAIN", 0);
  return v;
}

// CATEARS_LAT_FUSED_FINAL=0 keeps the last layer's split-K reduce as its own
// launch before the finalize (bit-identical; the default fuses the two)
static bool lat_fused_final() {
  static const bool v = CE_KNOB("CATEARS_LAT_FUSED_FINAL", 1) != 0;
  return v;
}

// -------------------------------------------------------- shared pieces --

static int tap_input(ce_gpu_ctx *ctx, CalibTap *tap, const GemmLayer &g, const float *x, int ldx, int rows,
                     const int *row_map) {
  if (!tap) return CE_GPU_OK;
  // the net's own columns: a padded model's zero columns are no activations
  return launch_i8_range(ctx->stream, x, ldx, rows, g.din_true, row_map, tap->row_edge, g.in_left, g.in_right,
                         tap->part, tap->ranges + 2 * tap->linear++);
}

// An incremental session chunk (inc, internal.h) runs every Linear causally:
// the layer's splice offsets less their largest one.  Without inc: as they are.
static int causal_shift(const GemmLayer &g, const IncrChunk *inc) {
  if (!inc) return 0;
  int mx = g.off[0];
  for (int i = 1; i < g.nseg; ++i) mx = std::max(mx, g.off[i]);
  return mx;
}

static void layer_offsets(const GemmLayer &g, const IncrChunk *inc, int *off) {
  const int shift = causal_shift(g, inc);
  for (int i = 0; i < 8; ++i) off[i] = inc && i >= g.nseg ? 0 : g.off[i] - shift;
}

// ... and exchanges the slots' cached context rows on Linear `linear`'s input
// (rows of row_bytes bytes, ld_bytes apart) before the launch that reads it
// through those offsets.
static int exchange_input(ce_gpu_ctx *ctx, const IncrChunk *inc, int linear, const void *buf, size_t row_bytes,
                          size_t ld_bytes, int32_t *rowsum = nullptr) {
  if (!inc || linear == 0) return CE_GPU_OK;
  return launch_session_exchange(ctx->stream, *inc, linear, const_cast<void *>(buf), row_bytes, ld_bytes, rowsum);
}

// The K geometry of a GEMM launch (GemmArgs / X6Gemm / X3Gemm): nseg segments
// of din columns read through the row offsets off (NULL: none).
template <class Args>
static void fill_geometry(Args &a, int din, int nseg, const int *off) {
  a.din = din;
  a.nseg = nseg;
  for (int s = 0; s < 8; ++s) a.off[s] = off ? off[s] : 0;
}

// ... and its epilogue: bias and the layer's fused post chain.
template <class Args>
static void fill_epilogue(Args &a, const GemmLayer &g) {
  a.bias = g.bias.as<float>();
  a.bn_scale = g.bn_scale.as<float>();
  a.bn_offset = g.bn_offset.as<float>();
  for (int q = 0; q < 4; ++q) a.post[q] = g.post[q];
  a.npost = g.npost;
}

// The widest operand row of a matrix-core program: a Linear's padded K, or
// its output rounded up to `round` columns for the layer that reads it.
static int max_operand_width(const ce_gpu_model *m, int round) {
  int w = 0;
  for (const Step &st : m->steps)
    if (st.is_gemm) w = std::max(w, std::max(st.gemm.kpad, (int)round_up(st.gemm.n, round)));
  return w;
}

size_t last_gemm_step(const ce_gpu_model *m) {
  size_t last = 0;
  for (size_t i = 0; i < m->steps.size(); ++i)
    if (m->steps[i].is_gemm) last = i;
  return last;
}

// The row steps at *si .. (up to the next Linear), in place on the fp32 rows
// the Linear before them wrote: one launch_rowop_chain per kRowChainMax
// steps.  With out16 the last launch leaves the rows as bf16 there instead,
// width16 columns of them (the plain bf16 program's hand-over to the next
// Linear).  With bytes the last launch leaves them as the next Linear's
// shifted bytes and row sums instead (the static int8 program's hand-over:
// launch_rowop_chain_q).  *si ends on the next GEMM step, or behind the last
// step; *launches (optional) grows by the launches made.
struct RowBytes {
  int8_t *q;
  int ldq;
  const void *qp;
  int32_t *rowsum, *zero;
};

static int run_row_steps(ce_gpu_ctx *ctx, const ce_gpu_model *m, size_t *si, float *x, int ldx, int rows,
                         uint16_t *out16 = nullptr, int ld16 = 0, int width16 = 0, const RowBytes *bytes = nullptr,
                         int *launches = nullptr) {
  size_t end = *si;
  while (end < m->steps.size() && !m->steps[end].is_gemm) ++end;
  while (*si < end) {
    RowChain ch;
    ch.dim = m->steps[*si].row.dim;
    for (; *si < end && ch.n < kRowChainMax; ++*si, ++ch.n) {
      const RowOp &op = m->steps[*si].row;
      ch.kind[ch.n] = op.kind;
      ch.scale[ch.n] = op.scale.as<float>();
      ch.offset[ch.n] = op.offset.as<float>();
    }
    const bool store16 = out16 && *si == end;
    if (bytes && *si == end) {
      // the next Linear's quantize pass as well, and timed as one: a
      // profiled call counts a CE_GPU_PROF_QUANT launch per Linear whose
      // bytes no GEMM epilogue wrote, whichever kernel wrote them
      ProfScope prof(ctx, CE_GPU_PROF_QUANT);
      CE_TRY(launch_rowop_chain_q(ctx->stream, ch, x, ldx, rows, ch.dim, bytes->q, bytes->ldq, bytes->qp, bytes->rowsum,
                                  bytes->zero));
    } else {
      CE_TRY(launch_rowop_chain(ctx->stream, ch, x, ldx, rows, store16 ? out16 : nullptr, ld16, width16));
    }
    if (launches) ++*launches;
    ctx->chain_end = nullptr;  // an untimed launch breaks a ProfChain
  }
  return CE_GPU_OK;
}

// ---------------------------------------------------------------- fp32 --

// Two blocks of rows x max_width floats (the int8 programs' fp32 activations
// as well); the spliced block of a first layer narrower than a K-tile.
static Layout layout_f32(const ce_gpu_model *m, int rows) {
  Layout L;
  L.blk = (size_t)rows * m->max_width;
  L.ws_floats = 2 * L.blk;
  if (splice_first_layer())
    for (const Step &st : m->steps)
      if (st.is_gemm && st.gemm.din % 32 != 0)
        L.scratch_bytes = std::max(L.scratch_bytes, (size_t)rows * st.gemm.kpad * sizeof(float));
  return L;
}

static int run_steps_f32(ce_gpu_ctx *ctx, const ce_gpu_model *m, const float *x, int ldx, int rows,
                         const int *row_map, const float **y, int *ldy, CalibTap *tap = nullptr,
                         const IncrChunk *inc = nullptr) {
  const Layout L = layout_f32(m, rows);
  CE_TRY(ensure_layout(ctx, L));
  float *buf[2] = {ctx->workspace.as<float>(), ctx->workspace.as<float>() + L.blk};
  int cur = 0, linear = 0;
  bool first = true;
  for (const Step &st : m->steps) {
    if (st.is_gemm) {
      const GemmLayer &g = st.gemm;
      GemmArgs a;
      a.x = x;
      a.ldx = ldx;
      a.row_map = first ? row_map : nullptr;
      a.m = rows;
      a.n = g.n;
      a.k = g.k;
      a.kpad = g.kpad;
      int off[8];
      layer_offsets(g, inc, off);
      fill_geometry(a, g.din, g.nseg, off);
      CE_TRY(exchange_input(ctx, inc, linear++, x, (size_t)g.din * 4, (size_t)ldx * 4));
      a.w = g.wt.as<float>();
      a.ldw = g.kpad;
      fill_epilogue(a, g);
      a.y = buf[cur];
      a.ldy = g.n;
      CE_TRY(tap_input(ctx, tap, g, x, ldx, rows, a.row_map));
      {
        ProfScope prof(ctx, g.din % 32 == 0 ? CE_GPU_PROF_GEMM : CE_GPU_PROF_GEMM_GATHER);
        if (g.din % 32 != 0 && splice_first_layer()) {
          // Segments narrower than a K-tile (the 40-wide first layer):
          // write the spliced block once (rows x kpad, zero padded) and run
          // the fast kernel on it -- cheaper than a per-element gather loader.
          float *xs = static_cast<float *>(ctx->scratch.ptr);
          CE_TRY(launch_splice_pad(ctx->stream, x, ldx, rows, g.din, g.nseg, off, a.row_map, xs, g.kpad));
          a.x = xs;
          a.ldx = g.kpad;
          a.row_map = nullptr;
          a.k = g.kpad;  // the padding columns are zero on both sides
          fill_geometry(a, g.kpad, 1, nullptr);
        }
        CE_TRY(launch_gemm_f32(ctx->stream, a));
      }
      x = buf[cur];
      ldx = g.n;
      cur ^= 1;
      first = false;
    } else if (!m->row_ops_admitted) {
      CE_TRY(launch_rowop(ctx->stream, st.row, const_cast<float *>(x), ldx, rows));
    } else if ((&st)[-1].is_gemm) {
      // an admitted model (ce_gpu_model_admit_row_ops): the run of row steps
      // that starts here in one launch per chain -- the same bits
      size_t si = &st - m->steps.data();
      CE_TRY(run_row_steps(ctx, m, &si, const_cast<float *>(x), ldx, rows));
    }
  }
  *y = x;
  *ldy = ldx;
  return CE_GPU_OK;
}

// -------------------------------------------- bf16x6, fp32 activations --

// The plane chain (CATEARS_X6_CHAIN) as far as the model decides it: the
// first layer gathers the caller's fp32 rows in its loader, every layer has
// the fragment image, the later layers' segments are whole K-tiles.
static bool x6f_planes_ok(const ce_gpu_model *m) {
  bool ok = x6_plane_chain_env() != 0 && x6_first_direct() && !has_row_steps(m) && m->steps[0].gemm.din % 8 == 0;
  for (size_t i = 0; ok && i < m->steps.size(); ++i)
    ok = m->steps[i].gemm.wdir.ptr && (i == 0 || m->steps[i].gemm.din % 32 == 0);
  return ok;
}

// Two blocks of rows x max_in floats, or of planes (rows x 3 x max_in bf16:
// 1.5 floats per element), and the fp32 output; in latency mode the largest
// layer's slice partials.
static Layout layout_x6f(const ce_gpu_model *m, int rows, bool latency, bool planes) {
  Layout L;
  L.blk = round_up((size_t)rows * max_operand_width(m, 32) * (planes ? 3 : 2) / 2, 64);
  L.out = 2 * L.blk;
  L.ws_floats = L.out + (size_t)rows * m->steps[last_gemm_step(m)].gemm.n;  // the last Linear's leading dimension
  for (size_t i = 0; latency && i < m->steps.size(); ++i) {
    if (!m->steps[i].is_gemm) continue;
    const GemmLayer &g = m->steps[i].gemm;
    const int kpad = i == 0 ? g.kpad : g.nseg * g.din;
    L.lat_words = std::max(L.lat_words, x6_lat_part_floats(rows, g.n, x6_lat_slices(kpad, g.n)));
  }
  return L;
}

static int run_steps_x6f(ce_gpu_ctx *ctx, const ce_gpu_model *m, const float *x, int ldx, int rows,
                         const int *row_map, const float **y, int *ldy, LatTail *tail, CalibTap *tap = nullptr,
                         const IncrChunk *inc = nullptr) {
  const int chain_mode = x6_plane_chain_env();
  const bool planes = chain_mode != 0 && !ctx->latency && ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 &&
                      x6f_planes_ok(m);
  const Layout L = layout_x6f(m, rows, ctx->latency != 0, planes);
  CE_TRY(ensure_layout(ctx, L));
  float *buf[2] = {ctx->workspace.as<float>(), ctx->workspace.as<float>() + L.blk};
  float *out = ctx->workspace.as<float>() + L.out;
  const float *xs = nullptr;
  int px = 0, cur = 0;
  ProfChain chain(ctx);  // every step below is one launch; GEMMs back to back
  const size_t last_gemm = last_gemm_step(m);
  int linear = 0;
  for (size_t i = 0; i < m->steps.size();) {
    // every step is a Linear but for an admitted model's row steps, which the
    // bottom of the loop runs behind the Linear they follow
    const GemmLayer &g = m->steps[i].gemm;
    const bool last = i == last_gemm;
    X6Gemm a;
    // calibration: the block entering this layer's Splice (the caller's rows,
    // or the previous layer's fp32 output)
    CE_TRY(i == 0 ? tap_input(ctx, tap, g, x, ldx, rows, row_map) : tap_input(ctx, tap, g, xs, px, rows, nullptr));
    // the latency kernel and the default direct-weight kernel splice the
    // caller's rows themselves (din % 8 == 0): no splice_pad launch
    const bool lat_direct = i == 0 && g.din % 8 == 0 && ldx % 4 == 0 &&
                            (reinterpret_cast<uintptr_t>(x) & 15) == 0 &&
                            (ctx->latency || (g.wdir.ptr && x6_first_direct()));
    int off[8];
    layer_offsets(g, inc, off);
    if (lat_direct) {
      xs = x;
      px = ldx;
      fill_geometry(a, g.din, g.nseg, off);
      a.row_map = row_map;
    } else if (i == 0) {
      ProfScope prof(ctx, CE_GPU_PROF_GEMM_GATHER);
      CE_TRY(launch_splice_pad(ctx->stream, x, ldx, rows, g.din, g.nseg, off, row_map, buf[cur], g.kpad));
      xs = buf[cur];
      px = g.kpad;
      cur ^= 1;
      fill_geometry(a, g.kpad, 1, nullptr);
    } else {
      fill_geometry(a, g.din, g.nseg, off);
      // (never the plane chain: an experiments-library knob, off by default)
      CE_TRY(exchange_input(ctx, inc, linear, xs, (size_t)px * 4, (size_t)px * 4));
    }
    ++linear;
    // planes into layer i / out of it: every layer after the first (mode 1),
    // or the output layer only (mode 2)
    const size_t nst = m->steps.size();
    const bool pin = planes && i > 0 && (chain_mode != 2 || i + 1 == nst);
    const bool pout = planes && !last && (chain_mode != 2 || i + 2 == nst);
    if (pin) {
      a.x = reinterpret_cast<const uint16_t *>(xs);
      a.ldx = 3 * px;
      a.px = px;
    } else {
      a.xf = xs;
      a.ldx = px;
    }
    a.wf = g.wt.as<float>();
    a.ldw = g.kpad;
    a.w = g.wsplit.as<uint16_t>();  // the same weights as planes (kernels that read them)
    a.pw = g.kpad;
    a.wd = g.wdir.as<uint16_t>();   // and as MFMA fragments (the default kernel)
    a.wd_kt = g.kpad / 32;
    a.wide = ctx->wide_tiles != 0;
    a.m = rows;
    a.n = g.n;
    a.kpad = i == 0 ? g.kpad : g.nseg * g.din;
    fill_epilogue(a, g);
    const int pn = (g.n + 31) / 32 * 32;
    if (pout) {
      a.y16 = reinterpret_cast<uint16_t *>(buf[cur]);
      a.ldy = 3 * pn;
      a.py = pn;
    } else {
      a.y32 = last ? out : buf[cur];
      a.ldy = last ? g.n : pn;
    }
    {
      ProfScope prof(ctx, CE_GPU_PROF_GEMM);
      if (ctx->latency) {
        const size_t pf = x6_lat_part_floats(a.m, a.n, x6_lat_slices(a.kpad, a.n));
        // the reduce may run inside the finalize -- which writes whole
        // float4 chunks of a row as wide as the partials, so not for a last
        // layer on a padded width (lat_reduce + launch_finalize then)
        // ... nor when row steps follow it: they need the reduced block
        if (last && i + 1 == m->steps.size() && lat_fused_final() && g.n == m->num_pdfs) a.tail = tail;
        CE_TRY(launch_gemm_bf16x6_lat(ctx->stream, a, ctx->lat_part.as<float>(), pf, ctx->lat_tickets.as<unsigned>()));
      } else if (!(diag_skip() & (i == 0 ? 1 : last ? 16 : 32))) {
        CE_TRY(launch_gemm_bf16x6(ctx->stream, a));
      }
    }
    ++i;
    // row steps behind this Linear: in place on the fp32 block it wrote (in
    // latency mode after the slice reduce), so the next Linear -- its tap and
    // its cache exchange -- sees its input after them
    CE_TRY(run_row_steps(ctx, m, &i, a.y32, a.ldy, rows));
    xs = buf[cur];
    px = pn;
    cur ^= 1;
  }
  *y = out;
  *ldy = m->steps[last_gemm].gemm.n;
  return CE_GPU_OK;
}

// ------------------------------------------ the 16-bit operand chains --

// Three programs are one loop: the first layer's spliced block is written
// into ping-pong block 0 as 16-bit words, every hidden layer's epilogue
// writes its output in that form for the next, the last layer writes fp32.
// A mode is described by: kWords 16-bit words per element (planes of width
// px side by side in a row), kRound the column count output widths round up
// to, kIncremental whether it runs an incremental session's chunk, kOverflow
// whether it reports through ctx->overflow, its splice and GEMM launchers,
// and weights(), which sets the weight and extra fields of its launch.

// bf16x6 on plane operands (kernels/gemm_bf16x6.hip, CE_GPU_GEMM_BF16X6_PLANES):
// three bf16 planes per operand.
struct ChainX6 {
  using Args = X6Gemm;
  static constexpr int kWords = 3, kRound = 32;
  static constexpr bool kIncremental = false, kOverflow = false;
  static int splice(ce_gpu_ctx *ctx, const float *x, int ldx, int rows, const GemmLayer &g, const int *off,
                    const int *row_map, uint16_t *out) {
    return launch_splice_pad_split(ctx->stream, x, ldx, rows, g.din, g.nseg, off, row_map, out, g.kpad);
  }
  static void weights(ce_gpu_ctx *, const GemmLayer &g, Args &a) {
    a.w = g.wsplit.as<uint16_t>();
    a.ldw = 3 * g.kpad;
    a.pw = g.kpad;
  }
  static int gemm(hipStream_t s, const Args &a) { return launch_gemm_bf16x6(s, a); }
};

// Plain bf16 (kernels/gemm_bf16.hip, CE_GPU_GEMM_BF16): bf16 activations, the
// fragment image's plane 0.  One kernel family, its tile a function of
// (rows, n); on a latency context every Linear's launch carries X6Gemm::lat,
// and launch_gemm_bf16 runs blocks of up to kB16LatMaxRows rows on
// kernels/gemm_bf16_lat.hip (the same bits, no workspace of its own).  The
// wide-tile setting is not read.
struct ChainBf16 {
  using Args = X6Gemm;
  static constexpr int kWords = 1, kRound = 32;
  static constexpr bool kIncremental = true, kOverflow = false;
  static int splice(ce_gpu_ctx *ctx, const float *x, int ldx, int rows, const GemmLayer &g, const int *off,
                    const int *row_map, uint16_t *out) {
    return launch_splice_pad_bf16(ctx->stream, x, ldx, rows, g.din, g.nseg, off, row_map, out, g.kpad);
  }
  static void weights(ce_gpu_ctx *ctx, const GemmLayer &g, Args &a) {
    a.wd = g.wdir.as<uint16_t>();
    a.wd_kt = g.kpad / 32;
    a.lat = ctx->latency != 0;
  }
  static int gemm(hipStream_t s, const Args &a) { return launch_gemm_bf16(s, a); }
};

// f16x3 (kernels/gemm_f16x3.hip, CE_GPU_GEMM_F16X3): two fp16 planes per
// operand; splits beyond the fp16 range set ctx->overflow.
struct ChainF16 {
  using Args = X3Gemm;
  static constexpr int kWords = 2, kRound = 64;
  static constexpr bool kIncremental = false, kOverflow = true;
  static int splice(ce_gpu_ctx *ctx, const float *x, int ldx, int rows, const GemmLayer &g, const int *off,
                    const int *row_map, uint16_t *out) {
    return launch_splice_pad_f16(ctx->stream, x, ldx, rows, g.din, g.nseg, off, row_map, out, g.kpad,
                                 ctx->overflow.as<int>());
  }
  static void weights(ce_gpu_ctx *ctx, const GemmLayer &g, Args &a) {
    a.w = g.wf16.as<uint16_t>();
    a.ldw = 2 * g.kpad;
    a.pw = g.kpad;
    a.unscale = ldexpf(1.0f, -(g.w_shift + kF16ActShift));
    a.overflow = ctx->overflow.as<int>();
  }
  static int gemm(hipStream_t s, const Args &a) { return launch_gemm_f16x3(s, a); }
};

// Two blocks of rows x kWords x max_in 16-bit words and the fp32 output;
// behind it (`f32`) the fp32 block of the widest hidden Linear that row steps
// follow (an admitted model in plain bf16: that Linear writes fp32, its row
// steps hand the next Linear bf16).
template <class Mode>
static Layout layout_chain16(const ce_gpu_model *m, int rows) {
  Layout L;
  L.blk = round_up(((size_t)rows * Mode::kWords * max_operand_width(m, Mode::kRound) + 1) / 2, 64);
  L.out = 2 * L.blk;
  const size_t last_gemm = last_gemm_step(m);
  L.f32 = round_up(L.out + (size_t)rows * m->steps[last_gemm].gemm.n, 64);  // the last Linear's leading dimension
  size_t hidden = 0;
  for (size_t i = 0; i < last_gemm; ++i)
    if (m->steps[i].is_gemm && !m->steps[i + 1].is_gemm)
      hidden = std::max(hidden, round_up(m->steps[i].gemm.n, Mode::kRound));
  L.ws_floats = hidden ? L.f32 + (size_t)rows * hidden : L.out + (size_t)rows * m->steps[last_gemm].gemm.n;
  L.overflow = Mode::kOverflow;
  return L;
}

template <class Mode>
static int run_steps_chain16(ce_gpu_ctx *ctx, const ce_gpu_model *m, const float *x, int ldx, int rows,
                             const int *row_map, const float **y, int *ldy, const IncrChunk *inc = nullptr) {
  if (inc && !Mode::kIncremental) return fail(CE_GPU_ENOTSUP, "incremental chunk: not in this GEMM mode");
  if (Mode::kWords != 1 && has_row_steps(m)) return fail(CE_GPU_ENOTSUP, "row steps: not on split planes");
  const Layout L = layout_chain16<Mode>(m, rows);
  CE_TRY(ensure_layout(ctx, L));
  uint16_t *sbuf[2] = {reinterpret_cast<uint16_t *>(ctx->workspace.as<float>()),
                       reinterpret_cast<uint16_t *>(ctx->workspace.as<float>() + L.blk)};
  float *out = ctx->workspace.as<float>() + L.out;
  float *hid32 = ctx->workspace.as<float>() + L.f32;
  const uint16_t *xs = nullptr;
  int px = 0, cur = 0, linear = 0;
  const size_t last_gemm = last_gemm_step(m);
  for (size_t i = 0; i < m->steps.size();) {
    // every step is a Linear but for an admitted model's row steps (plain
    // bf16 only), which the bottom of the loop runs behind their Linear
    const GemmLayer &g = m->steps[i].gemm;
    const bool last = i == last_gemm;
    // a hidden Linear with row steps behind it writes fp32, as the last one
    // does; they run in fp32 and the last of them stores bf16 for the next
    // Linear -- one rounding per value, by the consumer's rule
    const bool rows_follow = i + 1 < m->steps.size() && !m->steps[i + 1].is_gemm;
    typename Mode::Args a;
    int off[8];
    layer_offsets(g, inc, off);
    if (i == 0) {
      ProfScope prof(ctx, CE_GPU_PROF_GEMM_GATHER);
      CE_TRY(Mode::splice(ctx, x, ldx, rows, g, off, row_map, sbuf[cur]));
      xs = sbuf[cur];
      px = g.kpad;
      cur ^= 1;
      fill_geometry(a, g.kpad, 1, nullptr);
    } else {
      fill_geometry(a, g.din, g.nseg, off);
      CE_TRY(exchange_input(ctx, inc, linear, xs, (size_t)px * Mode::kWords * 2, (size_t)px * Mode::kWords * 2));
    }
    ++linear;
    a.x = xs;
    a.ldx = Mode::kWords * px;
    if (Mode::kWords > 1) a.px = px;  // (a single plane has no plane stride)
    Mode::weights(ctx, g, a);
    a.m = rows;
    a.n = g.n;
    a.kpad = i == 0 ? g.kpad : g.nseg * g.din;
    fill_epilogue(a, g);
    const int pn = (int)round_up(g.n, Mode::kRound);
    if (last) {
      a.y32 = out;
      a.ldy = g.n;
    } else if (rows_follow) {
      a.y32 = hid32;
      a.ldy = pn;
    } else {
      a.y16 = sbuf[cur];
      a.ldy = Mode::kWords * pn;
      if (Mode::kWords > 1) a.py = pn;
    }
    {
      ProfScope prof(ctx, CE_GPU_PROF_GEMM);
      CE_TRY(Mode::gemm(ctx->stream, a));
    }
    ++i;
    if (rows_follow)
      CE_TRY(run_row_steps(ctx, m, &i, a.y32, a.ldy, rows, last ? nullptr : sbuf[cur], pn, pn));
    xs = sbuf[cur];
    px = pn;
    cur ^= 1;
  }
  *y = out;
  *ldy = m->steps[last_gemm].gemm.n;
  return CE_GPU_OK;
}

// ----------------------------------------------------------------- int8 --

static int i8_max_ldq(const ce_gpu_model *m) {
  int max_ldq = 16;
  for (const Step &st : m->steps)
    if (st.is_gemm) max_ldq = std::max(max_ldq, st.i8.spliced ? st.i8.kpad : st.i8.in_width);
  return max_ldq;
}

// fp32 activation blocks as the fp32 program's; in scratch one operand
// buffer, one row-sum buffer, the block's parameters and the min / max
// partials.
static Layout layout_i8(const ce_gpu_model *m, int rows) {
  Layout L;
  L.blk = (size_t)rows * m->max_width;
  L.ws_floats = 2 * L.blk;
  int max_n = 1;
  for (const Step &st : m->steps)
    if (st.is_gemm) max_n = std::max(max_n, st.i8.n);
  L.rowsum = round_up((size_t)rows * i8_max_ldq(m), 256);
  L.params = L.rowsum + round_up((size_t)rows * 4, 256);
  L.part = L.params + 256;
  L.scratch_bytes = L.part + std::max(i8_params_scratch_bytes(), sizeof(float) * 2 * i8_gemm_parts(rows, max_n));
  return L;
}

// The int8 program (kernels/nnet_i8.hip): per Linear layer min/max ->
// quantize (+ row sums) -> u8 GEMM with float epilogue.
static int run_steps_i8(ce_gpu_ctx *ctx, const ce_gpu_model *m, const float *x, int ldx, int rows,
                        const int *row_map, const uint32_t *row_edge, const float **y, int *ldy) {
  const Layout lay = layout_i8(m, rows);
  CE_TRY(ensure_layout(ctx, lay));
  float *buf[2] = {ctx->workspace.as<float>(), ctx->workspace.as<float>() + lay.blk};
  char *base = static_cast<char *>(ctx->scratch.ptr);
  int8_t *xq = reinterpret_cast<int8_t *>(base);
  int32_t *rowsum = reinterpret_cast<int32_t *>(base + lay.rowsum);
  void *params = base + lay.params;
  void *part = base + lay.part;
  int cur = 0;
  bool first = true;
  int fused_parts = 0;  // > 0: the previous GEMM left this layer's min / max partials in `part`
  for (size_t si = 0; si < m->steps.size(); ++si) {
    const Step &st = m->steps[si];
    if (st.is_gemm) {
      const I8Layer &L = st.i8;
      const int *rm = first ? row_map : nullptr;
      const int ldq = L.spliced ? L.kpad : L.in_width;
      {
        ProfScope prof(ctx, CE_GPU_PROF_QUANT);
        const int zero[1] = {0};
        const int nseg = L.spliced ? st.gemm.nseg : 1;
        const int *offs = L.spliced ? st.gemm.off : zero;
        if (!(diag_skip() & 64)) {  // measurement library: 64 leaves the int8 quantize passes out
          if (fused_parts > 0)
            CE_TRY(launch_i8_params_fold(ctx->stream, part, fused_parts, params));
          else
            CE_TRY(launch_i8_params(ctx->stream, x, ldx, rows, L.in_width, rm, row_edge, L.in_left, L.in_right,
                                    part, params));
          CE_TRY(launch_i8_quantize(ctx->stream, x, ldx, rows, L.in_width, rm, nseg, offs, params, xq, ldq, rowsum));
        }
      }
      // the next step reads this GEMM's output directly: its min / max is
      // reduced in this GEMM's epilogue (the partials are read by the next
      // layer's fold before the next GEMM overwrites them: stream order)
      const bool fuse = si + 1 < m->steps.size() && m->steps[si + 1].is_gemm && m->steps[si + 1].i8.in_width == L.n;
      I8NextMinMax mm = {};
      if (fuse) {
        const I8Layer &N = m->steps[si + 1].i8;
        mm = I8NextMinMax{part, row_edge, N.in_left, N.in_right};
      }
      fused_parts = 0;
      ProfScope prof(ctx, CE_GPU_PROF_GEMM);
      CE_TRY(launch_i8_gemm(ctx->stream, L, xq, ldq, rows, rowsum, params, buf[cur], L.n, fuse ? &mm : nullptr,
                            fuse ? &fused_parts : nullptr));
      x = buf[cur];
      ldx = L.n;
      cur ^= 1;
      first = false;
    } else {
      // the run of row steps that starts here, one launch per chain in place
      // (launch_rowop's bits): this program's parameters are reduced over the
      // block behind them, so no byte store here
      fused_parts = 0;
      CE_TRY(run_row_steps(ctx, m, &si, const_cast<float *>(x), ldx, rows));
      --si;  // the loop steps on to the Linear behind the run
    }
  }
  *y = x;
  *ldy = ldx;
  return CE_GPU_OK;
}

// fp32 activation blocks as the fp32 program's; in scratch two operand
// buffers (a GEMM with the requantize epilogue reads one and writes the
// other) and three row-sum buffers (read / added into / cleared for the next
// launch); in latency mode the slice partials of the largest layer the slice
// rule gives the split-K pair at this row count.  Row steps that store bytes
// need nothing more: they read an fp32 block (rows x max_width) and write an
// operand buffer (rows x i8_max_ldq) and two row-sum buffers, as the quantize
// pass they replace does.
static Layout layout_i8_static(const ce_gpu_model *m, int rows, bool latency) {
  Layout L;
  L.blk = (size_t)rows * m->max_width;
  L.ws_floats = 2 * L.blk;
  L.xq_stride = round_up((size_t)rows * i8_max_ldq(m), 256);
  L.rowsum = 2 * L.xq_stride;
  L.rowsum_stride = round_up((size_t)rows * 4, 256);
  L.scratch_bytes = L.rowsum + 3 * L.rowsum_stride;
  for (const Step &st : m->steps) {
    if (!latency || !st.is_gemm || !i8_lat_eligible(st.i8, st.i8.spliced ? st.i8.kpad : st.i8.in_width)) continue;
    int slices = 0, per = 0;
    i8_lat_plan(st.i8.kpad, st.i8.n, rows, &slices, &per);
    L.lat_words = std::max(L.lat_words, i8_lat_part_words(rows, st.i8.n, slices));
  }
  return L;
}

// The static int8 program (ce_gpu_model_quantize_static): every Linear's
// activation parameters are the model's frozen ones, so nothing is reduced
// over the block.  A GEMM whose output is the next Linear's plain operand
// (that layer reads whole 128-byte K-tiles of it) writes that layer's bytes
// and row sums itself (I8NextBytes); every other layer input goes through the
// quantize pass with the frozen parameters.  CATEARS_I8_FUSED=0 (experiments
// library, read per call: tools/i8_static.py) keeps the quantize pass
// everywhere.
//   A run of row steps between two Linears goes through the chain kernel; where
// i8_rows_can_quantize holds, its last launch plays the quantize pass's role
// for the Linear behind it (launch_rowop_chain_q: that layer's bytes into
// xq[qc], their sums into rs[rc], rs[rc + 1] cleared; no rotation), and that
// Linear takes the bytes as it takes a requantizing GEMM's.
static bool i8_fused_env() { return CE_KNOB("CATEARS_I8_FUSED", 1) != 0; }

// true when the run of row steps that starts at step `first_row_step` can hand
// the Linear behind it its bytes: there is one, it reads the plain row
// (in_width bytes, ldq = in_width: not spliced), the steps work on that width,
// and the fused forms are on.  A function of the model alone: a row's bits do
// not depend on it, and no row count was measured slower.
static bool i8_rows_can_quantize(const ce_gpu_model *m, size_t first_row_step) {
  size_t end = first_row_step;
  while (end < m->steps.size() && !m->steps[end].is_gemm) ++end;
  if (end == first_row_step || end == m->steps.size() || !i8_fused_env()) return false;
  const I8Layer &N = m->steps[end].i8;
  for (size_t i = first_row_step; i < end; ++i)
    if (m->steps[i].row.dim != N.in_width) return false;
  return !N.spliced && N.qp != nullptr;
}

static std::atomic<int64_t> g_i8s_quantize{0}, g_i8s_row{0}, g_i8s_row_q{0};

void i8_static_launch_counts(int64_t *quantize_passes, int64_t *row_launches, int64_t *row_launches_q) {
  if (quantize_passes) *quantize_passes = g_i8s_quantize.load(std::memory_order_relaxed);
  if (row_launches) *row_launches = g_i8s_row.load(std::memory_order_relaxed);
  if (row_launches_q) *row_launches_q = g_i8s_row_q.load(std::memory_order_relaxed);
}

static int run_steps_i8_static(ce_gpu_ctx *ctx, const ce_gpu_model *m, const float *x, int ldx, int rows,
                               const int *row_map, const float **y, int *ldy, const IncrChunk *inc = nullptr) {
  const Layout lay = layout_i8_static(m, rows, ctx->latency != 0);
  CE_TRY(ensure_layout(ctx, lay));
  float *buf[2] = {ctx->workspace.as<float>(), ctx->workspace.as<float>() + lay.blk};
  char *base = static_cast<char *>(ctx->scratch.ptr);
  int8_t *xq[2] = {reinterpret_cast<int8_t *>(base), reinterpret_cast<int8_t *>(base + lay.xq_stride)};
  int32_t *rs[3];
  for (int i = 0; i < 3; ++i) rs[i] = reinterpret_cast<int32_t *>(base + lay.rowsum + i * lay.rowsum_stride);
  const bool fused_ok = i8_fused_env();
  int cur = 0, qc = 0, rc = 0, linear = 0;
  // have_bytes: the previous GEMM, or the row steps behind it, wrote xq[qc] / rs[rc]
  bool first = true, have_bytes = false;
  for (size_t si = 0; si < m->steps.size(); ++si) {
    const Step &st = m->steps[si];
    if (!st.is_gemm) {
      // the run of row steps that starts here (x: the fp32 rows the Linear
      // before them wrote)
      have_bytes = i8_rows_can_quantize(m, si);
      size_t end = si;
      while (end < m->steps.size() && !m->steps[end].is_gemm) ++end;
      RowBytes rb = {};
      if (have_bytes) rb = RowBytes{xq[qc], m->steps[end].i8.in_width, m->steps[end].i8.qp, rs[rc], rs[(rc + 1) % 3]};
      int launches = 0;
      CE_TRY(run_row_steps(ctx, m, &si, const_cast<float *>(x), ldx, rows, nullptr, 0, 0, have_bytes ? &rb : nullptr,
                           &launches));
      g_i8s_row.fetch_add(launches, std::memory_order_relaxed);
      if (have_bytes) g_i8s_row_q.fetch_add(1, std::memory_order_relaxed);
      --si;  // the loop steps on to the Linear behind the run
      continue;
    }
    const I8Layer &L = st.i8;
    const int ldq = L.spliced ? L.kpad : L.in_width;
    // an incremental chunk: the cached context joins the layer's input in the
    // form it has here -- fp32 rows ahead of the quantize pass, or the bytes
    // and row sums the previous GEMM or its row steps wrote -- and whichever
    // launch reads that input through the splice offsets reads it causally
    int off[8];
    layer_offsets(st.gemm, inc, off);
    if (!have_bytes) {
      CE_TRY(exchange_input(ctx, inc, linear, x, (size_t)L.in_width * 4, (size_t)ldx * 4));
      ProfScope prof(ctx, CE_GPU_PROF_QUANT);
      const int zero[1] = {0};
      CE_TRY(launch_i8_quantize(ctx->stream, x, ldx, rows, L.in_width, first ? row_map : nullptr,
                                L.spliced ? st.gemm.nseg : 1, L.spliced ? off : zero, L.qp, xq[qc], ldq, rs[rc],
                                rs[(rc + 1) % 3]));
      g_i8s_quantize.fetch_add(1, std::memory_order_relaxed);
    } else {
      CE_TRY(exchange_input(ctx, inc, linear, xq[qc], (size_t)L.in_width, (size_t)ldq, rs[rc]));
    }
    ++linear;
    const int shift = L.spliced ? 0 : causal_shift(st.gemm, inc);
    const I8Layer *N = si + 1 < m->steps.size() && m->steps[si + 1].is_gemm ? &m->steps[si + 1].i8 : nullptr;
    const bool fuse = fused_ok && N && N->in_width == L.n && !N->spliced && i8_gemm_can_requantize(L, ldq);
    // latency mode: the split-K pair where the slice rule gives it this layer
    // at this row count (the same bits, and the same row-sum rotation: either
    // producer reads rs[rc], adds into the cleared rs[rc + 1], clears rs[rc + 2])
    int lat_slices = 0, lat_per = 0;
    if (ctx->latency && i8_lat_eligible(L, ldq)) i8_lat_plan(L.kpad, L.n, rows, &lat_slices, &lat_per);
    const size_t lat_words = lat_slices > 0 ? i8_lat_part_words(rows, L.n, lat_slices) : 0;
    ProfScope prof(ctx, CE_GPU_PROF_GEMM);
    if (fuse) {
      const I8NextBytes nb = {xq[qc ^ 1], rs[(rc + 1) % 3], rs[(rc + 2) % 3], N->qp};
      if (lat_slices > 0)
        CE_TRY(launch_i8_lat(ctx->stream, L, xq[qc], ldq, rows, rs[rc], L.qp, nullptr, L.n, &nb,
                             ctx->lat_part.as<int32_t>(), lat_words, shift));
      else
        CE_TRY(launch_i8_gemm(ctx->stream, L, xq[qc], ldq, rows, rs[rc], L.qp, nullptr, L.n, nullptr, nullptr, &nb,
                              shift));
      qc ^= 1;
      rc = (rc + 1) % 3;
      x = nullptr;
    } else {
      if (lat_slices > 0)
        CE_TRY(launch_i8_lat(ctx->stream, L, xq[qc], ldq, rows, rs[rc], L.qp, buf[cur], L.n, nullptr,
                             ctx->lat_part.as<int32_t>(), lat_words, shift));
      else
        CE_TRY(launch_i8_gemm(ctx->stream, L, xq[qc], ldq, rows, rs[rc], L.qp, buf[cur], L.n, nullptr, nullptr, nullptr,
                              shift));
      x = buf[cur];
      cur ^= 1;
    }
    ldx = L.n;
    have_bytes = fuse;
    first = false;
  }
  *y = x;
  *ldy = ldx;
  return CE_GPU_OK;
}

// ------------------------------------------------------------- dispatch --

int run_steps(ce_gpu_ctx *ctx, const ce_gpu_model *m, const float *x, int ldx, int rows, const int *row_map,
              const uint32_t *row_edge, const float **y, int *ldy, LatTail *tail, CalibTap *tap,
              const IncrChunk *inc) {
  if (tail) tail->active = false;
  if (inc) {
    // an incremental session chunk (sessions_create_ex admitted these forms only)
    if (tap || (m->int8 && !m->int8_static)) return fail(CE_GPU_EINVAL, "incremental chunk: unsupported form");
    if (m->int8) return run_steps_i8_static(ctx, m, x, ldx, rows, row_map, y, ldy, inc);
    if (m->gemm == CE_GPU_GEMM_BF16) return run_steps_chain16<ChainBf16>(ctx, m, x, ldx, rows, row_map, y, ldy, inc);
    if (m->gemm == CE_GPU_GEMM_BF16X6 && ((x6_f32in() && x6_plane_chain_env() == 0) || has_row_steps(m)))
      return run_steps_x6f(ctx, m, x, ldx, rows, row_map, y, ldy, tail, nullptr, inc);
    if (m->gemm == CE_GPU_GEMM_FP32) return run_steps_f32(ctx, m, x, ldx, rows, row_map, y, ldy, nullptr, inc);
    return fail(CE_GPU_ENOTSUP, "incremental chunk: GEMM modes fp32, bf16x6 and bf16 only");
  }
  if (tap) {
    // calibration reads fp32 activations between the layers
    if (m->int8) return fail(CE_GPU_EINVAL, "model_calibrate: the model is already quantized");
    if (m->gemm == CE_GPU_GEMM_BF16X6 && ((x6_f32in() && x6_plane_chain_env() == 0) || has_row_steps(m)))
      return run_steps_x6f(ctx, m, x, ldx, rows, row_map, y, ldy, nullptr, tap);
    if (m->gemm == CE_GPU_GEMM_FP32) return run_steps_f32(ctx, m, x, ldx, rows, row_map, y, ldy, tap);
    return fail(CE_GPU_ENOTSUP, "model_calibrate: GEMM modes fp32 and bf16x6 only (the others keep activations as planes)");
  }
  if (m->int8 && m->int8_static) return run_steps_i8_static(ctx, m, x, ldx, rows, row_map, y, ldy);
  if (m->int8) return run_steps_i8(ctx, m, x, ldx, rows, row_map, row_edge, y, ldy);
  if (m->gemm == CE_GPU_GEMM_F16X3) return run_steps_chain16<ChainF16>(ctx, m, x, ldx, rows, row_map, y, ldy);
  if (m->gemm == CE_GPU_GEMM_BF16) return run_steps_chain16<ChainBf16>(ctx, m, x, ldx, rows, row_map, y, ldy);
  if (m->gemm == CE_GPU_GEMM_BF16X6_PLANES) return run_steps_chain16<ChainX6>(ctx, m, x, ldx, rows, row_map, y, ldy);
  if (m->gemm == CE_GPU_GEMM_BF16X6)
    return x6_f32in() || has_row_steps(m) ? run_steps_x6f(ctx, m, x, ldx, rows, row_map, y, ldy, tail)
                      : run_steps_chain16<ChainX6>(ctx, m, x, ldx, rows, row_map, y, ldy);
  return run_steps_f32(ctx, m, x, ldx, rows, row_map, y, ldy);
}

bool lat_tail_ok(const float *out, const float *log_prior) {
  return ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(log_prior)) & 15) == 0;
}

int finalize_output(ce_gpu_ctx *ctx, const float *y, int ldy, int first, int rows, int dim, bool log_softmax,
                    const float *log_prior, const int *row_dst, float *out, const LatTail &tail) {
  if (diag_skip() & 2) return CE_GPU_OK;
  if (tail.active) return launch_lat_finalize(ctx->stream, tail, first, rows, log_softmax, log_prior, row_dst, out);
  return launch_finalize(ctx->stream, y + (size_t)first * ldy, ldy, rows, dim, log_softmax, log_prior, row_dst,
                         out);
}

int score_packed_rows(ce_gpu_ctx *ctx, const ce_gpu_model *m, const float *feats, int rows, const int *row_src,
                      const uint32_t *row_edge, const int *row_dst, float *d_loglik, const IncrChunk *inc) {
  const float *y = nullptr;
  int ldy = 0;
  LatTail tail;
  CE_TRY(run_steps(ctx, m, feats, m->input_dim, rows, row_src, row_edge, &y, &ldy,
                   lat_tail_ok(d_loglik, m->log_prior.as<float>()) ? &tail : nullptr, nullptr, inc));
  ProfScope prof(ctx, CE_GPU_PROF_FINALIZE);
  return finalize_output(ctx, y, ldy, 0, rows, m->num_pdfs, m->final_log_softmax, m->log_prior.as<float>(), row_dst,
                         d_loglik, tail);
}

// The largest layout over the programs run_steps can dispatch to for this
// model, whatever GEMM mode it is switched to later, with latency mode on or
// off.  Every layout grows with the row count but the static int8 latency
// partials, whose slice rule depends on it: those take the largest over every
// count a later call may bring.
int reserve_packed_rows(ce_gpu_ctx *ctx, const ce_gpu_model *m, int rows) {
  if (m->int8 && !m->int8_static) return fail(CE_GPU_ENOTSUP, "reserve_packed_rows: int8 model");
  Layout all;
  if (m->int8_static) {
    cover(&all, layout_i8_static(m, rows, false));
    for (int r = 1; r <= std::min(rows, kI8LatMaxRows); ++r)
      all.lat_words = std::max(all.lat_words, layout_i8_static(m, r, true).lat_words);
    return ensure_layout(ctx, all);
  }
  cover(&all, layout_f32(m, rows));
  if (m->x6_ok) {
    cover(&all, layout_x6f(m, rows, true, false));
    cover(&all, layout_x6f(m, rows, false, x6f_planes_ok(m)));
    cover(&all, layout_chain16<ChainBf16>(m, rows));
    // the plane modes take no model with a row step
    if (!has_row_steps(m)) {
      cover(&all, layout_chain16<ChainX6>(m, rows));
      cover(&all, layout_chain16<ChainF16>(m, rows));
    }
  }
  return ensure_layout(ctx, all);
}

}  // namespace catears
