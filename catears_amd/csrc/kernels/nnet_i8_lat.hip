// nnet_i8_lat.hip -- latency mode of the static int8 GEMMs
// (ce_gpu_ctx_set_latency on a ce_gpu_model_quantize_static model): the
// streaming AcousticModel chunk or a session push, where the 256 x 128 tiles
// of gemm_i8_pipe_kernel leave most of the chip idle (70 rows on a 1024-wide
// layer: 8 blocks, each walking the whole K alone).
//
// The same contraction as the throughput kernel -- Splice folded into the A
// loader, sum a'b' on the shifted bytes -- with K split into S slices:
//
//   i8_lat_gemm_kernel    block (K slice, row tile of <= 96 rows, 64-column
//                         tile), one wave per 16 columns.  Every weight
//                         fragment of the slice is loaded up front, straight
//                         from I8Layer::wq into registers (wq is n x kpad,
//                         K contiguous: one lane's 16 K-bytes of a
//                         v_mfma_i32_16x16x64_i8 operand are one 16-byte
//                         load, so no fragment image is needed); the slice's
//                         activation bytes of the block's rows go through LDS
//                         once for the four waves, gathered through the
//                         splice offsets with row indices clamped to
//                         [0, m - 1]; the int32 partial tile is stored to
//                         part[s][row][col].
//   i8_lat_reduce_kernel  sums the S partials of each output in uint32, forms
//                         y with i8_ops.h's arithmetic (the throughput
//                         epilogues' own), and writes fp32 -- or, when the
//                         next step is a fusable Linear, that layer's shifted
//                         bytes and row sums (qbyte with its frozen
//                         parameters), as i8_epilogue_q does.
//
// The accumulators are integers modulo 2^32: any split of K and any order of
// the partial sums gives the same word, so the pair is bit-identical to the
// throughput kernel and the slice rule (i8_lat_plan) may depend on the row
// count.  The kernel boundary orders the partials for the reduce: no
// in-launch hand-off, no tickets, no fences.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "../i8_ops.h"
#include "../internal.h"

namespace catears {
namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kNW = 4;            // waves per block, 16 columns each
constexpr int kBN = 16 * kNW;     // columns per block
constexpr int kRT = 6;            // 16-row sub-tiles per block
constexpr int kBM = 16 * kRT;     // rows per block
constexpr int kMaxPer = 8;        // k-steps (of 64 bytes) per slice: all its weights in registers
constexpr int kMinPer = 2;
constexpr int kTarget = 256;      // blocks per launch the slice rule aims at: one per CU

struct LatArgs {
  const int8_t *a;   // quantized layer input, m x lda bytes
  int lda, m;
  int din, nseg;     // segment width (bytes) and count
  int off[8];
  const int8_t *w;   // shifted weights, n x kpad
  int n, kpad;
  int32_t *part;     // slices x m x ldp words
  int ldp;           // tiles_n * kBN
  int per, tiles_n, row_tiles;
};

template <int PER>
__global__ __launch_bounds__(64 * kNW) void i8_lat_gemm_kernel(LatArgs p) {
  constexpr int NT = 64 * kNW;
  constexpr int CPR = PER * 4;          // 16-byte chunks per staged row
  constexpr int ROWB = PER * 64 + 16;   // LDS row stride: 16 lanes' b128 reads of one k-step hit 64 distinct banks
  constexpr int ITER = kBM * CPR / NT;
  static_assert(ITER * NT == kBM * CPR, "staging loop covers the tile");
  __shared__ __attribute__((aligned(16))) int8_t As[kBM * ROWB];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  int b = blockIdx.x;
  const int tn = b % p.tiles_n;
  b /= p.tiles_n;
  const int tm = b % p.row_tiles, sl = b / p.row_tiles;
  const int ks0 = sl * p.per;
  const int nk = min(min(p.per, PER), p.kpad / 64 - ks0);  // >= 1: no slice is empty
  const int m0 = tm * kBM, n0 = tn * kBN;
  const int nsub = (min(kBM, p.m - m0) + 15) >> 4;

  // the slice's weight fragments, all in flight before anything else (columns
  // past n repeat column n - 1; the reduce never reads them)
  const int wcol = min(n0 + 16 * wave + r, p.n - 1);
  const int8_t *wp = p.w + (int64_t)wcol * p.kpad + 64 * ks0 + 16 * g;
  i32x4 wf[PER];
#pragma unroll
  for (int ks = 0; ks < PER; ++ks) wf[ks] = *reinterpret_cast<const i32x4 *>(wp + 64 * min(ks, nk - 1));

  // the block's rows of the slice through LDS, spliced: a 16-byte chunk lies
  // inside one segment (din % 128 == 0)
#pragma unroll
  for (int it = 0; it < ITER; ++it) {
    const int idx = tid + NT * it, row = idx / CPR, c = idx % CPR;
    if (row < 16 * nsub && c < 4 * nk) {
      const int k = 64 * ks0 + 16 * c;
      const int seg = k / p.din, kc = k - seg * p.din;
      int src = m0 + row + seg_off(p, seg);
      src = src < 0 ? 0 : (src > p.m - 1 ? p.m - 1 : src);
      i32x4 v = (i32x4){0, 0, 0, 0};
      if (seg < p.nseg) v = *reinterpret_cast<const i32x4 *>(p.a + (int64_t)src * p.lda + kc);
      *reinterpret_cast<i32x4 *>(As + row * ROWB + 16 * c) = v;
    }
  }
  __syncthreads();

  // weights as the A operand: lane (r, g) ends with columns 4g .. 4g + 3 of
  // the wave's 16 for row r of each sub-tile -- one 16-byte partial store
  i32x4 acc[kRT];
#pragma unroll
  for (int i = 0; i < kRT; ++i) acc[i] = (i32x4){0, 0, 0, 0};
#pragma unroll
  for (int ks = 0; ks < PER; ++ks) {
    if (ks < nk) {
#pragma unroll
      for (int i = 0; i < kRT; ++i) {
        if (i < nsub) {
          const i32x4 av = *reinterpret_cast<const i32x4 *>(As + (16 * i + r) * ROWB + 64 * ks + 16 * g);
          acc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wf[ks], av, acc[i], 0, 0, 0);
        }
      }
    }
  }
  int32_t *dst = p.part + (int64_t)sl * p.m * p.ldp + n0 + 16 * wave + 4 * g;
#pragma unroll
  for (int i = 0; i < kRT; ++i) {
    const int row = m0 + 16 * i + r;
    if (i < nsub && row < p.m) *reinterpret_cast<i32x4 *>(dst + (int64_t)row * p.ldp) = acc[i];
  }
}

struct LatReduceArgs {
  const int32_t *part;
  int ldp, slices, m, n, k;
  const int32_t *rowsum;   // per row of the layer input
  int nseg;
  int off[8];
  const int32_t *colsum;
  const void *pa;          // device QP of the activations
  float w_scale;
  int32_t w_zp;
  const float *bias, *bn_scale, *bn_offset;
  int post[4];
  int npost, post_mode;
  float *y;                // fp32 output (qy null)
  int ldy, vec;            // vec: 16-byte row stores
  // non-null: the next Linear's bytes (m x n) and row sums instead (I8NextBytes)
  int8_t *qy;
  int32_t *q_rowsum, *q_zero;
  const void *q_qp;
};

// One wave per (row, 256 columns): lane l sums the slices of columns 4l ..
// 4l + 3 (16-byte loads, 8 in flight), restores the zero points and writes
// four floats, or the next layer's four bytes and its share of the row sum.
__global__ __launch_bounds__(64) void i8_lat_reduce_kernel(LatReduceArgs p) {
  const int lane = threadIdx.x, row = blockIdx.y;
  const int col = 256 * blockIdx.x + 4 * lane;
  const bool live = col < p.n;
  const QP pa = *static_cast<const QP *>(p.pa);
  const I8Restore rc = i8_restore(pa, p.w_scale, p.w_zp, p.k);
  // columns past n: the tile's padding up to ldp is there to be read
  const int32_t *src = p.part + (int64_t)row * p.ldp + min(col, p.ldp - 4);
  const int64_t stride = (int64_t)p.m * p.ldp;
  uint32_t sum[4] = {0, 0, 0, 0};
  for (int s0 = 0; s0 < p.slices; s0 += 8) {
    i32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const i32x4 *>(src + min(s0 + u, p.slices - 1) * stride);
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (s0 + u < p.slices) {
#pragma unroll
        for (int e = 0; e < 4; ++e) sum[e] += (uint32_t)v[u][e];
      }
  }
  const uint32_t rterm = rc.cb * i8_spliced_rowsum(p.rowsum, row, p.m, p.nseg, p.off);
  float y[4];
  with_post_mode(p.post_mode, [&](auto M) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = min(col + e, p.n - 1);
      y[e] = i8_output<decltype(M)::value>(sum[e], rterm, i8_cterm(rc, p.colsum[c]), rc.cscale,
                                           p.bias ? p.bias[c] : 0.0f, p.bn_scale ? p.bn_scale[c] : 1.0f,
                                           p.bn_offset ? p.bn_offset[c] : 0.0f, p.post, p.npost);
    }
  });
  if (p.qy) {  // n % 128 == 0: a live lane's four columns exist
    const QP pn = *static_cast<const QP *>(p.q_qp);
    const float nzp = (float)pn.zp, nrs = qbyte_rscale(pn.scale);
    int bsum = 0;
    if (live) {
      int q[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        q[e] = qbyte(y[e], pn.scale, nzp, nrs);
        bsum += q[e];
      }
      *reinterpret_cast<uint32_t *>(p.qy + (int64_t)row * p.n + col) = i8_pack4(q[0], q[1], q[2], q[3]);
    }
    i8_rowsum_group_add<64>(bsum, true, p.q_rowsum + row);
    if (blockIdx.x == 0 && lane == 0 && p.q_zero) p.q_zero[row] = 0;  // for the launch after this one
    return;
  }
  if (!live) return;
  float *o = p.y + (int64_t)row * p.ldy + col;
  if (p.vec) {
    *reinterpret_cast<float4 *>(o) = make_float4(y[0], y[1], y[2], y[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (col + e < p.n) o[e] = y[e];
  }
}

std::atomic<int64_t> g_lat_launches{0};

}  // namespace

void i8_lat_plan(int kpad, int n, int rows, int *slices, int *per) {
  *slices = 0;
  *per = 0;
  // CATEARS_I8_LAT_MAXROWS (experiments library only): the crossover sweep of
  // tools/latency.py --static-int8 runs the pair at every row count
  static const int max_rows = CE_KNOB("CATEARS_I8_LAT_MAXROWS", kI8LatMaxRows);
  if (kpad <= 0 || n <= 0 || rows <= 0 || kpad % 128 != 0 || rows > max_rows) return;
  const int ksteps = kpad / 64;
  const int tiles = ((rows + kBM - 1) / kBM) * ((n + kBN - 1) / kBN);
  const int want = std::max(1, std::min(ksteps, kTarget / tiles));
  const int p = std::min(kMaxPer, std::max(kMinPer, (ksteps + want - 1) / want));
  *slices = (ksteps + p - 1) / p;  // no empty slice
  *per = p;
}

size_t i8_lat_part_words(int rows, int n, int slices) {
  return (size_t)slices * (size_t)rows * (size_t)((n + kBN - 1) / kBN * kBN);
}

bool i8_lat_eligible(const I8Layer &L, int lda) {
  return L.kpad % 128 == 0 && L.a_din % 128 == 0 && lda % 16 == 0 && L.a_nseg >= 1 && L.a_nseg <= 8 &&
         L.a_nseg * L.a_din <= L.kpad && L.a_din <= lda;
}

int64_t i8_lat_launch_count() { return g_lat_launches.load(std::memory_order_relaxed); }

int launch_i8_lat(hipStream_t s, const I8Layer &L, const int8_t *a, int lda, int m, const int32_t *rowsum,
                  const void *pa, float *y, int ldy, const I8NextBytes *nb, int32_t *part, size_t part_words,
                  int off_shift) {
  if (m <= 0) return CE_GPU_OK;
  int slices = 0, per = 0;
  i8_lat_plan(L.kpad, L.n, m, &slices, &per);
  if (slices == 0 || !i8_lat_eligible(L, lda))
    return fail(CE_GPU_EINVAL, "int8 latency GEMM: layer geometry or row count not eligible");
  if (nb && !i8_gemm_can_requantize(L, lda))
    return fail(CE_GPU_EINVAL, "int8 latency GEMM: no requantize output for this layer");
  if (!part || part_words < i8_lat_part_words(m, L.n, slices))
    return fail(CE_GPU_EINVAL, "int8 latency GEMM: partial workspace too small");
  if ((reinterpret_cast<uintptr_t>(a) & 15) || (reinterpret_cast<uintptr_t>(L.wq.ptr) & 15) ||
      (reinterpret_cast<uintptr_t>(part) & 15))
    return fail(CE_GPU_EINVAL, "int8 latency GEMM: operands must be 16-byte aligned");
  LatArgs g = {};
  g.a = a;
  g.lda = lda;
  g.m = m;
  g.din = L.a_din;
  g.nseg = L.a_nseg;
  for (int i = 0; i < 8; ++i) g.off[i] = i < L.a_nseg ? L.a_off[i] - off_shift : 0;
  g.w = L.wq.as<int8_t>();
  g.n = L.n;
  g.kpad = L.kpad;
  g.part = part;
  g.tiles_n = (L.n + kBN - 1) / kBN;
  g.ldp = g.tiles_n * kBN;
  g.per = per;
  g.row_tiles = (m + kBM - 1) / kBM;
  const dim3 grid(slices * g.row_tiles * g.tiles_n), block(64 * kNW);
  // the block sized for the slice (its weights all in registers)
  if (per <= 2)
    hipLaunchKernelGGL(i8_lat_gemm_kernel<2>, grid, block, 0, s, g);
  else if (per <= 4)
    hipLaunchKernelGGL(i8_lat_gemm_kernel<4>, grid, block, 0, s, g);
  else
    hipLaunchKernelGGL(i8_lat_gemm_kernel<8>, grid, block, 0, s, g);
  g_lat_launches.fetch_add(1, std::memory_order_relaxed);

  LatReduceArgs r = {};
  r.part = part;
  r.ldp = g.ldp;
  r.slices = slices;
  r.m = m;
  r.n = L.n;
  r.k = L.k;
  r.rowsum = rowsum;
  r.nseg = L.a_nseg;
  for (int i = 0; i < 8; ++i) r.off[i] = i < L.a_nseg ? L.a_off[i] - off_shift : 0;
  r.colsum = L.colsum.as<int32_t>();
  r.pa = pa;
  r.w_scale = L.w_scale;
  r.w_zp = L.w_zp;
  r.bias = L.bias;
  r.bn_scale = L.bn_scale;
  r.bn_offset = L.bn_offset;
  for (int i = 0; i < 4; ++i) r.post[i] = L.post[i];
  r.npost = L.npost;
  r.post_mode = post_mode(L.post, L.npost);
  if (nb) {
    r.qy = nb->xq;
    r.q_rowsum = nb->rowsum;
    r.q_zero = nb->zero;
    r.q_qp = nb->qp;
  } else {
    r.y = y;
    r.ldy = ldy;
    r.vec = L.n % 4 == 0 && ldy % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
  }
  hipLaunchKernelGGL(i8_lat_reduce_kernel, dim3((L.n + 255) / 256, m), dim3(64), 0, s, r);
  CE_HIP(hipGetLastError());
  return CE_GPU_OK;
}

}  // namespace catears
