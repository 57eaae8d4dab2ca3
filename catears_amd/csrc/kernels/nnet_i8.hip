// nnet_i8.hip -- the int8 nnet path (BASELINE config C5): every LinearLayer
// as Quantize + MatMat_U8U8F32 + bias (src/matrix.cc:329-420, the pieces the
// reference ships but never wires into Nnet, src/nnet.cc:29).
//
// Per layer and per chunk of packed rows:
//   1. minmax_kernel     min / max over the layer input X (rows x width; the
//      params_kernel     first layer reads its rows through row_map): block
//                        partials, then one block folds them, both seeded
//                        with FLT_MAX and FLT_MIN exactly like FindMinMax
//                        (matrix.cc:331-345: max starts at FLT_MIN), and
//                        applies ComputeQuantizationParams (matrix.cc:348-362).
//                        Only rows the reference chain still holds count: the
//                        packed buffers keep full height, so the edge rows the
//                        earlier Narrows dropped (computed from clamped
//                        indices) are skipped by their distance to the
//                        segment edges.  Layers whose input is the previous
//                        GEMM's output skip minmax_kernel: that GEMM's
//                        epilogue leaves per-wave partials (I8Args::mm_part).
//   2. quantize_kernel   q = roundf(clamp(x / scale + zp, 0, 255)) stored as the
//                        signed byte q ^ 0x80 = q - 128, with the row sums of
//                        those bytes.  Layers whose segment width is not a
//                        multiple of the 128-byte K-tile (the 40-wide first layer)
//                        are written already spliced (rows x K, zero padded).
//   3. gemm_i8_nnet      v_mfma_i32_32x32x32_i8 on the shifted bytes with the
//                        splice folded into the A loader; int32 epilogue
//                        restores the zero points,
//                          sum (a-zA)(b-zB) = sum a'b' + cB*rowsum(a') + cA*colsum(b') + K*cA*cB
//                        (cA = 128 - zA), all modulo 2^32 like gemmlowp's
//                        accumulator, then float(acc) * (sA*sB) + bias, ReLU /
//                        BatchNorm in the reference's rounding order.
// Quantising the block entering the Splice is the same as quantising the
// spliced block: the tensor parameters depend only on min / max, and Splice +
// Narrow read every held row of the block.
//
// Static int8 (ce_gpu_model_quantize_static): step 1 never runs -- every
// layer's parameters are the model's frozen ones -- and where a GEMM's output
// is the next layer's plain operand, step 2 moves into that GEMM's epilogue
// (i8_epilogue_q: the next layer's bytes and row sums instead of fp32
// outputs).  ce_gpu_model_calibrate uses step 1's two kernels on the fp32
// programs' activations to measure the ranges (launch_i8_range).
//
// This file is what the product library runs: steps 1 and 2, and
// launch_i8_gemm over the one GEMM kernel, gemm_i8_pipe_kernel of
// ../nnet_i8_kernels.h (with the epilogues).  The other GEMM kernels and
// tiles -- measured, bit-identical alternatives and the ablations -- are in
// nnet_i8_exp.hip, compiled into the experiments library only.
#include <math.h>
#include <stdlib.h>

#include "../nnet_i8_kernels.h"

namespace catears {
namespace {

// One wave per row (grid-stride over rows); rows outside what the reference
// chain holds at this layer (segment edges already narrowed away) are skipped.
// Each block leaves one (min, max) partial; params_kernel folds them.
constexpr int kMinmaxBlocks = 512;

__global__ __launch_bounds__(256) void minmax_kernel(const float *__restrict__ x, int ldx, int rows, int width,
                                                     const int *__restrict__ row_map,
                                                     const uint32_t *__restrict__ row_edge, int in_left,
                                                     int in_right, float2 *__restrict__ part) {
  float mn = FLT_MAX, mx = FLT_MIN;
  const int lane = threadIdx.x & 63;
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += gridDim.x * 4) {
    const int dl = row_edge ? (int)(row_edge[r] & 0xffff) : r;
    const int dr = row_edge ? (int)(row_edge[r] >> 16) : rows - 1 - r;
    if (dl < in_left || dr < in_right) continue;
    const int src = row_map ? row_map[r] : r;
    const float *xr = x + (int64_t)src * ldx;
    // float4 rows: also a base on 16 bytes (a caller's block may start at any float)
    if ((width & 3) == 0 && (ldx & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
      for (int c = 4 * lane; c < width; c += 256) {
        const float4 v = *reinterpret_cast<const float4 *>(xr + c);
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (e[t] > mx) mx = e[t];  // matrix.cc:337-342 (NaN never wins a comparison)
          if (e[t] < mn) mn = e[t];
        }
      }
    } else {
      for (int c = lane; c < width; c += 64) {
        const float v = xr[c];
        if (v > mx) mx = v;
        if (v < mn) mn = v;
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float omn = __shfl_xor(mn, d, 64), omx = __shfl_xor(mx, d, 64);
    mn = omn < mn ? omn : mn;
    mx = omx > mx ? omx : mx;
  }
  __shared__ float2 wv[4];
  if (lane == 0) wv[threadIdx.x >> 6] = make_float2(mn, mx);
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      mn = wv[w].x < mn ? wv[w].x : mn;
      mx = wv[w].y > mx ? wv[w].y : mx;
    }
    part[blockIdx.x] = make_float2(mn, mx);
  }
}

// ComputeQuantizationParams (matrix.cc:348-362) of a folded (min, max)
__device__ __forceinline__ QP qparams(float mn, float mx) {
  const double scale = (mx - mn) / 255.0;
  QP p;
  p.zp = (int32_t)round(-mn / scale);
  p.scale = (float)scale;
  return p;
}

// Folds the block partials and applies ComputeQuantizationParams
// (matrix.cc:348-362, double arithmetic) -- one block.  Calibration
// (ce_gpu_model_calibrate) passes `range` instead of `out`: the fold then
// takes in the (min, max) already there and leaves the result in its place,
// so one Linear's range accumulates over chunks and calls.
__global__ __launch_bounds__(256) void params_kernel(const float2 *__restrict__ part, int nparts,
                                                     QP *__restrict__ out, float2 *__restrict__ range) {
  float mn = FLT_MAX, mx = FLT_MIN;
  for (int i = threadIdx.x; i < nparts; i += 256) {
    mn = part[i].x < mn ? part[i].x : mn;
    mx = part[i].y > mx ? part[i].y : mx;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float omn = __shfl_xor(mn, d, 64), omx = __shfl_xor(mx, d, 64);
    mn = omn < mn ? omn : mn;
    mx = omx > mx ? omx : mx;
  }
  __shared__ float2 wv[4];
  if ((threadIdx.x & 63) == 0) wv[threadIdx.x >> 6] = make_float2(mn, mx);
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      mn = wv[w].x < mn ? wv[w].x : mn;
      mx = wv[w].y > mx ? wv[w].y : mx;
    }
    if (range) {
      mn = range->x < mn ? range->x : mn;
      mx = range->y > mx ? range->y : mx;
      *range = make_float2(mn, mx);
    }
    if (out) *out = qparams(mn, mx);
  }
}

// One wave per output row.  Plain mode: out row r = quantized X row
// (row_map[r] or r), width bytes, zero padded to ldq.  Spliced mode (nseg >
// 1 or width % 64): out row r = concat over segments s of quantized
// X[clamp(r + off[s])] (through row_map), zero padded to ldq.
struct SpliceOffsets {
  int off[8];
};

// Quantize row r of the layer input into q row r (one wave; lane = lane in
// the wave), and its row sum.
__device__ __forceinline__ void quantize_row(const float *__restrict__ x, int ldx, int rows, int width,
                                             const int *__restrict__ row_map, int nseg, const SpliceOffsets &so,
                                             float scale, float zp, int8_t *__restrict__ q, int ldq,
                                             int32_t *__restrict__ rowsum, int r, int lane) {
  int8_t *o = q + (int64_t)r * ldq;
  int32_t s = 0;
  const float rs = qbyte_rscale(scale);
  const bool vec = (width & 3) == 0 && (ldx & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  for (int seg = 0; seg < nseg; ++seg) {
    int src = r + so.off[seg];
    src = src < 0 ? 0 : (src > rows - 1 ? rows - 1 : src);
    if (row_map) src = row_map[src];
    const float *xr = x + (int64_t)src * ldx;
    int8_t *os = o + seg * width;
    if (vec) {
      // 1024 floats of the row per pass, the lane's four float4 loads issued
      // together (clamped addresses, used only in range): one memory round
      // trip per pass instead of one per float4
      for (int c0 = 0; c0 < width; c0 += 1024) {
        float4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          v[j] = *reinterpret_cast<const float4 *>(xr + min(c0 + 4 * lane + 256 * j, width - 4));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = c0 + 4 * lane + 256 * j;
          if (c >= width) break;
          const int b0 = qbyte(v[j].x, scale, zp, rs), b1 = qbyte(v[j].y, scale, zp, rs);
          const int b2 = qbyte(v[j].z, scale, zp, rs), b3 = qbyte(v[j].w, scale, zp, rs);
          s += b0 + b1 + b2 + b3;
          const uint32_t packed = i8_pack4(b0, b1, b2, b3);
          if ((((uintptr_t)(os + c)) & 3) == 0) {
            *reinterpret_cast<uint32_t *>(os + c) = packed;
          } else {
            os[c] = (int8_t)b0, os[c + 1] = (int8_t)b1, os[c + 2] = (int8_t)b2, os[c + 3] = (int8_t)b3;
          }
        }
      }
    } else {
      for (int c = lane; c < width; c += 64) {
        const int b = qbyte(xr[c], scale, zp, rs);
        os[c] = (int8_t)b;
        s += b;
      }
    }
  }
  for (int c = nseg * width + lane; c < ldq; c += 64) o[c] = 0;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if (lane == 0) rowsum[r] = s;
}

// The vector path of quantize_row for RPW rows per wave (plain mode: one
// segment, width and ldx multiples of 4, no row map): every row's loads are
// issued before any is converted, and the reciprocal product's rare fallback
// (a non-finite quotient, qbyte) is one wave-level branch per row instead of
// one per element: the quotients are formed for the whole row, and only if
// some lane holds a non-finite one are those recomputed by division.  The
// same arithmetic per element as qbyte: the same bytes and row sums.
template <int RPW>
__device__ __forceinline__ void quantize_rows_fast(const float *__restrict__ x, int ldx, int rows, int width,
                                                   float scale, float zp, int8_t *__restrict__ q, int ldq,
                                                   int32_t *__restrict__ rowsum, int r0, int lane) {
  const float rs = qbyte_rscale(scale);
  const bool rs_ok = rs != 0.0f;  // 0: the division for every element, as qbyte
  int32_t rsum[RPW];
#pragma unroll
  for (int i = 0; i < RPW; ++i) rsum[i] = 0;
  for (int c0 = 0; c0 < width; c0 += 1024) {
    float4 v[RPW][4];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const float *xr = x + (int64_t)min(r0 + i, rows - 1) * ldx;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        v[i][j] = *reinterpret_cast<const float4 *>(xr + min(c0 + 4 * lane + 256 * j, width - 4));
    }
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      if (r0 + i >= rows) break;
      float qv[16];
      bool bad = !rs_ok;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float e[4] = {v[i][j].x, v[i][j].y, v[i][j].z, v[i][j].w};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float q0 = e[t] * rs;
          const float qq = __builtin_fmaf(__builtin_fmaf(-scale, q0, e[t]), rs, q0);
          bad |= __builtin_isinf(qq) || __builtin_isnan(qq);
          qv[4 * j + t] = qq;
        }
      }
      if (__builtin_amdgcn_ballot_w64(bad)) {  // rare: the division, exactly as qbyte
        if (bad) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float e[4] = {v[i][j].x, v[i][j].y, v[i][j].z, v[i][j].w};
#pragma unroll
            for (int t = 0; t < 4; ++t)
              if (!rs_ok || __builtin_isinf(qv[4 * j + t]) || __builtin_isnan(qv[4 * j + t])) qv[4 * j + t] = e[t] / scale;
          }
        }
      }
      int8_t *os = q + (int64_t)(r0 + i) * ldq;
      int32_t &sum = rsum[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = c0 + 4 * lane + 256 * j;
        if (c >= width) break;
        int b[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          float w = qv[4 * j + t] + zp;
          w = (255.0f < w) ? 255.0f : w;
          w = (0.0f < w) ? w : 0.0f;
          b[t] = (int)(uint8_t)roundf(w) - 128;
          sum += b[t];
        }
        const uint32_t packed = i8_pack4(b[0], b[1], b[2], b[3]);
        *reinterpret_cast<uint32_t *>(os + c) = packed;
      }
    }
  }
  // the row sums (exact int32: any order)
#pragma unroll
  for (int i = 0; i < RPW; ++i) {
    int32_t sum = rsum[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0 && r0 + i < rows) rowsum[r0 + i] = sum;
  }
  // zero padding past the row (ldq > width)
#pragma unroll
  for (int i = 0; i < RPW; ++i) {
    if (r0 + i >= rows) break;
    int8_t *o = q + (int64_t)(r0 + i) * ldq;
    for (int c = width + lane; c < ldq; c += 64) o[c] = 0;
  }
}

template <int RPW>
__global__ __launch_bounds__(256) void quantize_fast_kernel(const float *__restrict__ x, int ldx, int rows, int width,
                                                            const QP *__restrict__ params, int8_t *__restrict__ q,
                                                            int ldq, int32_t *__restrict__ rowsum,
                                                            int32_t *__restrict__ zero) {
  const QP p = *params;
  const int r0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW, lane = threadIdx.x & 63;
  if (r0 >= rows) return;
  if (zero && lane < RPW && r0 + lane < rows) zero[r0 + lane] = 0;
  quantize_rows_fast<RPW>(x, ldx, rows, width, p.scale, (float)p.zp, q, ldq, rowsum, r0, lane);
}

__global__ __launch_bounds__(256) void quantize_kernel(const float *__restrict__ x, int ldx, int rows, int width,
                                                       const int *__restrict__ row_map, int nseg,
                                                       SpliceOffsets so, const QP *__restrict__ params,
                                                       int8_t *__restrict__ q, int ldq, int32_t *__restrict__ rowsum,
                                                       int32_t *__restrict__ zero) {
  const QP p = *params;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  if (zero && lane == 0) zero[r] = 0;
  quantize_row(x, ldx, rows, width, row_map, nseg, so, p.scale, (float)p.zp, q, ldq, rowsum, r, lane);
}

// minmax_kernel over the held rows of a layer input: its partials in `part`
// (kMinmaxBlocks float2 at most); returns their count.
int launch_minmax(hipStream_t s, const float *x, int ldx, int rows, int width, const int *row_map,
                  const uint32_t *row_edge, int in_left, int in_right, void *part) {
  const int blocks = std::max(1, std::min(kMinmaxBlocks, (rows + 3) / 4));
  hipLaunchKernelGGL(minmax_kernel, dim3(blocks), dim3(256), 0, s, x, ldx, rows, width, row_map, row_edge, in_left,
                     in_right, static_cast<float2 *>(part));
  return blocks;
}

// params_kernel over `nparts` partials: the parameters to *params, or the
// range folded into range[0..1]
int launch_fold(hipStream_t s, const void *part, int nparts, QP *params, float2 *range) {
  hipLaunchKernelGGL(params_kernel, dim3(1), dim3(256), 0, s, static_cast<const float2 *>(part), nparts, params, range);
  CE_HIP(hipGetLastError());
  return CE_GPU_OK;
}

}  // namespace

// Reduces the held rows of a layer input to QP params.
int launch_i8_params(hipStream_t s, const float *x, int ldx, int rows, int width, const int *row_map,
                     const uint32_t *row_edge, int in_left, int in_right, void *part, void *params) {
  const int nparts = launch_minmax(s, x, ldx, rows, width, row_map, row_edge, in_left, in_right, part);
  return launch_fold(s, part, nparts, static_cast<QP *>(params), nullptr);
}

// Calibration: folds the (min, max) of the held rows of a layer input into
// range[0..1] (device).
int launch_i8_range(hipStream_t s, const float *x, int ldx, int rows, int width, const int *row_map,
                    const uint32_t *row_edge, int in_left, int in_right, void *part, float *range) {
  const int nparts = launch_minmax(s, x, ldx, rows, width, row_map, row_edge, in_left, in_right, part);
  return launch_fold(s, part, nparts, nullptr, reinterpret_cast<float2 *>(range));
}

// The same fold of the partials that a GEMM's epilogue left (I8NextMinMax).
int launch_i8_params_fold(hipStream_t s, const void *part, int nparts, void *params) {
  return launch_fold(s, part, nparts, static_cast<QP *>(params), nullptr);
}

size_t i8_params_scratch_bytes() { return sizeof(float2) * kMinmaxBlocks + 256; }

int launch_i8_quantize(hipStream_t s, const float *x, int ldx, int rows, int width, const int *row_map, int nseg,
                       const int *offs, const void *params, int8_t *q, int ldq, int32_t *rowsum, int32_t *zero) {
  SpliceOffsets so = {};
  for (int i = 0; i < nseg; ++i) so.off[i] = offs[i];
  // Plain-mode layers (every layer after the first) go through
  // quantize_fast_kernel: one wave-level fallback branch per row instead of
  // one per element, same bytes and row sums; C5 +3.0 % (24.29 vs 23.58 M
  // frames/s, A B C C B A x2 on one box, same checksum,
  // profiles/r06k_c5_quantize.txt; two rows per wave: +2.1 %, removed).
  // CATEARS_I8_QFAST=0 (experiments library): quantize_kernel for these too.
  static const int qfast = CE_KNOB("CATEARS_I8_QFAST", 1);
  const bool plain = nseg == 1 && !row_map && so.off[0] == 0 && width % 4 == 0 && ldx % 4 == 0 && ldq % 4 == 0 &&
                     (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(q) & 3) == 0;
  if (rows > 0 && plain && qfast == 1) {
    hipLaunchKernelGGL(quantize_fast_kernel<1>, dim3((rows + 3) / 4), dim3(256), 0, s, x, ldx, rows, width,
                       static_cast<const QP *>(params), q, ldq, rowsum, zero);
  } else if (rows > 0)
    hipLaunchKernelGGL(quantize_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, ldx, rows, width, row_map, nseg,
                       so, static_cast<const QP *>(params), q, ldq, rowsum, zero);
  CE_HIP(hipGetLastError());
  return CE_GPU_OK;
}

// The product's tile: 256 x 128, 8 waves of 64 x 64, K-tiles of 128 bytes,
// three stages (144 KiB of LDS) -- measured best on TDNN-S, frame batch 8192
// (tools/i8_sweep.sh)
using ProductTile = I8Tile<256, 128, 4, 2>;
static_assert(ProductTile::BM % kI8MinTile == 0 && ProductTile::BN == kI8MinTile && ProductTile::NW == kI8MaxWaves,
              "i8_gemm_parts counts the product tile's partials");

// K (weights' kpad, and with it every activation row) is padded to the
// product tile's K-tile, bytes
int i8_k_align() { return ProductTile::BKB; }

// The (min, max) partials of a GEMM's epilogue, one per wave: at most the
// product tile's 8 on each 128 x 128 outputs (no tile of the experiments
// library is smaller or has more waves: i8_launch's static_assert)
size_t i8_gemm_parts(int m, int n) {
  return (size_t)((m + kI8MinTile - 1) / kI8MinTile) * ((n + kI8MinTile - 1) / kI8MinTile) * kI8MaxWaves;
}

// The requantize epilogue (I8NextBytes) is gemm_i8_pipe_kernel's, for whole
// column tiles; launch_i8_gemm's K geometry besides.
bool i8_gemm_can_requantize(const I8Layer &L, int lda) {
#ifdef CATEARS_EXPERIMENTS
  if (i8_gemm_variant() != 16 && i8_gemm_variant() != 17) return false;  // the other kernels have none
#endif
  return L.n % 128 == 0 && L.kpad % 128 == 0 && L.a_din % 128 == 0 && lda % 16 == 0;
}

int launch_i8_gemm(hipStream_t s, const I8Layer &L, const int8_t *a, int lda, int m, const int32_t *rowsum,
                   const void *pa, float *y, int ldy, const I8NextMinMax *mm, int *nparts, const I8NextBytes *nb,
                   int off_shift) {
  if (nb && !i8_gemm_can_requantize(L, lda))
    return fail(CE_GPU_EINVAL, "int8 GEMM: no requantize epilogue for this layer");
  // what quantize_weights and the nnet programs always provide (K padded to
  // i8_k_align, narrower segments spliced by the Quantize step)
  if (L.kpad % 128 != 0 || L.a_din % 128 != 0 || lda % 16 != 0)
    return fail(CE_GPU_EINVAL, "int8 GEMM: needs kpad % 128 == 0, segment width % 128 == 0 and lda % 16 == 0");
#ifdef CATEARS_EXPERIMENTS
  if (i8_gemm_variant() != 16)  // nnet_i8_exp.hip's table
    return launch_i8_gemm_exp(s, L, a, lda, m, rowsum, pa, y, ldy, mm, nparts, nb, off_shift);
#endif
  const I8Args p = i8_args(L, a, lda, m, rowsum, pa, y, ldy, mm, nb, off_shift);
  return i8_launch<ProductTile>(s, gemm_i8_pipe_kernel<256, 128, 3, 4, 2>, p, nparts);
}

}  // namespace catears
