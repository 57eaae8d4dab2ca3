// nnet_i8_kernels.h -- the device side that the int8 GEMM's two translation
// units both instantiate: kernels/nnet_i8.hip (what the product runs; the
// scheme is described there) and kernels/nnet_i8_exp.hip (the experiments
// library's other kernels and tiles).  The kernel arguments, the tile
// geometry with its loader addressing, the three epilogues, the product's
// kernel gemm_i8_pipe_kernel, the launch helper and the I8Layer -> I8Args
// fill.  Everything is in the unnamed namespace: each translation unit
// compiles its own instantiations.
#pragma once

#include <float.h>
#include <hip/hip_runtime.h>

#include "i8_ops.h"
#include "internal.h"
#include "lds_dma.h"
#include "tile_order.h"

namespace catears {

// kernels/nnet_i8_exp.hip, the experiments library only: CATEARS_I8_GEMM
// (16 is the product's kernel) and the dispatcher of its other values, for
// arguments launch_i8_gemm has checked.
int i8_gemm_variant();
int launch_i8_gemm_exp(hipStream_t s, const I8Layer &L, const int8_t *a, int lda, int m, const int32_t *rowsum,
                       const void *pa, float *y, int ldy, const I8NextMinMax *mm, int *nparts, const I8NextBytes *nb,
                       int off_shift);

// Every int8 GEMM tile covers at least kI8MinTile x kI8MinTile outputs with
// at most kI8MaxWaves waves (i8_launch asserts it of each tile it launches):
// what i8_gemm_parts sizes the per-wave (min, max) partials by.
constexpr int kI8MinTile = 128, kI8MaxWaves = 8;

namespace {

using dma::buf_lds16;
using dma::buf_rsrc;

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

struct I8Args {
  const int8_t *a;          // quantized layer input (rows x lda bytes)
  int lda, m;
  int din, nseg;            // segment width (bytes) and count; K = din * nseg
  int off[8];
  const int32_t *rowsum;    // per row of `a`
  const int8_t *w;          // shifted weights, n x kpad
  const int32_t *colsum;    // per column of w (shifted bytes)
  int n, k, kpad;
  const void *pa;           // device QP of the activations
  float w_scale;
  int32_t w_zp;
  const float *bias, *bn_scale, *bn_offset;
  int post[4];
  int npost, post_mode;
  float *y;
  int ldy;
  int tiles_n, tiles_m, group;
  int vec_epi;              // i8_epilogue_v (16-byte row stores)
  // Non-null: the epilogue also reduces the (min, max) of its outputs over the
  // rows the NEXT layer's Quantize reads (minmax_kernel's held-row rule with
  // that layer's in_left / in_right) into mm_part[blockIdx.x], so the next
  // layer's parameters fold these partials instead of re-reading the output.
  float2 *mm_part;
  const uint32_t *row_edge;
  int mm_left, mm_right;
  // Non-null (static int8, n % 128 == 0): no fp32 output; the epilogue writes
  // the next layer's shifted bytes (its frozen parameters *q_qp) to qy
  // (m x n) and adds their row sums into q_rowsum (I8NextBytes, internal.h)
  int8_t *qy;
  int32_t *q_rowsum, *q_zero;
  const void *q_qp;
};

// The block tile of the LDS-DMA kernels: BM x BN outputs, WGM x WGN waves of
// (TI x 32) x (TJ x 32), K-tiles of BKB bytes per row.  One DMA instruction
// (a piece) moves 1 KiB = RPI tile rows of CH 16-byte chunks; the stage holds
// the A tile's pieces, then the B tile's, each wave issuing NGA + NGB of
// them.  Bank spread: chunk c of tile row `row` is stored at chunk c ^
// swz(row), applied on the source address.  A 32x32x32 i8 MFMA operand is
// one ds_read_b128 per lane (row r, bytes 16h .. 16h + 15 of its 32-byte
// k-step), so a tile row of 128 bytes holds the four k-steps of the tile.
template <int BM_, int BN_, int WGM, int WGN, int BKB_ = 128>
struct I8Tile {
  static constexpr int BM = BM_, BN = BN_, BKB = BKB_;
  static constexpr int NW = WGM * WGN, NT = 64 * NW;
  static constexpr int CH = BKB / 16;     // 16-byte chunks per row
  static constexpr int TI = BM / WGM / 32, TJ = BN / WGN / 32;
  static constexpr int RPI = 1024 / BKB;  // rows per DMA instruction
  static constexpr int NGA = BM * BKB / 1024 / NW, NGB = BN * BKB / 1024 / NW, NG = NGA + NGB;
  static constexpr int STAGE = (BM + BN) * BKB;  // bytes
  static_assert(NGA >= 1 && NGB >= 1 && TI >= 1 && TJ >= 1, "tile too small");
  static_assert(BKB == 128 || BKB == 64, "K-tile of 64 or 128 bytes");

  static __device__ __forceinline__ int swz(int row) { return (row >> 1) & (CH - 1); }
  // A lane's 16 bytes of a piece are chunk lchunk = lane % CH of the piece's
  // row lrow = lane / CH: the tile row, and the source byte offset inside the
  // row's K-tile
  static __device__ __forceinline__ int dma_row(int piece, int lrow) { return piece * RPI + lrow; }
  static __device__ __forceinline__ int dma_byte(int row, int lchunk) { return 16 * (lchunk ^ swz(row)); }
};

// minmax_kernel's row rule: does the next layer's Quantize count row `row`?
__device__ __forceinline__ uint32_t mm_held(const uint32_t *row_edge, int m, int left, int right, int row) {
  if (row >= m) return 0;
  const int dl = row_edge ? (int)(row_edge[row] & 0xffff) : row;
  const int dr = row_edge ? (int)(row_edge[row] >> 16) : m - 1 - row;
  return dl >= left && dr >= right;
}

// FindMinMax's comparisons (matrix.cc:337-342: NaN never wins one)
__device__ __forceinline__ void mm_take(float y, float &mn, float &mx) {
  if (y > mx) mx = y;
  if (y < mn) mn = y;
}

// Wave (min, max) of the epilogue's held outputs -> part[blockIdx.x * NW +
// wave] (no block barrier: a barrier under the epilogue's runtime `mm` test
// made the compiler copy the whole argument struct to scratch memory).
template <int NT>
__device__ __forceinline__ void mm_store(float2 *part, float mn, float mx) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float omn = __shfl_xor(mn, d, 64), omx = __shfl_xor(mx, d, 64);
    mn = omn < mn ? omn : mn;
    mx = omx > mx ? omx : mx;
  }
  if ((threadIdx.x & 63) == 0) part[blockIdx.x * (NT / 64) + (threadIdx.x >> 6)] = make_float2(mn, mx);
}

// Zero-point restore + bias + ReLU / BatchNorm + store of one wave's
// (TI x 32) x (TJ x 32) accumulator tile at (m0 + wrow, col0).  Column
// constants are read once into registers (the output stores could alias them
// as far as the compiler knows, so reads inside the store loop reload after
// every store) and the spliced row sums once per block row into LDS (`srs`,
// BM words; a per-lane loop over rows x segments is a chain of dependent L2
// round trips).  Every thread of the block must call it.
template <int TI, int TJ, int BM, int NT>
__device__ __forceinline__ void i8_epilogue(const I8Args &p, const i32x16 (&acc)[TI][TJ], int m0, int wrow, int col0,
                                            int r, int h, uint32_t *srs) {
  const QP pa = *static_cast<const QP *>(p.pa);
  const I8Restore rc = i8_restore(pa, p.w_scale, p.w_zp, p.k);
  // cB * row sum of each spliced row of the block, one row per thread, into
  // LDS (the operand buffers are free once every wave is past the loop)
  __syncthreads();
  for (int t = threadIdx.x; t < BM; t += NT) {
    const int row = m0 + t;
    srs[t] = rc.cb * i8_spliced_rowsum(p.rowsum, row, p.m, p.nseg, p.off);
    if (p.mm_part) srs[BM + t] = mm_held(p.row_edge, p.m, p.mm_left, p.mm_right, row);
  }
  __syncthreads();
  const bool mm = p.mm_part != nullptr;
  const float2 mm2 = with_post_mode_r(p.post_mode, [&](auto M) {
    float mn = FLT_MAX, mx = FLT_MIN;  // matrix.cc:335-336
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      const int col = col0 + j * 32 + r;
      if (col >= p.n) continue;
      const uint32_t cterm = i8_cterm(rc, p.colsum[col]);
      const float bias = p.bias ? p.bias[col] : 0.0f;
      const float sc = p.bn_scale ? p.bn_scale[col] : 1.0f;
      const float of = p.bn_offset ? p.bn_offset[col] : 0.0f;
#pragma unroll
      for (int i = 0; i < TI; ++i) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int lr = wrow + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
          const float y = i8_output<decltype(M)::value>((uint32_t)acc[i][j][e], srs[lr], cterm, rc.cscale, bias, sc, of,
                                                        p.post, p.npost);
          if (mm && srs[BM + lr]) mm_take(y, mn, mx);
          if (m0 + lr < p.m) p.y[(int64_t)(m0 + lr) * p.ldy + col] = y;
        }
      }
    }
    return make_float2(mn, mx);
  });
  if (mm) mm_store<NT>(p.mm_part, mm2.x, mm2.y);
}

// The same epilogue with the stores vectorised: each wave finishes its tile
// one 32-row slab at a time into a wave-private LDS slab (row stride padded
// by 32 B so the two row groups of a write land in different banks), then
// writes the slab back as 16-byte row chunks -- a quarter of the store
// instructions of i8_epilogue, whose 4-byte column stores made the epilogue
// store-issue bound.  Same values, same bits.  Needs n % 4 ==
// 0 and ldy % 4 == 0 (host-checked) and NW slabs of 32 x (TJ 32 + 8) floats
// plus BM words of row sums in `lds`.
template <int TI, int TJ, int BM, int NT>
__device__ __forceinline__ void i8_epilogue_v(const I8Args &p, const i32x16 (&acc)[TI][TJ], int m0, int wrow,
                                              int col0, int r, int h, char *lds) {
  constexpr int NW = NT / 64, SW = TJ * 32 + 8;  // slab row stride, floats
  const QP pa = *static_cast<const QP *>(p.pa);
  const I8Restore rc = i8_restore(pa, p.w_scale, p.w_zp, p.k);
  uint32_t *srs = reinterpret_cast<uint32_t *>(lds + NW * 32 * SW * 4);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float *slab = reinterpret_cast<float *>(lds) + wave * 32 * SW;
  __syncthreads();
  for (int t = threadIdx.x; t < BM; t += NT) {
    const int row = m0 + t;
    srs[t] = rc.cb * i8_spliced_rowsum(p.rowsum, row, p.m, p.nseg, p.off);
  }
  __syncthreads();
  // the next layer's held rows among this wave's 64: bit t = row wrow + t
  static_assert(TI == 2, "one 64-row mask per wave");
  const bool mm = p.mm_part != nullptr;
  const uint64_t hmask =
      mm ? __builtin_amdgcn_ballot_w64(mm_held(p.row_edge, p.m, p.mm_left, p.mm_right, m0 + wrow + lane)) : 0;
  // column constants of this lane's TJ columns, loaded once (columns past n
  // take column n-1's, and so do their weight rows in the caller's B loader:
  // such lanes repeat a valid output, which cannot move a min or max)
  uint32_t cterm[TJ];
  float bias[TJ], sc[TJ], of[TJ];
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int col = min(col0 + j * 32 + r, p.n - 1);
    cterm[j] = i8_cterm(rc, p.colsum[col]);
    bias[j] = p.bias ? p.bias[col] : 0.0f;
    sc[j] = p.bn_scale ? p.bn_scale[col] : 1.0f;
    of[j] = p.bn_offset ? p.bn_offset[col] : 0.0f;
  }
  constexpr int C4 = TJ * 8;  // float4 chunks per slab row
  const float2 mm2 = with_post_mode_r(p.post_mode, [&](auto M) {
    // FindMinMax (matrix.cc:331-345) as max / min: NaN never wins either way,
    // and a zero's sign cannot change the parameters
    float mn = FLT_MAX, mx = FLT_MIN;  // matrix.cc:335-336
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      float rmn[16], rmx[16];  // per row of the lane, over its TJ columns
#pragma unroll
      for (int e = 0; e < 16; ++e) rmn[e] = FLT_MAX, rmx[e] = FLT_MIN;
#pragma unroll
      for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int rr = (e & 3) + 8 * (e >> 2) + 4 * h;  // row within the slab
          const float y = i8_output<decltype(M)::value>((uint32_t)acc[i][j][e], srs[wrow + i * 32 + rr], cterm[j],
                                                        rc.cscale, bias[j], sc[j], of[j], p.post, p.npost);
          rmx[e] = fmaxf(rmx[e], y);
          rmn[e] = fminf(rmn[e], y);
          slab[rr * SW + j * 32 + r] = y;
        }
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int rr = (e & 3) + 8 * (e >> 2) + 4 * h;
        if ((hmask >> (i * 32 + rr)) & 1) {
          mx = fmaxf(mx, rmx[e]);
          mn = fminf(mn, rmn[e]);
        }
      }
      wave_lds_sync();
#pragma unroll
      for (int q = 0; q < 32 * C4 / 64; ++q) {
        const int idx = lane + 64 * q, rr = idx / C4, c4 = idx % C4;
        const int row = m0 + wrow + i * 32 + rr, col = col0 + 4 * c4;
        const float4 v = *reinterpret_cast<const float4 *>(slab + rr * SW + 4 * c4);
        // non-temporal: the next layer's Quantize reads it once, later
        // (serial hidden layer 36.8-37.0 -> 35.3-35.8 us, Quantize +0.4 us;
        // tools/experiments/i8_nt.sh)
        if (row < p.m && col < p.n) {
          typedef float nt4 __attribute__((ext_vector_type(4)));
          __builtin_nontemporal_store(nt4{v.x, v.y, v.z, v.w},
                                      reinterpret_cast<nt4 *>(p.y + (int64_t)row * p.ldy + col));
        }
      }
      wave_lds_sync();
    }
    return make_float2(mn, mx);
  });
  if (mm) mm_store<NT>(p.mm_part, mm2.x, mm2.y);
}

// Fused requantize (static int8): y exactly as i8_epilogue_v forms it, then
// Quantize with the NEXT layer's frozen parameters (qbyte's arithmetic, the
// function the quantize passes use: the same bytes), staged through the wave's LDS slab
// (32 rows x TJ 32 bytes, row stride + 16 B) and stored as 16-byte row chunks
// into that layer's operand buffer.  The chunk's lanes add their bytes and
// one of them adds the sum to the row's word (integer atomics: a row is
// finished by n / (TJ 32) waves of different blocks, in any order).  The
// blocks of column tile 0 clear q_zero's rows for the launch after this one.
// No fp32 output, no min / max partials.  LDS: NW slabs + BM words.
template <int TI, int TJ, int BM, int NT>
__device__ __forceinline__ void i8_epilogue_q(const I8Args &p, const i32x16 (&acc)[TI][TJ], int m0, int wrow,
                                              int col0, int r, int h, bool first_col_tile, char *lds) {
  constexpr int NW = NT / 64, SB = TJ * 32 + 16;  // slab row stride, bytes
  constexpr int C16 = TJ * 2;                     // 16-byte chunks per slab row
  static_assert(C16 == 4 && (32 * C16) % 64 == 0, "four lanes per row chunk group");
  const QP pa = *static_cast<const QP *>(p.pa);
  const QP pn = *static_cast<const QP *>(p.q_qp);
  const I8Restore rc = i8_restore(pa, p.w_scale, p.w_zp, p.k);
  const float nzp = (float)pn.zp;
  const float nrs = qbyte_rscale(pn.scale);  // as quantize_row
  uint32_t *srs = reinterpret_cast<uint32_t *>(lds + NW * 32 * SB);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int8_t *slab = reinterpret_cast<int8_t *>(lds) + wave * 32 * SB;
  __syncthreads();
  for (int t = threadIdx.x; t < BM; t += NT) {
    const int row = m0 + t;
    srs[t] = rc.cb * i8_spliced_rowsum(p.rowsum, row, p.m, p.nseg, p.off);
    if (first_col_tile && p.q_zero && row < p.m) p.q_zero[row] = 0;
  }
  __syncthreads();
  uint32_t cterm[TJ];
  float bias[TJ], sc[TJ], of[TJ];
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int col = col0 + j * 32 + r;  // n % 128 == 0: every column exists
    cterm[j] = i8_cterm(rc, p.colsum[col]);
    bias[j] = p.bias ? p.bias[col] : 0.0f;
    sc[j] = p.bn_scale ? p.bn_scale[col] : 1.0f;
    of[j] = p.bn_offset ? p.bn_offset[col] : 0.0f;
  }
  with_post_mode(p.post_mode, [&](auto M) {
#pragma unroll
    for (int i = 0; i < TI; ++i) {
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        // qbyte over the lane's 16 outputs of column j with its fallback
        // test once per wave (as quantize_rows_fast): the corrected
        // quotients first, the division only where one is not finite
        float yv[16], qv[16];
        bool bad = nrs == 0.0f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int rr = (e & 3) + 8 * (e >> 2) + 4 * h;  // row within the slab
          const float y = i8_output<decltype(M)::value>((uint32_t)acc[i][j][e], srs[wrow + i * 32 + rr], cterm[j],
                                                        rc.cscale, bias[j], sc[j], of[j], p.post, p.npost);
          const float q0 = y * nrs;
          const float qq = __builtin_fmaf(__builtin_fmaf(-pn.scale, q0, y), nrs, q0);
          bad |= __builtin_isinf(qq) || __builtin_isnan(qq);
          yv[e] = y;
          qv[e] = qq;
        }
        if (__builtin_amdgcn_ballot_w64(bad)) {
          if (bad) {
#pragma unroll
            for (int e = 0; e < 16; ++e)
              if (nrs == 0.0f || __builtin_isinf(qv[e]) || __builtin_isnan(qv[e])) qv[e] = yv[e] / pn.scale;
          }
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int rr = (e & 3) + 8 * (e >> 2) + 4 * h;
          float w = qv[e] + nzp;
          w = (255.0f < w) ? 255.0f : w;  // std::min(w, 255.0f)
          w = (0.0f < w) ? w : 0.0f;      // std::max(0.0f, w)
          slab[rr * SB + j * 32 + r] = (int8_t)((int)(uint8_t)roundf(w) - 128);
        }
      }
      wave_lds_sync();
#pragma unroll
      for (int q = 0; q < 32 * C16 / 64; ++q) {
        const int idx = lane + 64 * q, rr = idx / C16, c = idx % C16;
        const int row = m0 + wrow + i * 32 + rr;
        const i32x4 v = *reinterpret_cast<const i32x4 *>(slab + rr * SB + 16 * c);
        int sum = byte_sum(v[0]) + byte_sum(v[1]) + byte_sum(v[2]) + byte_sum(v[3]);
        if (row < p.m) *reinterpret_cast<i32x4 *>(p.qy + (int64_t)row * p.n + col0 + 16 * c) = v;
        i8_rowsum_group_add<C16>(sum, row < p.m, p.q_rowsum + min(row, p.m - 1));  // lane c == 0 adds
      }
      wave_lds_sync();
    }
  });
}

// The int8 GEMM (the product's: <256, 128, 3, 4, 2, false>): K-tiles of 128
// bytes travel global -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds) into
// three stages with the XOR chunk swizzle applied on the source address, one
// barrier per K-tile, counted vmcnt; 8 waves of 64 x 64: one tile per CU on
// the 1024-wide layers and two K-tiles in flight.  The loop is software-
// pipelined so that the LDS fragment reads and the MFMAs overlap:
//   * fragments are double-buffered in registers: k-step s + 1's four
//     ds_read_b128 are issued before k-step s's four MFMAs, so a read's
//     latency hides under the MFMAs instead of a lgkmcnt(0) before each step;
//   * the K-tile hand-off (wait for tile kt + 1's DMA, barrier, refill of
//     the stage tile kt used, first reads of tile kt + 1) sits after tile
//     kt's last MFMAs are issued, so the barrier's wait overlaps them.
// int32 accumulation is exact, so any product order gives the same bits.
// STAG (the experiments library): waves NW/2 .. NW-1 (the second wave of
// every SIMD) run two k-steps behind the first half: their ks 0-1 of tile 0
// before the loop, then per K-tile ks 2-3 of tile kt, the hand-off, ks 0-1 of
// tile kt+1.  The barriers, and so the stage protocol, are unchanged (a wave
// reaches tile kt's hand-off only after all its reads of tile kt); the two
// waves of a SIMD then read fragments while the other one multiplies
// (MI355X_MICROARCH.md, "try a stagger").  Exact int32: same bits.
template <int BM, int BN, int STAGES, int WGM, int WGN, bool STAG = false>
__global__ __launch_bounds__(64 * WGM * WGN, 1) void gemm_i8_pipe_kernel(I8Args p) {
  static_assert(STAGES == 3, "tile kt + 3 refills tile kt's stage");
  using T = I8Tile<BM, BN, WGM, WGN>;
  constexpr int NW = T::NW, BKB = T::BKB, TI = T::TI, TJ = T::TJ;
  constexpr int NGA = T::NGA, NGB = T::NGB, NG = T::NG, STAGE = T::STAGE;
  __shared__ __attribute__((aligned(1024))) int8_t smem[STAGES * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN, r = lane & 31, h = lane >> 5;
  int tm, tn;
  tile_of(blockIdx.x, p.tiles_m, p.tiles_n, p.group, &tm, &tn);
  const int m0 = tm * BM, n0 = tn * BN;

  // Source byte offsets of the wave's pieces at K-tile 0: the weights' once
  // (rows past n repeat row n - 1), the activations' per segment (source row
  // clamped to [0, m - 1] as Splice does).  The loops over the pieces, the
  // accumulator zeroing and the epilogue choice are written out here: moved
  // into helpers over the arrays they gave this kernel other machine code
  // (DESIGN.md §8 r14).
  const int lrow = lane / T::CH, lchunk = lane & (T::CH - 1);
  uint32_t boff[NGB];
#pragma unroll
  for (int j = 0; j < NGB; ++j) {
    const int row = T::dma_row(wave * NGB + j, lrow);
    boff[j] = (uint32_t)(min(n0 + row, p.n - 1) * p.kpad + T::dma_byte(row, lchunk));
  }
  uint32_t aoff[NGA];
  int cur_seg = -1;
  const auto ra = buf_rsrc(p.a), rw = buf_rsrc(p.w);
  auto issue = [&](int kt) {
    const int k0 = kt * BKB;
    const int seg = k0 / p.din, col0 = k0 - seg * p.din;
    if (seg != cur_seg) {
      cur_seg = seg;
      const int shift = seg_off(p, seg);
#pragma unroll
      for (int i = 0; i < NGA; ++i) {
        const int row = T::dma_row(wave * NGA + i, lrow);
        int src = m0 + row + shift;
        src = src < 0 ? 0 : (src > p.m - 1 ? p.m - 1 : src);
        aoff[i] = (uint32_t)(src * p.lda + T::dma_byte(row, lchunk));
      }
    }
    int8_t *st = smem + (kt % STAGES) * STAGE;
#pragma unroll
    for (int i = 0; i < NGA; ++i) buf_lds16(ra, st + (wave * NGA + i) * 1024, aoff[i] + col0);
#pragma unroll
    for (int j = 0; j < NGB; ++j) buf_lds16(rw, st + BM * BKB + (wave * NGB + j) * 1024, boff[j] + k0);
  };

  i32x16 acc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;

  const int xr = T::swz(r) ^ h;  // chunk 2s + h -> (2s) ^ xr
  const int a_row = (wm * TI * 32 + r) * BKB, b_row = BM * BKB + (wn * TJ * 32 + r) * BKB;
  const int ktiles = p.kpad / BKB;
  i32x4 fa[2][TI], fb[2][TJ];
  auto read = [&](int kt, int s, int buf) {
    const int8_t *st = smem + (kt % STAGES) * STAGE;
    const int ch = ((2 * s) ^ xr) * 16;
#pragma unroll
    for (int i = 0; i < TI; ++i) fa[buf][i] = *reinterpret_cast<const i32x4 *>(st + a_row + i * 32 * BKB + ch);
#pragma unroll
    for (int j = 0; j < TJ; ++j) fb[buf][j] = *reinterpret_cast<const i32x4 *>(st + b_row + j * 32 * BKB + ch);
  };
  auto mma = [&](int buf) {
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[buf][i], fb[buf][j], acc[i][j], 0, 0, 0);
  };
  // tile kt has landed once at most the newer tiles' groups are outstanding
  auto wait_tile = [&](int newer) {
    if (newer >= 2)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NG) : "memory");
    else if (newer == 1)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NG) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };

  for (int t = 0; t < STAGES - 1 && t < ktiles; ++t) issue(t);
  wait_tile(min(ktiles - 1, STAGES - 2));
  __builtin_amdgcn_s_barrier();
  if (STAGES - 1 < ktiles) issue(STAGES - 1);
  read(0, 0, 0);
  if (STAG && wave >= NW / 2) {
    // the late half: ks 0-1 of tile 0 now, then two k-steps behind
    read(0, 1, 1);
    __builtin_amdgcn_sched_barrier(0);
    mma(0);
    __builtin_amdgcn_sched_barrier(0);
    read(0, 2, 0);
    __builtin_amdgcn_sched_barrier(0);
    mma(1);
    __builtin_amdgcn_sched_barrier(0);
    for (int kt = 0; kt < ktiles; ++kt) {
      read(kt, 3, 1);
      __builtin_amdgcn_sched_barrier(0);
      mma(0);
      __builtin_amdgcn_sched_barrier(0);
      mma(1);
      __builtin_amdgcn_sched_barrier(0);
      if (kt + 1 < ktiles) {
        wait_tile(kt + 2 < ktiles ? 1 : 0);
        __builtin_amdgcn_s_barrier();
        if (kt + STAGES < ktiles) issue(kt + STAGES);
        read(kt + 1, 0, 0);
        read(kt + 1, 1, 1);
        __builtin_amdgcn_sched_barrier(0);
        mma(0);
        __builtin_amdgcn_sched_barrier(0);
        read(kt + 1, 2, 0);
        __builtin_amdgcn_sched_barrier(0);
        mma(1);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  } else
  for (int kt = 0; kt < ktiles; ++kt) {
    // k-steps 0..2: the next step's reads, then this step's MFMAs
    read(kt, 1, 1);
    __builtin_amdgcn_sched_barrier(0);
    mma(0);
    __builtin_amdgcn_sched_barrier(0);
    read(kt, 2, 0);
    __builtin_amdgcn_sched_barrier(0);
    mma(1);
    __builtin_amdgcn_sched_barrier(0);
    read(kt, 3, 1);
    __builtin_amdgcn_sched_barrier(0);
    mma(0);
    __builtin_amdgcn_sched_barrier(0);
    // k-step 3's MFMAs first, then the hand-off to tile kt + 1 under them
    mma(1);
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 1 < ktiles) {
      // newer tiles than kt + 1 already issued: kt + 2 if it exists
      wait_tile(kt + 2 < ktiles ? 1 : 0);
      __builtin_amdgcn_s_barrier();  // every wave is past its reads of tile kt's stage
      if (kt + STAGES < ktiles) issue(kt + STAGES);
      read(kt + 1, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }

  if constexpr (TJ == 2) {
    static_assert(NW * 32 * (TJ * 32 + 16) + BM * 4 <= STAGES * STAGE, "byte slabs + row sums in the stages");
    if (p.qy) {
      i8_epilogue_q<TI, TJ, BM, 64 * NW>(p, acc, m0, wm * TI * 32, n0 + wn * TJ * 32, r, h, tn == 0,
                                         reinterpret_cast<char *>(smem));
      return;
    }
  }
  constexpr bool kVecFits = TI == 2 && NW * 32 * (TJ * 32 + 8) * 4 + BM * 4 <= STAGES * STAGE;
  if constexpr (kVecFits) {
    if (p.vec_epi) {
      i8_epilogue_v<TI, TJ, BM, 64 * NW>(p, acc, m0, wm * TI * 32, n0 + wn * TJ * 32, r, h,
                                         reinterpret_cast<char *>(smem));
      return;
    }
  }
  i8_epilogue<TI, TJ, BM, 64 * NW>(p, acc, m0, wm * TI * 32, n0 + wn * TJ * 32, r, h,
                                   reinterpret_cast<uint32_t *>(smem));
}

// One launch: `kernel`, an instantiation on T's tiles, one block per tile in
// tile_order.h's XCD groups (an XCD's tiles: 8 column tiles x its row
// blocks); *nparts = the (min, max) partials its epilogue leaves, one per wave.
template <class T>
int i8_launch(hipStream_t s, void (*kernel)(I8Args), I8Args p, int *nparts) {
  static_assert(T::BM >= kI8MinTile && T::BN >= kI8MinTile && T::NW <= kI8MaxWaves, "i8_gemm_parts' bound");
  p.tiles_n = (p.n + T::BN - 1) / T::BN;
  p.tiles_m = (p.m + T::BM - 1) / T::BM;
  p.group = 8;
  if (nparts) *nparts = p.tiles_m * p.tiles_n * T::NW;
  hipLaunchKernelGGL(kernel, dim3(p.tiles_m * p.tiles_n), dim3(T::NT), 0, s, p);
  CE_HIP(hipGetLastError());
  return CE_GPU_OK;
}

// launch_i8_gemm's arguments as the kernel arguments; the tile counts are
// i8_launch's.
inline I8Args i8_args(const I8Layer &L, const int8_t *a, int lda, int m, const int32_t *rowsum, const void *pa,
                      float *y, int ldy, const I8NextMinMax *mm, const I8NextBytes *nb, int off_shift) {
  I8Args p = {};
  if (nb) {
    p.qy = nb->xq;
    p.q_rowsum = nb->rowsum;
    p.q_zero = nb->zero;
    p.q_qp = nb->qp;
  }
  if (mm) {
    p.mm_part = static_cast<float2 *>(mm->part);
    p.row_edge = mm->row_edge;
    p.mm_left = mm->in_left;
    p.mm_right = mm->in_right;
  }
  p.a = a;
  p.lda = lda;
  p.m = m;
  p.din = L.a_din;
  p.nseg = L.a_nseg;
  for (int i = 0; i < 8; ++i) p.off[i] = i < L.a_nseg ? L.a_off[i] - off_shift : 0;
  p.rowsum = rowsum;
  p.w = L.wq.as<int8_t>();
  p.colsum = L.colsum.as<int32_t>();
  p.n = L.n;
  p.k = L.k;
  p.kpad = L.kpad;
  p.pa = pa;
  p.w_scale = L.w_scale;
  p.w_zp = L.w_zp;
  p.bias = L.bias;
  p.bn_scale = L.bn_scale;
  p.bn_offset = L.bn_offset;
  for (int i = 0; i < 4; ++i) p.post[i] = L.post[i];
  p.npost = L.npost;
  p.post_mode = post_mode(L.post, L.npost);
  p.y = y;
  p.ldy = ldy;
  static const int vec_epi = CE_KNOB("CATEARS_I8_EPI", 1);
  p.vec_epi = vec_epi && L.n % 4 == 0 && ldy % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
  return p;
}

}  // namespace
}  // namespace catears
