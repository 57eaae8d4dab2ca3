// gemm_bf16.hip -- the TDNN layers as plain bf16 GEMMs (CE_GPU_GEMM_BF16).
//
// Same contraction as gemm_bf16x6.hip (Splice + Narrow + LinearLayer + bias /
// ReLU / BatchNorm), with both operands rounded to bf16 once and one
// v_mfma_f32_16x16x32_bf16 product per K-tile of 32:
//
//   y_j = sum_k bf16(a_k) * bf16(w_kj)      (exact products, fp32 accumulator,
//                                            ascending K, one accumulator)
//
// then x6_epilogue's arithmetic (+ bias, post chain in the reference's
// rounding order); a hidden layer stores bf16(y) (v_cvt_pk_bf16_f32, round to
// nearest even), the last layer fp32.
//
// Layout (HBM):
//   weights  plane 0 of the bf16x6 fragment image (X6Gemm::wd): fragment
//            (16-unit block u, K-tile t) is the contiguous 1 KB at
//            ((u * wd_kt + t) * 3) * 512 elements, lane l's 8 bf16 at 8 l;
//            units zero padded to a multiple of kX6DirUnits, so no tile of
//            either shape reads past the image
//   acts     rows x ldx bf16, written by the previous layer's epilogue (or by
//            splice_pad_bf16 for the first layer), read through the splice
//            offsets with rows clamped to [0, m-1]; a K-tile lies inside one
//            segment (din % 32 == 0)
//
// The MFMA's A operand is the weights, B the activations: a lane ends with
// four consecutive units of one frame (one 8-byte bf16 store, or 16 bytes of
// fp32).
//
// Both operands travel global -> LDS by 16-byte LDS-DMA into a STAGES-deep
// ring, one raw barrier per K-tile, counted vmcnt (gemm_bf16x6q_kernel's
// protocol with one plane).  A weight piece is one fragment, stored as it is
// (lane-linear: the fragment read is conflict free); an activation piece is
// 16 rows x 64 B with gemm_bf16x6q_kernel's source-side chunk swizzle.
// Weights go through LDS too rather than straight into registers: an
// ordinary VGPR load beside LDS-DMAs in flight makes the compiler drain the
// whole VM queue at its use, which would serialise the ring.
//
// Two tile shapes (the host's choice is bf16_small_tile, a function of rows
// and n only): 128 units x 128 frames on 8 waves of 32 x 64 (two per SIMD;
// measured 18 % faster per 4072-row TDNN-S block than 4 waves of 64 x 64,
// DESIGN.md §8) for full batches, 32 x 32 on 2 waves so that a 70-row chunk
// or a single row is not one mostly empty tile.  Both use the same MFMA, the
// same K order and no split-K, so a row's bits do not depend on the shape,
// the row count or its place in the block.
//
// A third kernel, kernels/gemm_bf16_lat.hip, takes the launches of a latency
// context (X6Gemm::lat) up to kB16LatMaxRows rows: the same arithmetic without
// LDS.  The arguments and the epilogue of all three are gemm_bf16_kernels.h's.
#include <hip/hip_runtime.h>

#include "../gemm_bf16_kernels.h"
#include "../internal.h"
#include "../lds_dma.h"
#include "../tile_order.h"

namespace catears {
namespace {

using dma::clampi;
using dma::glds16;
using dma::wait_vmcnt;

template <int BW_, int BF_, int WGW_, int WGF_, int STAGES_>
struct B16Cfg {
  static constexpr int BW = BW_, BF = BF_, WGW = WGW_, WGF = WGF_, STAGES = STAGES_;
  static constexpr int NW = WGW * WGF, NT = 64 * NW;
  static constexpr int TW = BW / WGW / 16, TF = BF / WGF / 16;  // 16 x 16 fragments per wave
  static constexpr int QW = BW / 16, QF = BF / 16;               // DMA pieces per stage
  static constexpr int NQW = QW / NW, NQF = QF / NW, NQ = NQW + NQF;
  static constexpr int STAGE = (BW + BF) * 64;                   // bytes per stage
  static_assert(TW >= 1 && TF >= 1 && QW % NW == 0 && QF % NW == 0, "bad bf16 tile");
  static_assert(STAGES >= 2 && STAGES * STAGE <= 64 * 1024, "LDS");
};

// Step kt holds tile kt's fragments in registers (read from stage kt % S at
// the end of step kt-1).  Once every wave has drained those reads
// (lgkmcnt(0)) and passed the barrier, stage kt % S is free and tile kt+S is
// issued into it, S-1 steps ahead of its first read.  RAW: tile kt+1 is read
// right after the barrier; every wave's vmcnt((S-2) NQ) before it retired all
// but its newest S-2 issues (tiles kt+2 .. kt+S-1), i.e. its pieces of tile
// kt+1.  Past the end the issued tile is clamped to ktiles-1: a refetch of
// the last tile into the stage it already occupies (the same bytes), which
// keeps one issue per step for the vmcnt count; the fragment read of the
// nonexistent tile ktiles is never used.
template <class C, bool OUT16>
__global__ __launch_bounds__(C::NT) void gemm_bf16_kernel(B16Args p) {
  constexpr int BW = C::BW, BF = C::BF, TW = C::TW, TF = C::TF;
  constexpr int STAGE = C::STAGE, NQ = C::NQ, QW = C::QW, S = C::STAGES;
  __shared__ __attribute__((aligned(1024))) char smem[S * STAGE];
  auto swz = [](int row) { return ((row >> 3) & 1) << 1; };

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ww = wave / C::WGF, wf = wave % C::WGF;
  int tm, tn;
  tile_of(blockIdx.x, p.tiles_m, p.tiles_n, p.group, &tm, &tn);
  const int f0 = tm * BF, n0 = tn * BW;

  // wave w issues weight pieces w NQW .. and activation pieces w NQF ..;
  // piece q is stored at stage + 1 KB * q (weights first)
  const int lrow = lane >> 2, lch = lane & 3;
  int piece[NQ];
  uint32_t pconst[NQ];  // weight: byte offset of the fragment at K-tile 0; activation: chunk offset
  int xrow[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    if (i < C::NQW) {
      const int q = wave * C::NQW + i;
      piece[i] = q;
      pconst[i] = (uint32_t)(((n0 / 16 + q) * p.wd_kt * 3) * 1024 + lane * 16);
      xrow[i] = 0;
    } else {
      const int q2 = wave * C::NQF + (i - C::NQW), row = q2 * 16 + lrow;
      piece[i] = QW + q2;
      pconst[i] = (uint32_t)(16 * (lch ^ swz(row)));
      xrow[i] = f0 + row;
    }
  }
  const int ktiles = p.kpad / 32;
  auto issue = [&](int kt) {
    kt = min(kt, ktiles - 1);
    const int k0 = kt * 32;
    const int seg = k0 / p.din, col0 = k0 - seg * p.din;
    const int shift = (int)(signed char)(p.off_packed >> (8 * seg));
    char *st = smem + (kt % S) * STAGE;
    const char *wbase = reinterpret_cast<const char *>(p.wd) + (size_t)kt * 3 * 1024;
    const char *xbase = reinterpret_cast<const char *>(p.x) + (size_t)col0 * 2;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const uint32_t xo = (uint32_t)(clampi(xrow[i] + shift, 0, p.m - 1) * p.ldx * 2) + pconst[i];
      const char *src = i < C::NQW ? wbase + pconst[i] : xbase + xo;
      glds16(src, st + piece[i] * 1024);
    }
  };
  const int foff = (lane & 15) * 64 + (((lane >> 4) ^ (((lane >> 3) & 1) << 1)) * 16);
  const int wfrag = ww * TW, frow = wf * TF * 16;
  auto rd = [&](const char *st, bf16x8 *a, bf16x8 *b) {
#pragma unroll
    for (int i = 0; i < TW; ++i) a[i] = *reinterpret_cast<const bf16x8 *>(st + (wfrag + i) * 1024 + lane * 16);
#pragma unroll
    for (int j = 0; j < TF; ++j) b[j] = *reinterpret_cast<const bf16x8 *>(st + QW * 1024 + (frow + j * 16) * 64 + foff);
  };
  f32x4 acc[TW][TF];
#pragma unroll
  for (int i = 0; i < TW; ++i)
#pragma unroll
    for (int j = 0; j < TF; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  bf16x8 a[2][TW], b[2][TF];
#pragma unroll
  for (int t = 0; t < S; ++t) issue(t);
  wait_vmcnt<(S - 1) * NQ>();
  __builtin_amdgcn_s_barrier();
  rd(smem, a[0], b[0]);

  auto body = [&](int kt, auto cc) {
    constexpr int c = decltype(cc)::value;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wait_vmcnt<(S - 2) * NQ>();
    __builtin_amdgcn_s_barrier();
    issue(kt + S);
    rd(smem + ((kt + 1) % S) * STAGE, a[c ^ 1], b[c ^ 1]);
#pragma unroll
    for (int i = 0; i < TW; ++i)
#pragma unroll
      for (int j = 0; j < TF; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[c][i], b[c][j], acc[i][j], 0, 0, 0);
  };
  int kt = 0;
  for (; kt + 1 < ktiles; kt += 2) {
    body(kt, std::integral_constant<int, 0>());
    body(kt + 1, std::integral_constant<int, 1>());
  }
  if (kt < ktiles) body(kt, std::integral_constant<int, 0>());
  wait_vmcnt<0>();  // drain the tail refetches before the block ends

  b16_epilogue<TW, TF, OUT16>(p, acc, n0 + wfrag * 16, f0 + frow, lane);
}

// First layer: the gathered (row_map), spliced, zero-padded input rows as
// bf16 (splice_pad_split_kernel's plane 0): out row r is `po` wide, columns
// nseg*din .. po-1 are zero.
__global__ __launch_bounds__(256) void splice_pad_bf16_kernel(const float *__restrict__ in, int ld_in, int rows, int din,
                                                              int nseg, SpliceIdx8 idx, const int *__restrict__ row_map,
                                                              uint16_t *__restrict__ out, int po) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  uint16_t *o = out + (int64_t)r * po;
  for (int c = lane; c < po; c += 64) {
    const int s = c / din;
    float v = 0.0f;
    if (s < nseg) {
      int src = clampi(r + idx.v[s], 0, rows - 1);
      if (row_map) src = row_map[src];
      v = in[(int64_t)src * ld_in + (c - s * din)];
    }
    o[c] = (uint16_t)bf16_pair(v, 0.0f);
  }
}

template <class C>
int launch_b16(hipStream_t s, B16Args p, bool out16) {
  p.tiles_n = (p.n + C::BW - 1) / C::BW;
  p.tiles_m = (p.m + C::BF - 1) / C::BF;
  dim3 grid(p.tiles_m * p.tiles_n), block(C::NT);
  if (out16)
    hipLaunchKernelGGL((gemm_bf16_kernel<C, true>), grid, block, 0, s, p);
  else
    hipLaunchKernelGGL((gemm_bf16_kernel<C, false>), grid, block, 0, s, p);
  CE_HIP(hipGetLastError());
  return CE_GPU_OK;
}

}  // namespace

// The tile rule: 128 x 128 tiles once they number at least kB16LargeMinTiles
// (a quarter of the chip's 256 CUs; below that the 32 x 32 tiles, sixteen
// times as many, spread the layer over more of them).  Unmeasured choice.
bool bf16_small_tile(int rows, int n) {
  return (int64_t)((rows + 127) / 128) * ((n + 127) / 128) < kB16LargeMinTiles;
}

int launch_gemm_bf16(hipStream_t s, const X6Gemm &a) {
  if (a.m <= 0 || a.n <= 0) return CE_GPU_OK;
  // latency mode: a function of the row count only (the same bits)
  if (a.lat && a.m <= b16_lat_max_rows()) return launch_gemm_bf16_lat(s, a);
  B16Args p;
  CE_TRY(b16_fill_args(a, &p));
  const bool out16 = a.y16 != nullptr;
  if (bf16_small_tile(a.m, a.n)) return launch_b16<B16Cfg<32, 32, 2, 1, 4>>(s, p, out16);
  return launch_b16<B16Cfg<128, 128, 4, 2, 3>>(s, p, out16);
}

int launch_splice_pad_bf16(hipStream_t s, const float *in, int ld_in, int rows, int din, int nseg, const int *off,
                           const int *row_map, uint16_t *out, int po) {
  if (rows <= 0) return CE_GPU_OK;
  if (nseg < 1 || nseg > 8 || din <= 0 || nseg * din > po) return fail(CE_GPU_EINVAL, "splice_pad_bf16: bad geometry");
  SpliceIdx8 idx;
  for (int i = 0; i < 8; ++i) idx.v[i] = i < nseg ? off[i] : 0;
  hipLaunchKernelGGL(splice_pad_bf16_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, in, ld_in, rows, din, nseg, idx,
                     row_map, out, po);
  CE_HIP(hipGetLastError());
  return CE_GPU_OK;
}

}  // namespace catears
