// nnet_i8_exp.hip -- the int8 GEMM's measurement variants: what the
// experiments library (`make EXPERIMENTS=1`, libcatears_hip_exp.so) carries
// beside the product's launch_i8_gemm of nnet_i8.hip.  The product object of
// this file is empty.  CATEARS_I8_GEMM selects:
//
//    0          gemm_i8_nnet_kernel: 128 x 128 tiles, 64-byte K-tiles loaded
//               through registers, one stage -- the first int8 GEMM
//   10, 11      gemm_i8_reg_kernel: K-tiles through registers instead of
//               LDS-DMA, 128 x 128 (4 waves) and the product's tile
//   15          gemm_i8_glds_kernel on the product's tile: the product's
//               kernel before its loop was software-pipelined
//   16          the product's kernel (nnet_i8.hip; never dispatched here)
//   17          16 with waves 4-7 two k-steps behind waves 0-3 (STAG)
//   40, 41, 44  gemm_i8_glds_kernel on 64-byte K-tiles: 256 x 256 with 4 / 3
//               stages, 256 x 128 with 4 (tools/experiments/i8_tiles.sh)
//   61-71       DIAG ablations of 15 (wrong results, timing only;
//               tools/experiments/i8_diag.sh)
// All but the ablations give the product's bits (int32 accumulation is
// exact; tests/test_gpu_i8_variants.py).  Kernels and tiles that were
// measured slower and then removed are recorded with their numbers in
// DESIGN.md §8 (r14) and profiles/.
#ifdef CATEARS_EXPERIMENTS
#include <string>

#include "../nnet_i8_kernels.h"

namespace catears {
namespace {

template <int TI, int TJ>
__device__ __forceinline__ void i8_zero(i32x16 (&acc)[TI][TJ]) {
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;
}

constexpr int IBM = 128, IBN = 128, IBK = 64, ILD = IBK + 16;  // bytes

__global__ __launch_bounds__(256, 2) void gemm_i8_nnet_kernel(I8Args p) {
  __shared__ __attribute__((aligned(16))) int8_t As[IBM * ILD];
  __shared__ __attribute__((aligned(16))) int8_t Bs[IBN * ILD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, r = lane & 31, h = lane >> 5;
  const int tm = blockIdx.x / p.tiles_n, tn = blockIdx.x - tm * p.tiles_n;
  const int m0 = tm * IBM, n0 = tn * IBN;

  i32x16 acc[2][2];
  i8_zero(acc);

  for (int k0 = 0; k0 < p.kpad; k0 += IBK) {
    // one K-tile never straddles a segment (din % 64 == 0 or nseg == 1)
    const int seg = k0 / p.din, col0 = k0 - seg * p.din;
    const int shift = seg_off(p, seg);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + 256 * i, row = idx >> 2, c16 = idx & 3;
      int src = m0 + row + shift;
      src = src < 0 ? 0 : (src > p.m - 1 ? p.m - 1 : src);
      i32x4 v = (i32x4){0, 0, 0, 0};
      if (col0 + 16 * c16 < p.din && k0 < p.k)
        v = *reinterpret_cast<const i32x4 *>(p.a + (int64_t)src * p.lda + col0 + 16 * c16);
      *reinterpret_cast<i32x4 *>(As + row * ILD + 16 * c16) = v;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + 256 * i, row = idx >> 2, c16 = idx & 3;
      const int gn = min(n0 + row, p.n - 1);
      *reinterpret_cast<i32x4 *>(Bs + row * ILD + 16 * c16) =
          *reinterpret_cast<const i32x4 *>(p.w + (int64_t)gn * p.kpad + k0 + 16 * c16);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < IBK / 32; ++s) {
      i32x4 af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        af[i] = *reinterpret_cast<const i32x4 *>(As + (wm * 64 + i * 32 + r) * ILD + 32 * s + 16 * h);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        bf[j] = *reinterpret_cast<const i32x4 *>(Bs + (wn * 64 + j * 32 + r) * ILD + 32 * s + 16 * h);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  i8_epilogue<2, 2, IBM, 256>(p, acc, m0, wm * 64, n0 + wn * 64, r, h, reinterpret_cast<uint32_t *>(As));
}

// The plain LDS-DMA loop on an I8Tile (the fp32 kernel's structure,
// gemm_f32.hip): global_load_lds_dwordx4 into STAGES stages, one barrier per
// K-tile, the four (BKB = 64: two) k-steps' fragment reads each right before
// their MFMAs.  DIAG (timing breakdowns, wrong results): bit 1 no DMA after
// the prologue, 2 no MFMAs (fragment reads kept live), 4 no fragment reads
// (MFMAs on constant operands), 8 no epilogue.
template <int BM, int BN, int STAGES, int WGM = 2, int WGN = 2, int BKB = 128, int DIAG = 0>
__global__ __launch_bounds__(64 * WGM * WGN, 1) void gemm_i8_glds_kernel(I8Args p) {
#ifndef CATEARS_DIAG
  static_assert(DIAG == 0, "diagnostic schedules are CATEARS_DIAG builds only");
#endif
  using T = I8Tile<BM, BN, WGM, WGN, BKB>;
  constexpr int NW = T::NW, TI = T::TI, TJ = T::TJ;
  constexpr int NGA = T::NGA, NGB = T::NGB, NG = T::NG, STAGE = T::STAGE;
  __shared__ __attribute__((aligned(1024))) int8_t smem[STAGES * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN, r = lane & 31, h = lane >> 5;
  int tm, tn;
  tile_of(blockIdx.x, p.tiles_m, p.tiles_n, p.group, &tm, &tn);
  const int m0 = tm * BM, n0 = tn * BN;

  // the loader addressing of gemm_i8_pipe_kernel
  const int lrow = lane / T::CH, lchunk = lane & (T::CH - 1);
  uint32_t boff[NGB];
#pragma unroll
  for (int j = 0; j < NGB; ++j) {
    const int row = T::dma_row(wave * NGB + j, lrow);
    boff[j] = (uint32_t)(min(n0 + row, p.n - 1) * p.kpad + T::dma_byte(row, lchunk));
  }
  uint32_t aoff[NGA];
  int cur_seg = -1;
  auto issue = [&](int kt) {
    const int k0 = kt * BKB;
    const int seg = k0 / p.din, col0 = k0 - seg * p.din;
    if (seg != cur_seg) {
      cur_seg = seg;
      const int shift = seg_off(p, seg);
#pragma unroll
      for (int i = 0; i < NGA; ++i) {
        const int row = T::dma_row(wave * NGA + i, lrow);
        aoff[i] = (uint32_t)(dma::clampi(m0 + row + shift, 0, p.m - 1) * p.lda + T::dma_byte(row, lchunk));
      }
    }
    char *st = reinterpret_cast<char *>(smem) + (kt % STAGES) * STAGE;
    const char *abase = reinterpret_cast<const char *>(p.a) + col0;
    const char *bbase = reinterpret_cast<const char *>(p.w) + k0;
#pragma unroll
    for (int i = 0; i < NGA; ++i) dma::glds16(abase + aoff[i], st + (wave * NGA + i) * 1024);
#pragma unroll
    for (int j = 0; j < NGB; ++j) dma::glds16(bbase + boff[j], st + BM * BKB + (wave * NGB + j) * 1024);
  };

  i32x16 acc[TI][TJ];
  i8_zero(acc);

  const int xr = T::swz(r) ^ h;  // chunk 2s + h -> (2s) ^ xr
  const int a_row = (wm * TI * 32 + r) * BKB, b_row = BM * BKB + (wn * TJ * 32 + r) * BKB;
  const int ktiles = p.kpad / BKB;
  // STAGES-1 tiles in flight: tile kt has landed once at most STAGES-2 newer
  // tiles' DMAs are outstanding (counted vmcnt, raw barrier: the DMAs stay in
  // flight across it); the stage refilled at kt is the one read at kt-1.
  for (int t = 0; t < STAGES - 1 && t < ktiles; ++t) issue(t);
  for (int kt = 0; kt < ktiles; ++kt) {
    const int ahead = min(ktiles - 1 - kt, STAGES - 2);  // newer tiles already issued
    if (ahead >= 2)
      dma::wait_vmcnt<2 * NG>();
    else if (ahead == 1)
      dma::wait_vmcnt<NG>();
    else
      dma::wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (!(DIAG & 1) && kt + STAGES - 1 < ktiles) issue(kt + STAGES - 1);
    const int8_t *st = smem + (kt % STAGES) * STAGE;
#pragma unroll
    for (int s = 0; s < BKB / 32; ++s) {
      const int ch = ((2 * s) ^ xr) * 16;
      i32x4 af[TI], bf[TJ];
#pragma unroll
      for (int i = 0; i < TI; ++i)
        af[i] = (DIAG & 4) ? i32x4{kt, s, i, 1} : *reinterpret_cast<const i32x4 *>(st + a_row + i * 32 * BKB + ch);
#pragma unroll
      for (int j = 0; j < TJ; ++j)
        bf[j] = (DIAG & 4) ? i32x4{s, kt, j, 2} : *reinterpret_cast<const i32x4 *>(st + b_row + j * 32 * BKB + ch);
      if constexpr ((DIAG & 2) != 0) {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < TJ; ++j) acc[i][j][0] ^= af[i][0] ^ bf[j][1];
        continue;
      }
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  }

  if constexpr ((DIAG & 8) != 0) {  // no epilogue: one word per lane keeps the loop live
    int t = 0;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < TJ; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) t ^= acc[i][j][e];
    p.y[(int64_t)blockIdx.x * 64 * NW + tid] = (float)t;
    return;
  }
  // slabs + row sums in the stages; one 64-row held-row mask per wave
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

// Register-staged form: the next K-tile is fetched with global_load_dwordx4
// into VGPRs while the current one is multiplied, then written to the other
// LDS buffer with ds_write_b128.  An LDS-DMA piece costs its wave ~60-180
// issue cycles per KiB (MI355X_MICROARCH.md, per-instruction constants), and
// an i8 MFMA consumes operands as fast as a bf16 one (1 KiB per 32 cycles),
// so at 128 x 128 the DMA issue alone matched the MFMA time; a plain
// 16-byte load + LDS write per KiB costs a few cycles.  One barrier per
// K-tile: the buffer written at kt was last read at kt-1, before that
// iteration's barrier.  The tile, swizzle and fragment reads of I8Tile.
// Kept here because no measurement of it is on record.
template <int BM, int BN, int WGM, int WGN>
__global__ __launch_bounds__(64 * WGM * WGN, 1) void gemm_i8_reg_kernel(I8Args p) {
  using T = I8Tile<BM, BN, WGM, WGN>;
  constexpr int NT = T::NT, BKB = T::BKB, TI = T::TI, TJ = T::TJ, STAGE = T::STAGE;
  constexpr int LA = BM * 8 / NT, LB = BN * 8 / NT;  // 16-byte chunks per thread
  static_assert(LA * NT == BM * 8 && LB * NT == BN * 8, "tile shape");
  __shared__ __attribute__((aligned(16))) int8_t smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN, r = lane & 31, h = lane >> 5;
  int tm, tn;
  tile_of(blockIdx.x, p.tiles_m, p.tiles_n, p.group, &tm, &tn);
  const int m0 = tm * BM, n0 = tn * BN;

  // thread -> (row, chunk) of the tile: chunk = tid & 7 for every piece
  const int chunk = tid & 7, row_base = tid >> 3;
  constexpr int RSTEP = NT / 8;
  uint32_t boff[LB], bdst[LB];
#pragma unroll
  for (int j = 0; j < LB; ++j) {
    const int row = row_base + j * RSTEP;
    boff[j] = (uint32_t)(min(n0 + row, p.n - 1) * p.kpad + 16 * chunk);
    bdst[j] = (uint32_t)(BM * BKB + row * BKB + T::dma_byte(row, chunk));
  }
  uint32_t aoff[LA], adst[LA];
#pragma unroll
  for (int i = 0; i < LA; ++i) {
    const int row = row_base + i * RSTEP;
    adst[i] = (uint32_t)(row * BKB + T::dma_byte(row, chunk));
  }
  int cur_seg = -1;
  i32x4 ra[LA], rb[LB];
  auto fetch = [&](int kt) {
    const int k0 = kt * BKB;
    const int seg = k0 / p.din, col0 = k0 - seg * p.din;
    if (seg != cur_seg) {
      cur_seg = seg;
      const int shift = seg_off(p, seg);
#pragma unroll
      for (int i = 0; i < LA; ++i)
        aoff[i] = (uint32_t)(dma::clampi(m0 + row_base + i * RSTEP + shift, 0, p.m - 1) * p.lda + 16 * chunk);
    }
    const int8_t *abase = p.a + col0;
    const int8_t *bbase = p.w + k0;
#pragma unroll
    for (int i = 0; i < LA; ++i) ra[i] = *reinterpret_cast<const i32x4 *>(abase + aoff[i]);
#pragma unroll
    for (int j = 0; j < LB; ++j) rb[j] = *reinterpret_cast<const i32x4 *>(bbase + boff[j]);
  };
  auto stash = [&](int8_t *st) {
#pragma unroll
    for (int i = 0; i < LA; ++i) *reinterpret_cast<i32x4 *>(st + adst[i]) = ra[i];
#pragma unroll
    for (int j = 0; j < LB; ++j) *reinterpret_cast<i32x4 *>(st + bdst[j]) = rb[j];
  };

  i32x16 acc[TI][TJ];
  i8_zero(acc);

  const int xr = T::swz(r) ^ h;
  const int a_row = (wm * TI * 32 + r) * BKB, b_row = BM * BKB + (wn * TJ * 32 + r) * BKB;
  const int ktiles = p.kpad / BKB;
  fetch(0);
  stash(smem);
  __syncthreads();
  for (int kt = 0; kt < ktiles; ++kt) {
    const bool more = kt + 1 < ktiles;
    if (more) fetch(kt + 1);
    const int8_t *st = smem + (kt & 1) * STAGE;
#pragma unroll
    for (int s = 0; s < BKB / 32; ++s) {
      const int ch = ((2 * s) ^ xr) * 16;
      i32x4 af[TI], bf[TJ];
#pragma unroll
      for (int i = 0; i < TI; ++i) af[i] = *reinterpret_cast<const i32x4 *>(st + a_row + i * 32 * BKB + ch);
#pragma unroll
      for (int j = 0; j < TJ; ++j) bf[j] = *reinterpret_cast<const i32x4 *>(st + b_row + j * 32 * BKB + ch);
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if (more) stash(smem + ((kt + 1) & 1) * STAGE);
    __syncthreads();
  }
  i8_epilogue<TI, TJ, BM, NT>(p, acc, m0, wm * TI * 32, n0 + wn * TJ * 32, r, h, reinterpret_cast<uint32_t *>(smem));
}

// gemm_i8_glds_kernel<BM, BN, STAGES, WGM, WGN, BKB, DIAG> on its tile
template <int BM, int BN, int STAGES, int WGM, int WGN, int BKB = 128, int DIAG = 0>
int launch_glds(hipStream_t s, const I8Args &p, int *nparts) {
  return i8_launch<I8Tile<BM, BN, WGM, WGN, BKB>>(s, gemm_i8_glds_kernel<BM, BN, STAGES, WGM, WGN, BKB, DIAG>, p,
                                                  nparts);
}

}  // namespace

int i8_gemm_variant() {
  static const int v = CE_KNOB("CATEARS_I8_GEMM", 16);
  return v;
}

int launch_i8_gemm_exp(hipStream_t s, const I8Layer &L, const int8_t *a, int lda, int m, const int32_t *rowsum,
                       const void *pa, float *y, int ldy, const I8NextMinMax *mm, int *nparts, const I8NextBytes *nb,
                       int off_shift) {
  const I8Args p = i8_args(L, a, lda, m, rowsum, pa, y, ldy, mm, nb, off_shift);
  const int v = i8_gemm_variant();
  // every tile here is at least 128 x 128 with at most 8 waves, as
  // i8_gemm_parts assumes: i8_launch's static_assert
  switch (v) {
    case 0: return i8_launch<I8Tile<IBM, IBN, 2, 2, IBK>>(s, gemm_i8_nnet_kernel, p, nparts);
    case 10: return i8_launch<I8Tile<128, 128, 2, 2>>(s, gemm_i8_reg_kernel<128, 128, 2, 2>, p, nparts);
    case 11: return i8_launch<I8Tile<256, 128, 4, 2>>(s, gemm_i8_reg_kernel<256, 128, 4, 2>, p, nparts);
    case 15: return launch_glds<256, 128, 3, 4, 2>(s, p, nparts);
    case 17: return i8_launch<I8Tile<256, 128, 4, 2>>(s, gemm_i8_pipe_kernel<256, 128, 3, 4, 2, true>, p, nparts);
    // 256-wide column tiles on 64-byte K-tiles (half the L2 bytes per MFMA of
    // 15), 4 / 3 stages; 44: 15's tile on them
    case 40: return launch_glds<256, 256, 4, 4, 2, 64>(s, p, nparts);
    case 41: return launch_glds<256, 256, 3, 4, 2, 64>(s, p, nparts);
    case 44: return launch_glds<256, 128, 4, 4, 2, 64>(s, p, nparts);
#ifdef CATEARS_DIAG
    // timing-only ablations of 15 (wrong results): 60 + DIAG
    case 61: return launch_glds<256, 128, 3, 4, 2, 128, 1>(s, p, nparts);
    case 62: return launch_glds<256, 128, 3, 4, 2, 128, 2>(s, p, nparts);
    case 63: return launch_glds<256, 128, 3, 4, 2, 128, 3>(s, p, nparts);
    case 64: return launch_glds<256, 128, 3, 4, 2, 128, 4>(s, p, nparts);
    case 65: return launch_glds<256, 128, 3, 4, 2, 128, 5>(s, p, nparts);
    case 68: return launch_glds<256, 128, 3, 4, 2, 128, 8>(s, p, nparts);
    case 71: return launch_glds<256, 128, 3, 4, 2, 128, 11>(s, p, nparts);
#endif
    default:
      return fail(CE_GPU_EINVAL, "int8 GEMM variant " + std::to_string(v) +
                                     " is not in this build (the experiments library carries 0, 10, 11, 15-17, 40, "
                                     "41, 44)");
  }
}

}  // namespace catears
#endif  // CATEARS_EXPERIMENTS
