// gemm_bf16x6_exp.hip -- the bf16x6 GEMM's measurement variants: what the
// experiments library (`make EXPERIMENTS=1`, libcatears_hip_exp.so) carries
// beside the product dispatch of gemm_bf16x6.hip.  The product object of this
// file is empty.
//
//   * the fp32-operand kernel `f` (variants 40 and 160: the weights split in
//     the kernel, no fragment image) and the warp-specialised `ws` (200);
//   * the CATEARS_X6_VARIANT table over them and over other tiles of the
//     product's `d` and `w` kernels (300, 500-503, 505, 507, 508);
//   * the d kernel's KS = 2, 256-unit FIRST and plane-chain (PIN / OUT16)
//     instantiations: CATEARS_X6_KS, CATEARS_X6_FIRST_TILE, CATEARS_X6_CHAIN;
//   * CATEARS_X6W_GROUP, the w kernel's XCD tile group;
//   * the DIAG ablations 310-316 of d (wrong results, timing only).
// All but the ablations give the product's bits (tests/test_gpu_x6_variants.py).
// Schedules that were measured slower and then removed are recorded with
// their numbers in DESIGN.md §8 and profiles/.
#ifdef CATEARS_EXPERIMENTS
#include <string>

#include "../gemm_bf16x6_kernels.h"

namespace catears {
namespace {

// fp32-in schedule: operands stay fp32 in HBM (4 B per element instead of
// the planes' 6) and are split into the three bf16 planes on their way into
// LDS.  The plane kernel (gemm_bf16x6q_kernel) is bound by the bytes the L2
// can move into LDS (f16x3's 4 B per element runs at 6/4 of its fp32-FLOP rate
// with half the MFMA work), so the fill carries fp32 and the VALU pays for the
// split, interleaved with the MFMAs.  Per K-tile each thread loads 8
// consecutive floats of one weight row and of one activation row (one 128-B
// line per row across 4 threads; global_load_dwordx4 x 2), splits them with
// the same split3 as the epilogue (so the planes -- and the results -- are
// bit-identical to the plane path), and writes 16 B per plane with
// ds_write_b128 into the layout the fragment reads expect.  Two LDS stages,
// registers one tile ahead:
//   step kt: write tile kt+1 (loaded during step kt-1) into stage (kt+1) % 2,
//            load tile kt+2 into registers, fragment reads + MFMAs of stage
//            kt % 2, lgkmcnt(0), raw s_barrier (no vmcnt: the loads stay in
//            flight across it).
//   WAR: stage (kt+1) % 2 was read in step kt-1, whose reads all fed MFMAs
//        before that step's barrier.  RAW: the writes of tile kt+1 are
//        drained before step kt's barrier; step kt+1 reads after it.
// Tiles past the end are clamped to the last one (written to a stage no
// later step reads), so the body is one basic block.
// SCHED: 0 = split of tile kt+1 before the MFMAs of tile kt (round 1);
// 8 = MFMAs first in explicit regions (the round-2 default).
template <class C, int SCHED>
__global__ __launch_bounds__(C::NT, 1) void gemm_bf16x6f_kernel(X6Args p) {
  constexpr int BW = C::BW, BF = C::BF, TW = C::TW, TF = C::TF, NT = C::NT, STAGE = C::STAGE;
  static_assert(SCHED == 0 || SCHED == 8, "the schedules that remain");
  constexpr int RPP = NT / 4;  // rows per pass (4 threads x 32 B per row)
  static_assert(BW % RPP == 0 && BF % RPP == 0, "rows per pass");
  constexpr int NPW = BW / RPP, NPX = BF / RPP;
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];
  auto swz = [](int row) { return ((row >> 3) & 1) << 1; };
  typedef float f32x4v __attribute__((ext_vector_type(4)));
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ww = wave / C::WGF, wf = wave % C::WGF;
  int tm, tn;
  tile_of(blockIdx.x, p.tiles_m, p.tiles_n, p.group, &tm, &tn);
  const int f0 = tm * BF, n0 = tn * BW;
  const int prow = tid >> 2, pch = tid & 3;

  typedef const __attribute__((address_space(1))) f32x4v gvec;
  uint32_t wsrc[NPW];  // float offset of this thread's weight row at k = 0
#pragma unroll
  for (int i = 0; i < NPW; ++i) wsrc[i] = (uint32_t)(min(n0 + prow + i * RPP, p.n - 1) * p.ldw + 8 * pch);
  const int kbeg = 0, ktiles = p.kpad / 32;
  f32x4v rw0[NPW], rw1[NPW], rx0[NPX], rx1[NPX];
  auto load = [&](int kt) {
    kt = min(kt, ktiles - 1);
    const int k0 = kt * 32;
    const int seg = k0 / p.din, col0 = k0 - seg * p.din;
    const int shift = (int)(signed char)(p.off_packed >> (8 * seg));
    gvec *wb = (gvec *)(p.wf + k0);
#pragma unroll
    for (int i = 0; i < NPW; ++i) {
      rw0[i] = wb[wsrc[i] / 4];
      rw1[i] = wb[wsrc[i] / 4 + 1];
    }
    gvec *xb = (gvec *)(p.xf + col0 + 8 * pch);
#pragma unroll
    for (int i = 0; i < NPX; ++i) {
      const int src = clampi(f0 + prow + i * RPP + shift, 0, p.m - 1);
      const uint32_t o = (uint32_t)(src * p.ldx) / 4;
      rx0[i] = xb[o];
      rx1[i] = xb[o + 1];
    }
  };
  // 8 floats -> three 16-B plane chunks at row r of the plane block `base`
  auto put = [&](char *base, int nrows, int r, f32x4v v0, f32x4v v1) {
    const Planes2 q0 = split3_pair(v0.x, v0.y), q1 = split3_pair(v0.z, v0.w);
    const Planes2 q2 = split3_pair(v1.x, v1.y), q3 = split3_pair(v1.z, v1.w);
    const int off = r * 64 + ((pch ^ swz(r)) * 16);
    *reinterpret_cast<u32x4 *>(base + off) = u32x4{q0.h, q1.h, q2.h, q3.h};
    *reinterpret_cast<u32x4 *>(base + nrows * 64 + off) = u32x4{q0.m, q1.m, q2.m, q3.m};
    *reinterpret_cast<u32x4 *>(base + 2 * nrows * 64 + off) = u32x4{q0.l, q1.l, q2.l, q3.l};
  };
  auto store = [&](int kt) {
    char *st = smem + (kt & 1) * STAGE;
#pragma unroll
    for (int i = 0; i < NPW; ++i) put(st, BW, prow + i * RPP, rw0[i], rw1[i]);
#pragma unroll
    for (int i = 0; i < NPX; ++i) put(st + 3 * BW * 64, BF, prow + i * RPP, rx0[i], rx1[i]);
  };

  const int foff = (lane & 15) * 64 + (((lane >> 4) ^ (((lane >> 3) & 1) << 1)) * 16);
  const int wrow = ww * TW * 16, frow = wf * TF * 16;
  f32x4 acc[TW][TF];
#pragma unroll
  for (int i = 0; i < TW; ++i)
#pragma unroll
    for (int j = 0; j < TF; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  load(kbeg);
  store(kbeg);
  load(kbeg + 1);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if constexpr (SCHED == 8) {
    // The MFMAs of tile kt first, then the split of tile kt+1.  Same barrier
    // count and LDS protocol as the SCHED 0 loop:
    //   WAR: stage (kt+1) % 2 was last read in tile kt-1, before the
    //        barrier that closed it;
    //   RAW: every wave's writes of stage kt+1 precede the barrier that
    //        closes tile kt.
    bf16x8 a[3][TW], b[3][TF];
    // Region-scheduled loop (sched_barrier between regions; the compiler
    // interleaves inside each): plane 0 and 1 fragment reads + the 16
    // plane-0 MFMAs + the weight-row split of tile kt+1 and the weight
    // loads of tile kt+2 | half the plane-1 MFMAs + activation row 0's
    // split and loads | the other half + row 1 + plane-2 reads | the 32
    // plane-2 MFMAs.  Each load is issued as soon as the split has freed
    // its registers, about one iteration before its data is split.
    static_assert(NPW == 1 && NPX == 2 && TW % 2 == 0, "SCHED 8 geometry");
    auto read_plane = [&](const char *st, int pl) {
#pragma unroll
      for (int i = 0; i < TW; ++i)
        a[pl][i] = *reinterpret_cast<const bf16x8 *>(st + (pl * BW + wrow + i * 16) * 64 + foff);
#pragma unroll
      for (int j = 0; j < TF; ++j)
        b[pl][j] = *reinterpret_cast<const bf16x8 *>(st + 3 * BW * 64 + (pl * BF + frow + j * 16) * 64 + foff);
    };
    auto kpos = [&](int kt, int *k0, int *col0, int *shift) {
      kt = min(kt, ktiles - 1);
      *k0 = kt * 32;
      const int seg = *k0 / p.din;
      *col0 = *k0 - seg * p.din;
      *shift = (int)(signed char)(p.off_packed >> (8 * seg));
    };
    auto load_w = [&](int kt) {
      int k0, col0, shift;
      kpos(kt, &k0, &col0, &shift);
      gvec *wb = (gvec *)(p.wf + k0);
      rw0[0] = wb[wsrc[0] / 4];
      rw1[0] = wb[wsrc[0] / 4 + 1];
    };
    auto load_x = [&](int kt, int i) {
      int k0, col0, shift;
      kpos(kt, &k0, &col0, &shift);
      gvec *xb = (gvec *)(p.xf + col0 + 8 * pch);
      const int src = clampi(f0 + prow + i * RPP + shift, 0, p.m - 1);
      const uint32_t o = (uint32_t)(src * p.ldx) / 4;
      rx0[i] = xb[o];
      rx1[i] = xb[o + 1];
    };
    for (int kt = 0; kt < ktiles; ++kt) {
      const char *st = smem + (kt & 1) * STAGE;
      char *sn = smem + ((kt + 1) & 1) * STAGE;
      read_plane(st, 0);
      read_plane(st, 1);
#pragma unroll
      for (int i = 0; i < TW; ++i)
#pragma unroll
        for (int j = 0; j < TF; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][i], b[0][j], acc[i][j], 0, 0, 0);
      put(sn, BW, prow, rw0[0], rw1[0]);
      load_w(kt + 2);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = h * TW / 2; i < (h + 1) * TW / 2; ++i)
#pragma unroll
          for (int j = 0; j < TF; ++j) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][i], b[1][j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1][i], b[0][j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1][i], b[1][j], acc[i][j], 0, 0, 0);
          }
        put(sn + 3 * BW * 64, BF, prow + h * RPP, rx0[h], rx1[h]);
        load_x(kt + 2, h);
        if (h == 1) read_plane(st, 2);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int i = 0; i < TW; ++i)
#pragma unroll
        for (int j = 0; j < TF; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][i], b[2][j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2][i], b[0][j], acc[i][j], 0, 0, 0);
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    x6_epilogue<TW, TF, false>(p, acc, n0 + wrow, f0 + frow, lane);
    return;
  }
  for (int kt = kbeg; kt < ktiles; ++kt) {
    store(kt + 1);
    load(kt + 2);
    const char *st = smem + (kt & 1) * STAGE;
    bf16x8 a[3][TW], b[3][TF];
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
      for (int i = 0; i < TW; ++i)
        a[pl][i] = *reinterpret_cast<const bf16x8 *>(st + (pl * BW + wrow + i * 16) * 64 + foff);
#pragma unroll
      for (int j = 0; j < TF; ++j)
        b[pl][j] = *reinterpret_cast<const bf16x8 *>(st + 3 * BW * 64 + (pl * BF + frow + j * 16) * 64 + foff);
    }
#pragma unroll
    for (int i = 0; i < TW; ++i)
#pragma unroll
      for (int j = 0; j < TF; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][i], b[0][j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < TW; ++i)
#pragma unroll
      for (int j = 0; j < TF; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][i], b[1][j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1][i], b[0][j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1][i], b[1][j], acc[i][j], 0, 0, 0);
      }
#pragma unroll
    for (int i = 0; i < TW; ++i)
#pragma unroll
      for (int j = 0; j < TF; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][i], b[2][j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2][i], b[0][j], acc[i][j], 0, 0, 0);
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  x6_epilogue<TW, TF, false>(p, acc, n0 + wrow, f0 + frow, lane);
}

// Warp-specialised fp32-in schedule: the block is C::NW MFMA waves plus
// NPV producer waves.  The producers do all the global loads, splits and
// plane writes of tile kt+1 while the MFMA waves read and multiply tile kt,
// so the split VALU issues in the cycles the matrix pipe leaves free on the
// same SIMD instead of between a wave's own MFMAs.  Same LDS stages, layout,
// product order and per-K-tile barrier as gemm_bf16x6f_kernel's SCHED 0 loop
// (bit-identical results):
//   WAR: stage (kt+1) % 2 was read in step kt-1, whose reads were drained
//        (lgkmcnt(0)) before the barrier closing it;
//   RAW: the producers' writes of tile kt+1 are drained before the barrier
//        closing step kt, and the MFMA waves read them after it.
// Both roles pass the same number of barriers (one prologue + one per K-tile;
// the role test is wave-uniform, readfirstlane).  Producer rows: the stage's
// BW weight rows then BF activation rows, 4 threads x 32 B per row, pass i
// covering rows i RPP .. i RPP + RPP - 1 (a pass may straddle the two kinds:
// per-thread selects).  Measured against the default: DESIGN.md §8.
template <class C, int NPV>
__global__ __launch_bounds__(C::NT + 64 * NPV, 1) void gemm_bf16x6ws_kernel(X6Args p) {
  constexpr int BW = C::BW, BF = C::BF, TW = C::TW, TF = C::TF, NT = C::NT, STAGE = C::STAGE;
  constexpr int RPP = 16 * NPV;  // producer rows per pass
  static_assert((BW + BF) % RPP == 0, "rows per pass");
  constexpr int NP = (BW + BF) / RPP;
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];
  auto swz = [](int row) { return ((row >> 3) & 1) << 1; };
  typedef float f32x4v __attribute__((ext_vector_type(4)));
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef const __attribute__((address_space(1))) f32x4v gvec;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int tm, tn;
  tile_of(blockIdx.x, p.tiles_m, p.tiles_n, p.group, &tm, &tn);
  const int f0 = tm * BF, n0 = tn * BW;
  const int ktiles = p.kpad / 32;

  if (wave >= C::NW) {  // producer
    const int pt = tid - NT, prow = pt >> 2, pch = pt & 3;
    bool isw[NP];
    int trow[NP];         // row within its plane block
    uint32_t wsrc[NP];    // weight rows: float offset at k = 0
    int dst[NP];          // byte offset of the chunk in the stage
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int r = i * RPP + prow;
      isw[i] = BW % RPP == 0 ? i < BW / RPP : r < BW;  // compile-time when no pass straddles
      trow[i] = isw[i] ? r : r - BW;
      wsrc[i] = (uint32_t)(min(n0 + trow[i], p.n - 1) * p.ldw + 8 * pch);
      dst[i] = (isw[i] ? 0 : 3 * BW * 64) + trow[i] * 64 + ((pch ^ swz(trow[i])) * 16);
    }
    f32x4v r0[NP], r1[NP];
    auto load = [&](int kt) {
      kt = min(kt, ktiles - 1);
      const int k0 = kt * 32;
      const int seg = k0 / p.din, col0 = k0 - seg * p.din;
      const int shift = (int)(signed char)(p.off_packed >> (8 * seg));
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        gvec *src;
        if (isw[i]) {
          src = (gvec *)(p.wf + k0 + wsrc[i]);
        } else {
          const int x = clampi(f0 + trow[i] + shift, 0, p.m - 1);
          src = (gvec *)(p.xf + (uint32_t)(x * p.ldx) + col0 + 8 * pch);
        }
        r0[i] = src[0];
        r1[i] = src[1];
      }
    };
    auto store = [&](int kt) {
      char *st = smem + (kt & 1) * STAGE;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const f32x4v v0 = r0[i], v1 = r1[i];
        const Planes2 q0 = split3_pair(v0.x, v0.y), q1 = split3_pair(v0.z, v0.w);
        const Planes2 q2 = split3_pair(v1.x, v1.y), q3 = split3_pair(v1.z, v1.w);
        const int ps = (isw[i] ? BW : BF) * 64;  // plane stride in the stage
        char *d = st + dst[i];
        *reinterpret_cast<u32x4 *>(d) = u32x4{q0.h, q1.h, q2.h, q3.h};
        *reinterpret_cast<u32x4 *>(d + ps) = u32x4{q0.m, q1.m, q2.m, q3.m};
        *reinterpret_cast<u32x4 *>(d + 2 * ps) = u32x4{q0.l, q1.l, q2.l, q3.l};
      }
    };
    load(0);
    store(0);
    load(1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int kt = 0; kt < ktiles; ++kt) {
      store(kt + 1);  // past the end: the clamped last tile into a stage no step reads
      load(kt + 2);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return;
  }

  // MFMA waves
  const int ww = wave / C::WGF, wf = wave % C::WGF;
  const int foff = (lane & 15) * 64 + (((lane >> 4) ^ (((lane >> 3) & 1) << 1)) * 16);
  const int wrow = ww * TW * 16, frow = wf * TF * 16;
  f32x4 acc[TW][TF];
#pragma unroll
  for (int i = 0; i < TW; ++i)
#pragma unroll
    for (int j = 0; j < TF; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  __builtin_amdgcn_s_barrier();
  for (int kt = 0; kt < ktiles; ++kt) {
    const char *st = smem + (kt & 1) * STAGE;
    bf16x8 a[3][TW], b[3][TF];
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
      for (int i = 0; i < TW; ++i)
        a[pl][i] = *reinterpret_cast<const bf16x8 *>(st + (pl * BW + wrow + i * 16) * 64 + foff);
#pragma unroll
      for (int j = 0; j < TF; ++j)
        b[pl][j] = *reinterpret_cast<const bf16x8 *>(st + 3 * BW * 64 + (pl * BF + frow + j * 16) * 64 + foff);
    }
#pragma unroll
    for (int i = 0; i < TW; ++i)
#pragma unroll
      for (int j = 0; j < TF; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][i], b[0][j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < TW; ++i)
#pragma unroll
      for (int j = 0; j < TF; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][i], b[1][j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1][i], b[0][j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1][i], b[1][j], acc[i][j], 0, 0, 0);
      }
#pragma unroll
    for (int i = 0; i < TW; ++i)
#pragma unroll
      for (int j = 0; j < TF; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][i], b[2][j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2][i], b[0][j], acc[i][j], 0, 0, 0);
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  x6_epilogue<TW, TF, false>(p, acc, n0 + wrow, f0 + frow, lane);
}

// --------------------------------------------------------- the switches --

// CATEARS_X6_VARIANT: the schedule of the fp32-activation bf16x6 GEMM.
//   0    the product's dispatch (gemm_bf16x6.hip)
//   300  d on 256 x 128 tiles for every layer after the first (the rounds 3-5
//        default)
//   160  f, region-scheduled on 128 x 256 tiles (the round-2 default)
//   40   f on 128 x 128 tiles
//   200  ws: 4 MFMA waves (64 x 64 each) + 4 producer waves on 128 x 128
//   500-503, 505, 507, 508  w on other tiles (below)
//   310-316  ablations of 300 (wrong results, timing only)
// Any other value makes every fp32-activation launch fail with CE_GPU_EINVAL.
int x6_variant() {
  static int v = CE_KNOB("CATEARS_X6_VARIANT", 0);
  return v;
}

// CATEARS_X6_KS: K-tiles per LDS stage of the direct-weight kernel's hidden
// layers (1 or 2; same bits).  Measured (tools/experiments/gpu_r5e.sh, one
// box, alternating): two per stage is 2 % slower -- serial hidden layer 158.5
// vs 155.6 us, C3 at the driver's flags 6.36-6.38 vs 6.40-6.46 M frames/s --
// so one stays the default; the barrier is not what the loop waits on.
int x6_ks() {
  static int v = CE_KNOB("CATEARS_X6_KS", 1);
  return v;
}

// CATEARS_X6_FIRST_TILE: unit width of the gathered first layer's tiles.
// 128 (default): 256 blocks for a 4072-row batch instead of 128, 26.5 ->
// 20.9 us per launch in a serial run (r4c); 256: the hidden layers' tiles.
// Same bits either way (tests/test_gpu_x6_variants.py).
int x6_first_tile() {
  static int v = CE_KNOB("CATEARS_X6_FIRST_TILE", 128);
  return v;
}

// CATEARS_X6W_GROUP forces one XCD tile group for the w kernel (0: the
// product's rule, x6w_group)
int x6w_group_forced() {
  static int v = CE_KNOB("CATEARS_X6W_GROUP", 0);
  return v;
}

// ------------------------------------------------------------- launches --

// d on C's tiles, the instantiation the operands ask for: the gathered first
// layer, planes in and / or out (the plane chain), two K-tiles per stage
template <class C, int DIAG = 0>
int launch_d(hipStream_t s, const X6Args &p) {
  const bool out16 = p.y16 != nullptr;
  void (*k)(X6Args);
  if (p.row_map || p.din % 32 != 0)  // the same rule as launch_gemm_bf16x6's `first`
    k = out16 ? gemm_bf16x6d_kernel<C, true, 0, 1, false, true> : gemm_bf16x6d_kernel<C, true>;
  else if (!p.xf)  // plane input
    k = out16 ? gemm_bf16x6d_kernel<C, false, 0, 1, true, true> : gemm_bf16x6d_kernel<C, false, 0, 1, true, false>;
  else if (out16)  // fp32 input, planes out (a chain's whole-K-tile first layer)
    k = gemm_bf16x6d_kernel<C, false, 0, 1, false, true>;
  else if (x6_ks() == 2 && (p.kpad / 32) % 2 == 0)
    k = gemm_bf16x6d_kernel<C, false, DIAG, 2>;
  else
    k = gemm_bf16x6d_kernel<C, false, DIAG>;
  return x6_launch<C>(s, k, p);
}

// w on C's tiles; d on 256 x 128 where w cannot run the layer (x6w_fits)
template <class C, bool SG = false>
int launch_w(hipStream_t s, X6Args p, int min_tiles = 0) {
  if (!x6w_fits<C>(p, min_tiles)) return launch_d<X6D256>(s, p);
  p.group = x6w_group_forced() > 0 ? x6w_group_forced() : x6w_group((p.n + C::BW - 1) / C::BW);
  return x6_launch<C>(s, gemm_bf16x6w_kernel<C, SG>, p);
}

}  // namespace

bool x6_exp_takes(const X6Gemm &a) {
  const bool chain = a.wd && (!a.xf || a.y16);  // planes in or out of the d kernel
  if (!a.xf && !chain) return false;            // plane operands: the product's q kernel
  return chain || x6_variant() != 0 || x6_ks() != 1 || x6_first_tile() != 128 || x6w_group_forced() != 0;
}

int launch_gemm_bf16x6_exp(hipStream_t s, const X6Gemm &a) {
  X6Args p;
  CE_TRY(x6_args(a, &p));
  const int v = x6_variant();
  const bool first = a.row_map != nullptr || a.din % 32 != 0, f32in = a.xf != nullptr;
  if (first && v != 0 && v != 300 && (v < 310 || v > 316))
    return fail(CE_GPU_EINVAL, "gemm_bf16x6: a gathered first layer needs fp32 input and the direct-weight kernel");
  const bool image = a.wd && a.wd_kt * 32 >= a.kpad && (reinterpret_cast<uintptr_t>(a.wd) & 15) == 0;
  const bool d128 = a.wide || (first && x6_first_tile() == 128);
  if (!f32in || a.y16) {  // the plane chain (nnet_programs.cc, CATEARS_X6_CHAIN)
    const bool direct = a.wd && (v == 0 || v == 300);
    if (!f32in && (!direct || first || a.ldx % 8 || a.px % 8 || (reinterpret_cast<uintptr_t>(a.x) & 15) ||
                   (int64_t)a.m * a.ldx >= ((int64_t)1 << 31) || (int64_t)a.m * a.ldy >= ((int64_t)1 << 31)))
      return fail(CE_GPU_EINVAL, "gemm_bf16x6: plane input needs the direct-weight kernel, din % 32 == 0, "
                                 "16-byte aligned planes and 2^31-element operands");
    if (!direct) return fail(CE_GPU_EINVAL, "gemm_bf16x6: fp32 input with split output needs the direct-weight kernel");
    if (!image) return fail(CE_GPU_EINVAL, "gemm_bf16x6: weight fragment image does not cover K");
    return d128 ? launch_d<X6D128>(s, p) : launch_d<X6D256>(s, p);
  }
  if (v != 40 && v != 160 && v != 200 && !image)
    return fail(CE_GPU_EINVAL, "gemm_bf16x6: schedule " + std::to_string(v) + " needs the weight fragment image");
  switch (v) {
    case 0:    // the product's dispatch, under the other switches
    case 300:  // ... without the w kernel
      if (d128) return launch_d<X6D128>(s, p);
      if (v == 0 && !first) return launch_w<X6W512, true>(s, p, kX6WideMinTiles);
      return launch_d<X6D256>(s, p);
    case 160:
      return x6_launch<X6Cfg<128, 256, 2, 4, 2>>(s, gemm_bf16x6f_kernel<X6Cfg<128, 256, 2, 4, 2>, 8>, p);
    case 40:  // fills all CUs on a 1024-wide layer (one batch at a time on an idle GPU)
      return x6_launch<X6Cfg<128, 128, 4, 2, 2>>(s, gemm_bf16x6f_kernel<X6Cfg<128, 128, 4, 2, 2>, 0>, p);
    case 200: {
      using C = X6Cfg<128, 128, 2, 2, 2>;
      return x6_launch<C>(s, gemm_bf16x6ws_kernel<C, 4>, p, C::NT + 64 * 4);
    }
    case 500:  // one wave per SIMD: 512 x 128 tiles, 4 waves of 128 units x 128 frames
    case 501:  // 512 x 64, 4 waves of 128 x 64
    case 502:  // 256 x 128, 4 waves of 64 x 128
    case 503:  // 256 x 256, 2 x 2 waves of 128 x 128
    case 505:  // 501 with the interleave pinned (sched_group_barrier)
    case 507:  // 502 with the interleave pinned
    case 508:  // 512 x 128 as 8 waves (two per SIMD) of 128 units x 64 frames, pinned: the product's
      if (first || a.wide) return launch_d<X6D128>(s, p);
      return v == 500   ? launch_w<W6Cfg<512, 128, 4, 1>>(s, p)
             : v == 501 ? launch_w<W6Cfg<512, 64, 4, 1>>(s, p)
             : v == 502 ? launch_w<W6Cfg<256, 128, 4, 1>>(s, p)
             : v == 503 ? launch_w<W6Cfg<256, 256, 2, 2>>(s, p)
             : v == 505 ? launch_w<W6Cfg<512, 64, 4, 1>, true>(s, p)
             : v == 507 ? launch_w<W6Cfg<256, 128, 4, 1>, true>(s, p)
                        : launch_w<X6W512, true>(s, p);
#ifdef CATEARS_DIAG
    // ablations of the direct-weight 300 (layers 2-7; wrong results, timing
    // only): 310 no split, 311 no activation stage writes, 312 no activation
    // path, 313 no weight loads, 314 no barrier, 315 no MFMAs, 316 MFMAs only
    case 310: return first ? launch_d<X6D128>(s, p) : launch_d<X6D256, 1>(s, p);
    case 311: return first ? launch_d<X6D128>(s, p) : launch_d<X6D256, 2>(s, p);
    case 312: return first ? launch_d<X6D128>(s, p) : launch_d<X6D256, 6>(s, p);
    case 313: return first ? launch_d<X6D128>(s, p) : launch_d<X6D256, 8>(s, p);
    case 314: return first ? launch_d<X6D128>(s, p) : launch_d<X6D256, 16>(s, p);
    case 315: return first ? launch_d<X6D128>(s, p) : launch_d<X6D256, 32>(s, p);
    case 316: return first ? launch_d<X6D128>(s, p) : launch_d<X6D256, 2 | 4 | 8 | 16>(s, p);
#endif
    default:
      return fail(CE_GPU_EINVAL, "bf16x6 schedule " + std::to_string(v) + " is not in the experiments library");
  }
}

}  // namespace catears
#endif  // CATEARS_EXPERIMENTS

