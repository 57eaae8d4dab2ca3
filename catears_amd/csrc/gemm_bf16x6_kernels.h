// gemm_bf16x6_kernels.h -- the device side that the bf16x6 GEMM's two
// translation units both instantiate: kernels/gemm_bf16x6.hip (what the
// product runs; the scheme and the layouts are described there) and
// kernels/gemm_bf16x6_exp.hip (the experiments library's schedules and
// ablations).  The kernel arguments, the tile configurations, the epilogue,
// the direct-weight kernel `d`, the one-wave-per-SIMD kernel `w` and their
// launch helper.  Everything is in the unnamed namespace: each translation
// unit compiles its own instantiations.
#pragma once

#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "bf16_split.h"
#include "internal.h"
#include "lds_dma.h"
#include "tile_order.h"

// measurement builds (X6FLAGS): non-temporal output stores
#ifndef CATEARS_X6_NT
#define CATEARS_X6_NT 0
#endif

namespace catears {

// kernels/gemm_bf16x6_exp.hip, the experiments library only: whether a launch
// is its dispatcher's (a CATEARS_X6_* switch off its default, or the plane
// chain's operands), and that dispatcher, for arguments launch_gemm_bf16x6
// has checked.
bool x6_exp_takes(const X6Gemm &a);
int launch_gemm_bf16x6_exp(hipStream_t s, const X6Gemm &a);

namespace {

using dma::clampi;
using dma::glds16;
using dma::wait_vmcnt;
using split::Planes2;
using split::split3;
using split::split3_pair;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// The kernel arguments (the field order is the kernarg layout).
struct X6Args {
  const uint16_t *w;  // weights, n x ldw, plane stride pw (elements)
  const uint16_t *x;  // activations, rows x ldx, plane stride px
  const float *wf, *xf;  // or fp32 operands (gemm_bf16x6f_kernel; ldw / ldx in floats)
  const float *bias, *bn_scale, *bn_offset;
  float *y32;         // fp32 output (ldy floats per row), or
  uint16_t *y16;      // split output (ldy elements per row, plane stride py)
  int ldw, pw, ldx, px, ldy, py;
  int m, n, kpad, din;
  uint64_t off_packed;  // splice offset of segment s in signed byte s
  int post[4];
  int npost, post_mode;
  int tiles_m, tiles_n, group;
  const uint16_t *wd;  // weights as MFMA A fragments (gemm_bf16x6d_kernel), see X6Gemm::wd
  int wd_kt;           // K-tiles per 16-unit block in that image
  // first layer read straight from the caller's rows (gemm_bf16x6d_kernel
  // FIRST): nseg segments of din (a multiple of 8) floats, segment s of
  // packed row r = xf row row_map[clamp(r + off[s])]; zeros past them
  const int *row_map;
  int nseg;
};

template <int BW_, int BF_, int WGW_, int WGF_, int STAGES_>
struct X6Cfg {
  static constexpr int BW = BW_, BF = BF_, WGW = WGW_, WGF = WGF_, STAGES = STAGES_;
  static constexpr int NW = WGW * WGF, NT = 64 * NW;
  static constexpr int TW = BW / WGW / 16, TF = BF / WGF / 16;  // 16 x 16 fragments per wave
  static constexpr int QW = 3 * BW / 16, QF = 3 * BF / 16;       // DMA instructions per stage
  static constexpr int NQW = QW / NW, NQF = QF / NW;
  static constexpr int NQM = (QW + QF) / NW;                      // pieces per wave, mixed
  static constexpr int STAGE = 3 * (BW + BF) * 64;                // bytes per stage
  static_assert(TW >= 1 && TF >= 1 && (QW + QF) % NW == 0, "bad bf16x6 tile");
  static_assert(STAGES == 2 || STAGES == 3, "2 or 3 LDS stages");
  static_assert(STAGES * STAGE <= 160 * 1024, "LDS");
};

// Epilogue: lane holds units n .. n+3 of frame f for each fragment pair.
// + bias, post chain in model order with the reference's roundings; an
// absent bias adds -0 (identity).  Requires n % 4 == 0 (host-checked).
template <int TW, int TF, bool OUT16>
__device__ __forceinline__ void x6_epilogue(const X6Args &p, const f32x4 (&acc)[TW][TF], int nw0, int fw0, int lane) {
  with_post_mode(p.post_mode, [&](auto M) {
#pragma unroll
    for (int i = 0; i < TW; ++i) {
      const int n = nw0 + i * 16 + 4 * (lane >> 4);
      if (n >= p.n) continue;
      const f32x4 bias = p.bias ? *reinterpret_cast<const f32x4 *>(p.bias + n) : f32x4{-0.0f, -0.0f, -0.0f, -0.0f};
      const f32x4 sc = p.bn_scale ? *reinterpret_cast<const f32x4 *>(p.bn_scale + n) : f32x4{1.0f, 1.0f, 1.0f, 1.0f};
      const f32x4 of = p.bn_offset ? *reinterpret_cast<const f32x4 *>(p.bn_offset + n) : f32x4{-0.0f, -0.0f, -0.0f, -0.0f};
#pragma unroll
      for (int j = 0; j < TF; ++j) {
        const int f = fw0 + j * 16 + (lane & 15);
        if (f >= p.m) continue;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = apply_post<decltype(M)::value>(acc[i][j][e] + bias[e], sc[e], of[e], p.post, p.npost);
        if constexpr (OUT16) {
          uint16_t h[4], m[4], l[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) split3(v[e], &h[e], &m[e], &l[e]);
          uint16_t *dst = p.y16 + (int64_t)f * p.ldy + n;
          typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));
          *reinterpret_cast<u16x4 *>(dst) = u16x4{h[0], h[1], h[2], h[3]};
          *reinterpret_cast<u16x4 *>(dst + p.py) = u16x4{m[0], m[1], m[2], m[3]};
          *reinterpret_cast<u16x4 *>(dst + 2 * p.py) = u16x4{l[0], l[1], l[2], l[3]};
        } else {
#if CATEARS_X6_NT
          // measurement build (X6FLAGS=-DCATEARS_X6_NT=1): non-temporal output stores
          __builtin_nontemporal_store(v, reinterpret_cast<f32x4 *>(p.y32 + (int64_t)f * p.ldy + n));
#else
          *reinterpret_cast<f32x4 *>(p.y32 + (int64_t)f * p.ldy + n) = v;
#endif
        }
      }
    }
  });
}

// Direct-weight schedule (the default): the constant weights are split into
// their three bf16 planes once, at model load, and stored in the order the
// MFMA reads its A operand (X6Gemm::wd: per 16-unit block, K-tile and plane
// one contiguous 1 KB fragment, lane l's 16 bytes at 16 l).  Each wave loads
// its weight fragments straight from L2 into registers with one
// global_load_dwordx4 per fragment -- no split VALU, no LDS write and no LDS
// read for the weights -- so LDS carries only the activations, split once per
// block on their way in (as gemm_bf16x6f_kernel does).  Per K-tile and CU
// that removes 2/3 of the ds_write_b128 traffic, half the fragment reads and
// 2/3 of the split VALU of the fp32-operand kernel, whose ablations placed its
// overhead over the bare MFMA loop in exactly that LDS-write path (DESIGN.md
// §8).  Tile: BW = 256 units x BF = 128 frames, 8 waves of 64 x 64 (4 along
// the units, 2 along the frames: each weight fragment is loaded by two waves,
// the second from L1).  Products, their order per output element and the
// planes are those of gemm_bf16x6f_kernel, so results are bit-identical to
// it.  Per K-tile, in order (the weights of tile kt+1 are issued as soon as
// tile kt's registers are free: a0 one tile ahead in a second buffer, a1
// after its last product, a2 at the end of the tile):
//   read b0 b1 (planes 0, 1 of the activations) | load a0 of kt+1 |
//   16 MFMAs a0 b0 | split + write activation tile kt+1, load tile kt+2 |
//   48 MFMAs a0 b1, a1 b0, a1 b1 | read b2 | load a1 of kt+1 |
//   32 MFMAs a0 b2, a2 b0 | load a2 of kt+1 | lgkmcnt(0), barrier.
//   WAR: activation stage (kt+1) % 2 was last read in tile kt-1, before the
//        barrier that closed it; RAW: its writes precede the barrier that
//        closes tile kt.
// DIAG (ablation builds, wrong results, timing only; -DCATEARS_DIAG): bit 1 =
// no split (the fp32 bits written as the planes), 2 = no activation stage
// writes at all, 4 = no activation loads after the prologue, 8 = no weight
// loads after the prologue, 16 = no K-tile barrier, 32 = no MFMAs.
// KS: K-tiles per LDS stage.  KS = 2 holds two K-tiles per stage (96 KB for
// both stages), so the block barrier comes once per two K-tiles; tile t
// lives in sub-stage t & 1 of stage (t >> 1) & 1, tile t + 2 is split and
// written during tile t and loaded during tile t - 1 (one tile more of load
// slack).  Same products in the same order: bit-identical to KS = 1.
// PIN / OUT16 (the plane chain, CATEARS_X6_CHAIN in nnet_programs.cc): the activations
// arrive already split -- three bf16 planes per row, written once by the
// previous layer's OUT16 epilogue -- so the loader moves three 16-byte plane
// chunks per thread into LDS with no split VALU; OUT16 writes this layer's
// output the same way for the next.  The planes are split3's, the loader's
// split3_pair gives the same bits, so the chain is bit-identical to the fp32
// chain.  Each activation is split once instead of once per unit tile that
// reads it (4 per hidden layer, 14 for the output layer).
// The product instantiates DIAG = 0, KS = 1, PIN = OUT16 = false only
// (tests/test_abi.py); the rest are the experiments library's.
template <class C, bool FIRST = false, int DIAG = 0, int KS = 1, bool PIN = false, bool OUT16 = false>
__global__ __launch_bounds__(C::NT, 512 / C::NT) void gemm_bf16x6d_kernel(X6Args p) {  // 8 waves per CU
#ifndef CATEARS_DIAG
  static_assert(DIAG == 0, "ablation builds (wrong results) only with -DCATEARS_DIAG");
#endif
  static_assert(KS == 1 || (KS == 2 && !FIRST), "two K-tiles per stage: hidden layers only (even K-tile count)");
  static_assert(!PIN || (!FIRST && KS == 1 && DIAG == 0), "plane input: hidden / output layers, one K-tile per stage");
  constexpr int BF = C::BF, TW = C::TW, TF = C::TF, NT = C::NT;
  constexpr int RPP = NT / 4;  // activation rows per pass (4 threads x 32 B per row)
  static_assert(BF == RPP, "one activation row chunk per thread");
  constexpr int ASTAGE = 3 * BF * 64;  // bytes: one K-tile of activation planes
  __shared__ __attribute__((aligned(1024))) char smem[2 * KS * ASTAGE];
  auto stage_of = [&](int t) -> char * {
    if constexpr (KS == 1) return smem + (t & 1) * ASTAGE;
    else return smem + ((((t >> 1) & 1) << 1) + (t & 1)) * ASTAGE;
  };
  auto swz = [](int row) { return ((row >> 3) & 1) << 1; };
  typedef float f32x4v __attribute__((ext_vector_type(4)));
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef const __attribute__((address_space(1))) f32x4v gvec;
  typedef const __attribute__((address_space(1))) bf16x8 gfrag;
  typedef const __attribute__((address_space(1))) u32x4 gchunk;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ww = wave / C::WGF, wf = wave % C::WGF;
  int tm, tn;
  tile_of(blockIdx.x, p.tiles_m, p.tiles_n, p.group, &tm, &tn);
  const int f0 = tm * BF, n0 = tn * C::BW;
  const int prow = tid >> 2, pch = tid & 3;
  const int ktiles = p.kpad / 32;

  // weight fragment i of this wave: 16-unit block (n0 + 64 ww + 16 i) / 16
  gfrag *wb[TW];
#pragma unroll
  for (int i = 0; i < TW; ++i)
    wb[i] = (gfrag *)(p.wd + ((size_t)((n0 >> 4) + ww * TW + i) * p.wd_kt * 3 * 64 + lane) * 8);
  auto load_w = [&](int kt, int pl, bf16x8 *dst) {
    if constexpr ((DIAG & 8) != 0) {
      if (kt > 0) return;
    }
    kt = min(kt, ktiles - 1);
#pragma unroll
    for (int i = 0; i < TW; ++i) dst[i] = wb[i][(kt * 3 + pl) * 64];
  };
  f32x4v rx0[2], rx1[2];  // activation row chunks of tiles kt+1 / kt+2 (by parity)
  u32x4 rp[3][2];         // PIN: the three plane chunks of tiles kt+1 / kt+2
  // FIRST: every (segment, tile row)'s source row, gathered once into LDS
  // (a row_map load per K-tile would put a dependent global load in front of
  // every activation load; eight values in registers went to scratch)
  __shared__ int src_tab[FIRST ? 8 * BF : 1];
  if constexpr (FIRST) {
    for (int i = tid; i < 8 * BF; i += NT) {
      const int sg = i / BF, row = i % BF;
      const int shift = (int)(signed char)(p.off_packed >> (8 * min(sg, p.nseg - 1)));
      const int src = clampi(clampi(f0 + row, 0, p.m - 1) + shift, 0, p.m - 1);
      src_tab[i] = p.row_map ? p.row_map[src] : src;
    }
    __syncthreads();
  }
  auto load_x = [&](int kt, int r) {
    if constexpr ((DIAG & 4) != 0) {
      if (kt > 1) return;
    }
    kt = min(kt, ktiles - 1);
    const int k0 = kt * 32;
    if constexpr (FIRST) {
      // the splice (5 x 40 for TDNN-S) and row_map gather of splice_pad,
      // per thread: its 8 k lie in one segment; past the segments, zeros
      // (read from column 0 of a valid row)
      const int k = k0 + 8 * pch, seg = k / p.din, segc = min(seg, p.nseg - 1);
      const int src = src_tab[segc * BF + prow];
      gvec *xb = (gvec *)(p.xf + (size_t)src * p.ldx + (seg < p.nseg ? k - segc * p.din : 0));
      rx0[r] = xb[0];
      rx1[r] = xb[1];
      if (seg >= p.nseg) rx0[r] = rx1[r] = f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    } else if constexpr (PIN) {
      // row src's 8 bf16 at k of each plane: element src * ldx + pl * px + k
      const int seg = k0 / p.din, col0 = k0 - seg * p.din;
      const int shift = (int)(signed char)(p.off_packed >> (8 * seg));
      const int src = clampi(f0 + prow + shift, 0, p.m - 1);
      const uint32_t o = ((uint32_t)(src * p.ldx) + col0 + 8 * pch) / 8, ps = (uint32_t)p.px / 8;
      gchunk *xb = (gchunk *)p.x;
      rp[0][r] = xb[o];
      rp[1][r] = xb[o + ps];
      rp[2][r] = xb[o + 2 * ps];
    } else {
      const int seg = k0 / p.din, col0 = k0 - seg * p.din;
      const int shift = (int)(signed char)(p.off_packed >> (8 * seg));
      gvec *xb = (gvec *)(p.xf + col0 + 8 * pch);
      const int src = clampi(f0 + prow + shift, 0, p.m - 1);
      const uint32_t o = (uint32_t)(src * p.ldx) / 4;
      rx0[r] = xb[o];
      rx1[r] = xb[o + 1];
    }
  };
  auto put = [&](char *st, int r) {
    if constexpr ((DIAG & 2) != 0) return;
    if constexpr (PIN) {
      const int off = prow * 64 + ((pch ^ swz(prow)) * 16);
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<u32x4 *>(st + pl * BF * 64 + off) = rp[pl][r];
      return;
    }
    Planes2 q0, q1, q2, q3;
    if constexpr ((DIAG & 1) != 0) {
      auto raw = [](float a, float b) {
        const uint32_t u = __builtin_bit_cast(uint32_t, a) ^ __builtin_bit_cast(uint32_t, b);
        return Planes2{u, u >> 1, u >> 2};
      };
      q0 = raw(rx0[r].x, rx0[r].y), q1 = raw(rx0[r].z, rx0[r].w);
      q2 = raw(rx1[r].x, rx1[r].y), q3 = raw(rx1[r].z, rx1[r].w);
    } else {
      q0 = split3_pair(rx0[r].x, rx0[r].y), q1 = split3_pair(rx0[r].z, rx0[r].w);
      q2 = split3_pair(rx1[r].x, rx1[r].y), q3 = split3_pair(rx1[r].z, rx1[r].w);
    }
    const int off = prow * 64 + ((pch ^ swz(prow)) * 16);
    *reinterpret_cast<u32x4 *>(st + off) = u32x4{q0.h, q1.h, q2.h, q3.h};
    *reinterpret_cast<u32x4 *>(st + BF * 64 + off) = u32x4{q0.m, q1.m, q2.m, q3.m};
    *reinterpret_cast<u32x4 *>(st + 2 * BF * 64 + off) = u32x4{q0.l, q1.l, q2.l, q3.l};
  };
  const int foff = (lane & 15) * 64 + (((lane >> 4) ^ (((lane >> 3) & 1) << 1)) * 16);
  const int frow = wf * TF * 16;
  auto read_b = [&](const char *st, int pl, bf16x8 *b) {
#pragma unroll
    for (int j = 0; j < TF; ++j) b[j] = *reinterpret_cast<const bf16x8 *>(st + (pl * BF + frow + j * 16) * 64 + foff);
  };

  f32x4 acc[TW][TF];
#pragma unroll
  for (int i = 0; i < TW; ++i)
#pragma unroll
    for (int j = 0; j < TF; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  bf16x8 a0[2][TW], a1[TW], a2[TW], b0[TF], b1[TF], b2[TF];
  load_x(0, 0);
  load_w(0, 0, a0[0]);
  load_w(0, 1, a1);
  load_w(0, 2, a2);
  if constexpr (KS == 1) {
    put(smem, 0);
    load_x(1, 1);
  } else {
    load_x(1, 1);
    put(stage_of(0), 0);
    put(stage_of(1), 1);
    load_x(2, 0);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  auto body = [&](int kt, auto cc) {
    constexpr int c = decltype(cc)::value;
    const char *st = stage_of(kt);
    char *sn = stage_of(kt + KS);
    // Regions (sched_barrier): the compiler would otherwise sink every load
    // to its registers' last use and then wait on it at the next tile's
    // head.  The loads sit in regions of their own at the top of the
    // phase after their registers' last use; the split VALU of the next
    // activation tile shares the 48-MFMA region so it interleaves.
    // Activation registers alternate by tile parity: tile kt+1's chunk
    // (loaded one tile ago) is written while tile kt+2's is loaded.
    read_b(st, 0, b0);
    read_b(st, 1, b1);
    load_w(kt + 1, 0, a0[c ^ 1]);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr ((DIAG & 32) == 0) {
#pragma unroll
      for (int i = 0; i < TW; ++i)
#pragma unroll
        for (int j = 0; j < TF; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[c][i], b0[j], acc[i][j], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    // KS 1: load tile kt + 2 into rx[c], write tile kt + 1 from rx[c ^ 1];
    // KS 2: load tile kt + 3 into rx[c ^ 1], write tile kt + 2 from rx[c]
    load_x(kt + KS + 1, KS == 1 ? c : c ^ 1);
    __builtin_amdgcn_sched_barrier(0);
    put(sn, KS == 1 ? c ^ 1 : c);
    if constexpr ((DIAG & 32) == 0) {
#pragma unroll
      for (int i = 0; i < TW; ++i)
#pragma unroll
        for (int j = 0; j < TF; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[c][i], b1[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[i], b0[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[i], b1[j], acc[i][j], 0, 0, 0);
        }
    }
    read_b(st, 2, b2);
    __builtin_amdgcn_sched_barrier(0);
    load_w(kt + 1, 1, a1);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr ((DIAG & 32) == 0) {
#pragma unroll
      for (int i = 0; i < TW; ++i)
#pragma unroll
        for (int j = 0; j < TF; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[c][i], b2[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2[i], b0[j], acc[i][j], 0, 0, 0);
        }
    } else {
      // keep the fragment registers live
#pragma unroll
      for (int j = 0; j < TF; ++j) acc[0][j][0] += (float)b0[j][0] + (float)b1[j][0] + (float)b2[j][0] +
                                                   (float)a0[c][0][0] + (float)a1[0][0] + (float)a2[0][0];
    }
    __builtin_amdgcn_sched_barrier(0);
    load_w(kt + 1, 2, a2);
    if constexpr (KS == 1 || c == 1) {  // KS 2: once per stage (after its odd tile)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if constexpr ((DIAG & 16) == 0) __builtin_amdgcn_s_barrier();
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  int kt = 0;
  for (; kt + 1 < ktiles; kt += 2) {
    body(kt, std::integral_constant<int, 0>());
    body(kt + 1, std::integral_constant<int, 1>());
  }
  if (KS == 1 && kt < ktiles) body(kt, std::integral_constant<int, 0>());
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped tail prefetches
  x6_epilogue<TW, TF, OUT16>(p, acc, n0 + ww * TW * 16, f0 + frow, lane);
}

// One wave per SIMD (gemm_bf16x6w_kernel): 4 waves per block, each with up
// to 512 registers (the 256 accumulators of a 128 x 128 wave tile live in
// AGPRs), so every operand fragment feeds twice the products of the 8-wave
// kernel.  Block BW units x BF frames as WGW x WGF waves of TW x TF 16 x 16
// fragments.  At 512 x 128 (4 x 1 waves of 128 units x 128 frames), per
// output element and K-tile this halves the weight fragments loaded (each is
// loaded by exactly one wave), the activation fragments read from LDS (read
// by 4 waves for 128 frames x 512 units instead of 4 for 128 x 256) and the
// activation loads + split + LDS writes (one block covers 512 units) -- the
// bytes and VALU that cost clock at the chip's power cap (DESIGN.md §8 r5,
// r05z5 ablations).
// Per K-tile the wave runs its TW unit blocks in order; unit block i takes
// the TF frame blocks with the six products in gemm_bf16x6d_kernel's order
// per accumulator (a0b0, a0b1, a1b0, a1b1, a0b2, a2b0; K-tiles in order), so
// the results are bit-identical to it.
//   * weights: a ring of 4 unit-block buffers (3 planes each), each loaded
//     3 unit blocks (3 x 6 TF MFMAs) ahead of its use, straight from the
//     fragment image to registers, across K-tile boundaries;
//   * activations: the TF x 3 plane fragments of the K-tile stay in registers
//     for all TW unit blocks; in the last unit block each frame block's
//     fragments are replaced by the next K-tile's as soon as its six
//     products are issued;
//   * unit block 0: the next K-tile's activation rows (loaded one K-tile
//     ago) are split into the free LDS stage and the one after is loaded;
//     after unit block TW/2 - 1: lgkmcnt(0) and the block barrier (RAW for
//     the next K-tile's stage; WAR: a stage is rewritten one K-tile after
//     the barrier that follows its last reads).
template <int BW_, int BF_, int WGW_, int WGF_>
struct W6Cfg {
  static constexpr int BW = BW_, BF = BF_, WGW = WGW_, WGF = WGF_;
  static constexpr int NW = WGW * WGF, NT = 64 * NW;
  static constexpr int TW = BW / WGW / 16, TF = BF / WGF / 16;  // 16 x 16 fragments per wave
  static_assert(TW * WGW * 16 == BW && TF * WGF * 16 == BF, "bad one-wave-per-SIMD tile");
};

// SG: pin the interleave with sched_group_barrier -- the split + LDS writes of
// unit block 0 between its MFMAs (1 MFMA : 2 VALU), and in the last unit
// block each frame block's three fragment reads right after its six MFMAs
// (the compiler otherwise issues the split as one VALU block ahead of the
// MFMAs and sinks the reads to the end of the K-tile).
// RING: unit-block weight buffers in flight (RING - 1 unit blocks ahead).
// NW = 8 (two waves per SIMD, 256 registers each) is the same schedule with
// the accumulators of a 128 x 64 wave tile in AGPRs.
template <class C, bool SG = false, int RING = 4>
__global__ __launch_bounds__(C::NT, C::NW / 4) void gemm_bf16x6w_kernel(X6Args p) {
  constexpr int BF = C::BF, TW = C::TW, TF = C::TF, NT = C::NT;
  static_assert(C::NW == 4 || C::NW == 8, "one or two waves per SIMD");
  static_assert(TW % RING == 0, "a ring of unit-block weight buffers that divides the unit blocks");
  constexpr int RQ = BF / (NT / 4);  // activation rows per thread per K-tile
  static_assert(RQ >= 1 && RQ * (NT / 4) == BF, "whole activation rows per thread");
  constexpr int ASTAGE = 3 * BF * 64;
  __shared__ __attribute__((aligned(1024))) char smem[2 * ASTAGE];
  auto swz = [](int row) { return ((row >> 3) & 1) << 1; };
  typedef float f32x4v __attribute__((ext_vector_type(4)));
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef const __attribute__((address_space(1))) f32x4v gvec;
  typedef const __attribute__((address_space(1))) bf16x8 gfrag;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ww = wave / C::WGF, wf = wave % C::WGF;
  int tm, tn;
  tile_of(blockIdx.x, p.tiles_m, p.tiles_n, p.group, &tm, &tn);
  const int f0 = tm * BF, n0 = tn * C::BW;
  const int prow = tid >> 2, pch = tid & 3;
  const int ktiles = p.kpad / 32;

  // the wave's unit block i, K-tile kt, plane pl: fragment
  // ((ub0 + i) * wd_kt + kt) * 3 + pl of the image, lane's 16 bytes
  gfrag *wbase = (gfrag *)(p.wd + ((size_t)((n0 >> 4) + ww * TW) * p.wd_kt * 3 * 64 + lane) * 8);
  bf16x8 wa[RING][3];
  auto load_w = [&](int kt, int i, int buf) {
    kt = min(kt, ktiles - 1);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) wa[buf][pl] = wbase[((size_t)(i * p.wd_kt + kt) * 3 + pl) * 64];
  };
  f32x4v rx0[RQ], rx1[RQ];
  auto load_x = [&](int kt) {
    kt = min(kt, ktiles - 1);
    const int k0 = kt * 32;
    const int seg = k0 / p.din, col0 = k0 - seg * p.din;
    const int shift = (int)(signed char)(p.off_packed >> (8 * seg));
    gvec *xb = (gvec *)(p.xf + col0 + 8 * pch);
#pragma unroll
    for (int q = 0; q < RQ; ++q) {
      const int src = clampi(f0 + prow + q * (NT / 4) + shift, 0, p.m - 1);
      const uint32_t o = (uint32_t)(src * p.ldx) / 4;
      rx0[q] = xb[o];
      rx1[q] = xb[o + 1];
    }
  };
  auto put = [&](char *st) {
#pragma unroll
    for (int q = 0; q < RQ; ++q) {
      const Planes2 q0 = split3_pair(rx0[q].x, rx0[q].y), q1 = split3_pair(rx0[q].z, rx0[q].w);
      const Planes2 q2 = split3_pair(rx1[q].x, rx1[q].y), q3 = split3_pair(rx1[q].z, rx1[q].w);
      const int row = prow + q * (NT / 4);
      const int off = row * 64 + ((pch ^ swz(row)) * 16);
      *reinterpret_cast<u32x4 *>(st + off) = u32x4{q0.h, q1.h, q2.h, q3.h};
      *reinterpret_cast<u32x4 *>(st + BF * 64 + off) = u32x4{q0.m, q1.m, q2.m, q3.m};
      *reinterpret_cast<u32x4 *>(st + 2 * BF * 64 + off) = u32x4{q0.l, q1.l, q2.l, q3.l};
    }
  };
  const int foff = (lane & 15) * 64 + (((lane >> 4) ^ (((lane >> 3) & 1) << 1)) * 16);
  const int frow = wf * TF * 16;
  auto frag = [&](const char *st, int pl, int j) {
    return *reinterpret_cast<const bf16x8 *>(st + (pl * BF + frow + j * 16) * 64 + foff);
  };

  f32x4 acc[TW][TF];
#pragma unroll
  for (int i = 0; i < TW; ++i)
#pragma unroll
    for (int j = 0; j < TF; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  bf16x8 b0[TF], b1[TF], b2[TF];

  load_x(0);
#pragma unroll
  for (int i = 0; i < RING - 1; ++i) load_w(0, i, i);
  put(smem);
  load_x(1);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int j = 0; j < TF; ++j) {
    b0[j] = frag(smem, 0, j);
    b1[j] = frag(smem, 1, j);
    b2[j] = frag(smem, 2, j);
  }

  for (int kt = 0; kt < ktiles; ++kt) {
    char *sn = smem + ((kt + 1) & 1) * ASTAGE;
#pragma unroll
    for (int i = 0; i < TW; ++i) {
      // the weights three unit blocks ahead (the next K-tile's first ones
      // from unit block TW - 3 on)
      load_w(kt + (i + RING - 1) / TW, (i + RING - 1) % TW, (i + RING - 1) % RING);
      if (i == 0) {
        if constexpr (!SG) {
          put(sn);
          load_x(kt + 2);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (SG) {
        if (i == 0) {
          put(sn);
          load_x(kt + 2);
#pragma unroll
          for (int g = 0; g < 6 * TF; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);  // 2 VALU
            if (g % 4 == 3) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);  // an LDS write
          }
        }
      }
      constexpr int u = 0;  // (the ring slot is i % RING, a constant once unrolled)
#pragma unroll
      for (int j = 0; j < TF; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[i % RING][u], b0[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[i % RING][u], b1[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[i % RING][u + 1], b0[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[i % RING][u + 1], b1[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[i % RING][u], b2[j], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[i % RING][u + 2], b0[j], acc[i][j], 0, 0, 0);
        if (i == TW - 1) {  // frame block j is done for this K-tile: the next one's fragments
          b0[j] = frag(sn, 0, j);
          b1[j] = frag(sn, 1, j);
          b2[j] = frag(sn, 2, j);
        }
      }
      if constexpr (SG) {
        if (i == TW - 1) {
#pragma unroll
          for (int j = 0; j < TF; ++j) {
            __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);  // frame block j's six MFMAs
            __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);  // its next fragments
          }
        }
      }
      if (i == TW / 2 - 1) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // the clamped tail prefetches
  x6_epilogue<TW, TF, false>(p, acc, n0 + ww * TW * 16, f0 + frow, lane);
}

// ------------------------------------------------------------ host side --

// The tiles the product runs (kernels/gemm_bf16x6.hip).
using X6D128 = X6Cfg<128, 128, 2, 4, 2>;          // d: the gathered first layer, wide tiles
using X6D256 = X6Cfg<kX6DirUnits, 128, 4, 2, 2>;  // d: 8 waves of 64 units x 64 frames
using X6W512 = W6Cfg<512, 128, 4, 2>;             // w: 8 waves of 128 units x 64 frames
// 512 x 128 tiles only for layers of at least this many
constexpr int kX6WideMinTiles = 48;

// Column tiles per XCD tile group (tile_order.h) of the d and q kernels.  A
// hidden layer's 128 tiles (32 row x 4 unit) give each XCD 16: group 2 makes
// that 8 row x 2 unit tiles -- 9.5 MB of weight fragments + 12.5 MB of
// activations into its L2, against 18.9 + 6.3 MB for the whole-width group 8
// (C3 at the driver's step counts, alternating builds: 5.53-5.61 vs 5.45-5.52
// M frames/s).
#ifndef CATEARS_X6_GROUP
#define CATEARS_X6_GROUP 2
#endif

// The XCD tile groups of the 512-unit tiles (tile_order.h), by the layer's
// column tiles.  A 1024-unit layer (2 column tiles, 64 tiles): groups of 1
// put 8 row panels x 1 weight panel on each XCD (each row panel fetched into
// 2 XCDs' L2s, each weight panel into 4 -- the a . w = 8 minimum of DESIGN.md
// §8 r5): PMC 200 MB per hidden-layer launch against 223 MB with groups of 2
// (the whole width, a = 1, w = 8), C3 +1.1 % at the driver's flags
// (profiles/r06h_group_abc.txt).  The 3456-unit output layer (7 column
// tiles) keeps groups of 2: 214 MB against 243 MB.
inline int x6w_group(int tiles_n) { return tiles_n <= 2 ? 1 : 2; }

// Whether the w kernel on C's tiles can run the layer: the fragment image
// (units padded to a multiple of 256) covers the last unit tile, and the
// layer has at least min_tiles tiles.
template <class C>
bool x6w_fits(const X6Args &p, int min_tiles = 0) {
  const int tiles_n = (p.n + C::BW - 1) / C::BW, tiles_m = (p.m + C::BF - 1) / C::BF;
  return (p.n + 255) / 256 * 256 >= tiles_n * C::BW && tiles_n * tiles_m >= min_tiles;
}

// One launch: `kernel`, an instantiation on C's tiles, with one block of
// `threads` per tile.
template <class C>
int x6_launch(hipStream_t s, void (*kernel)(X6Args), X6Args p, int threads = C::NT) {
  p.tiles_n = (p.n + C::BW - 1) / C::BW;
  p.tiles_m = (p.m + C::BF - 1) / C::BF;
  hipLaunchKernelGGL(kernel, dim3(p.tiles_m * p.tiles_n), dim3(threads), 0, s, p);
  CE_HIP(hipGetLastError());
  return CE_GPU_OK;
}

// X6Gemm (checked by launch_gemm_bf16x6) as the kernel arguments; the tile
// counts are x6_launch's.
inline int x6_args(const X6Gemm &a, X6Args *out) {
  X6Args &p = *out;
  p.w = a.w;
  p.x = a.x;
  p.wf = a.wf;
  p.xf = a.xf;
  p.bias = a.bias;
  p.bn_scale = a.bn_scale;
  p.bn_offset = a.bn_offset;
  p.y32 = a.y32;
  p.y16 = a.y16;
  p.ldw = a.ldw;
  p.pw = a.pw;
  p.ldx = a.ldx;
  p.px = a.px;
  p.ldy = a.ldy;
  p.py = a.py;
  p.m = a.m;
  p.n = a.n;
  p.kpad = a.kpad;
  p.din = a.din;
  p.nseg = a.nseg;
  p.row_map = a.row_map;
  p.off_packed = 0;
  for (int i = 0; i < a.nseg; ++i) {
    if (a.off[i] < -128 || a.off[i] > 127) return fail(CE_GPU_ENOTSUP, "gemm_bf16x6: splice offset beyond +-127");
    p.off_packed |= (uint64_t)(uint8_t)(int8_t)a.off[i] << (8 * i);
  }
  for (int i = 0; i < 4; ++i) p.post[i] = a.post[i];
  p.npost = a.npost;
  p.post_mode = post_mode(a.post, a.npost);
  p.tiles_m = p.tiles_n = 0;
  p.group = CATEARS_X6_GROUP;
  p.wd = a.wd;
  p.wd_kt = a.wd_kt;
  return CE_GPU_OK;
}

}  // namespace
}  // namespace catears
