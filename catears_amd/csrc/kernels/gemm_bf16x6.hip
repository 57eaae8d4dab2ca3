// gemm_bf16x6.hip -- the TDNN layers' fp32 GEMM on the bf16 matrix cores.
//
// Same contraction as gemm_f32.hip (Splice + Narrow + LinearLayer + bias /
// ReLU / BatchNorm, src/nnet.cc:22-43,50-75,106-117,149-160,182-202;
// MatMat -> cblas_sgemm, src/matrix.cc:300-323), computed to fp32 accuracy
// with v_mfma_f32_16x16x32_bf16:
//
//   every fp32 operand x is stored as three bf16 planes x = x0 + x1 + x2
//   (x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1); each
//   subtraction is exact, and 3 x 8 significand bits plus the signs cover
//   fp32's 24, so the split is exact for every normal fp32 value), and
//
//   w . x = w0x0 + w0x1 + w1x0 + w1x1 + w0x2 + w2x0  (+ w1x2 + w2x1 + w2x2)
//
// The six kept products are exact in the MFMA (8 x 8 significand bits) and
// accumulate in fp32; the three dropped ones are below 2^-25 |w x| each,
// under the 2^-24 rounding of a single fp32 multiply.  So the result is an
// fp32 GEMM with a different (blocked) summation order -- the same status as
// the fp32-MFMA kernel -- at 6 bf16 MFMAs per fp32 MAC block: the bf16 rate
// is 16x the fp32 MFMA rate on gfx950, i.e. 2.7x the fp32 ceiling.
//
// Layout (HBM):
//   weights  n x ldw bf16, row j = [plane0 | plane1 | plane2], plane stride pw
//            (= kpad, zero padded), uploaded once (weight_images.cc bf16_plane_image)
//   acts     rows x ldx bf16, row r = [plane0 | plane1 | plane2], stride px;
//            written split by the previous layer's epilogue (or by
//            splice_pad_split for the first layer)
//   output   split bf16 (a hidden layer) or fp32 (the last layer, which
//            finalize reads)
//
// The MFMA's A operand is the weights (M = output units), B the activations
// (N = frames): the accumulator then holds four consecutive units of one
// frame per lane, so the epilogue reads bias/BN as float4 and stores 8 bytes
// per plane (16 for fp32) per lane.
//
// Tiling: BW units x BF frames per block, K-tile 32 (one MFMA k-step, 64 B
// per row per plane), 4 waves of (BW/2) x (BF/2).  Operands travel global ->
// LDS by LDS-DMA (global_load_lds_dwordx4: one wave instruction = 16 rows x
// 64 B of one plane), STAGES-deep ring, one barrier per K-tile, counted
// vmcnt (same protocol as gemm_f32_glds_kernel).  Bank spread: 16-B chunk c
// of tile row r is stored at chunk c ^ (2 * ((r >> 3) & 1)), applied on the
// source address; each of ds_read_b128's four 16-lane groups ({0-3,12-15,
// 20-27}, {4-11,16-19,28-31}, +32) then hits 16 distinct bank slots
// (MI355X_MICROARCH.md, LDS; the plain (r >> 2) & 3 swizzle is 2-way there).
//
// This file is what the product library runs: the argument checks, the plane
// kernel `q` (the tiling above), splice_pad_split, and the dispatch at the end
// over `q` and the fp32-activation kernels `d` and `w` of
// ../gemm_bf16x6_kernels.h.  Every other schedule -- measured, bit-identical
// alternatives and the ablations -- is in gemm_bf16x6_exp.hip, compiled into
// the experiments library only.
#include "../gemm_bf16x6_kernels.h"

namespace catears {
namespace {

// The plane kernel: a phased schedule with a branch-free loop body.  Three
// plane groups per K-tile on an LDS ring; every K-tile step runs the same
// straight-line code: the barrier, the DMA issue (clamped to the last tile:
// a dummy refetch into the free stage once the tail is reached) and the next
// tile's plane-0 fragment reads are unconditional, and the splice row
// offsets are recomputed per issue (no cached-segment branch).  One basic
// block per step lets the waitcnt pass count outstanding LDS reads exactly
// (lgkmcnt(N) instead of the lgkmcnt(0) a control-flow merge forces), so
// fragment reads of the next group stay in flight under this group's MFMAs.
// SCHED is 0 (the parameter stays in the kernel's name, which the tools spell).
template <class C, bool OUT16, int SCHED>
__global__ __launch_bounds__(C::NT, 1) void gemm_bf16x6q_kernel(X6Args p) {
  constexpr int BW = C::BW, BF = C::BF, TW = C::TW, TF = C::TF;
  constexpr int STAGE = C::STAGE, NQ = C::NQM, QW = C::QW;
  constexpr int S = C::STAGES;  // 2 or 3
  __shared__ __attribute__((aligned(1024))) char smem[S * STAGE];
  auto swz = [](int row) { return ((row >> 3) & 1) << 1; };

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ww = wave / C::WGF, wf = wave % C::WGF;
  int tm, tn;
  tile_of(blockIdx.x, p.tiles_m, p.tiles_n, p.group, &tm, &tn);
  const int f0 = tm * BF, n0 = tn * BW;

  // DMA pieces: the stage's QW weight pieces then QF activation pieces (one
  // piece = 16 rows x 64 B of one plane, stored at stage + 1 KB * piece).
  // Balanced when both kinds divide over the waves (each wave NQW weight +
  // NQF activation pieces: measured faster than giving some waves only one
  // kind); otherwise wave w issues pieces w NQ .. w NQ + NQ - 1 (wave-uniform
  // selects, no branch).
  constexpr bool BAL = C::QW % C::NW == 0 && C::QF % C::NW == 0;
  const int lrow = lane >> 2, lch = lane & 3;
  bool isw[NQ];
  int piece[NQ];
  uint32_t pconst[NQ];  // weight: byte offset at K-tile 0; activation: plane / chunk offset
  int xrow[NQ];         // activation tile row
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    int q;
    if constexpr (BAL) {
      isw[i] = i < C::NQW;
      q = isw[i] ? wave * C::NQW + i : QW + wave * C::NQF + (i - C::NQW);
    } else {
      q = wave * NQ + i;
      isw[i] = q < QW;
    }
    piece[i] = q;
    if (isw[i]) {
      const int plane = q / (BW / 16), row = (q % (BW / 16)) * 16 + lrow;
      pconst[i] = (uint32_t)((min(n0 + row, p.n - 1) * p.ldw + plane * p.pw + 8 * (lch ^ swz(row))) * 2);
      xrow[i] = 0;
    } else {
      const int q2 = q - QW, plane = q2 / (BF / 16), row = (q2 % (BF / 16)) * 16 + lrow;
      pconst[i] = (uint32_t)((plane * p.px + 8 * (lch ^ swz(row))) * 2);
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
    const char *wbase = reinterpret_cast<const char *>(p.w) + (size_t)k0 * 2;
    const char *xbase = reinterpret_cast<const char *>(p.x) + (size_t)col0 * 2;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const uint32_t xo = (uint32_t)(clampi(xrow[i] + shift, 0, p.m - 1) * p.ldx * 2) + pconst[i];
      const char *src = isw[i] ? wbase + pconst[i] : xbase + xo;
      glds16(src, st + piece[i] * 1024);
    }
  };
  const int foff = (lane & 15) * 64 + (((lane >> 4) ^ (((lane >> 3) & 1) << 1)) * 16);
  const int wrow = ww * TW * 16, frow = wf * TF * 16;
  auto rd = [&](const char *st, int pl, bf16x8 *a, bf16x8 *b) {
#pragma unroll
    for (int i = 0; i < TW; ++i) a[i] = *reinterpret_cast<const bf16x8 *>(st + (pl * BW + wrow + i * 16) * 64 + foff);
#pragma unroll
    for (int j = 0; j < TF; ++j)
      b[j] = *reinterpret_cast<const bf16x8 *>(st + 3 * BW * 64 + (pl * BF + frow + j * 16) * 64 + foff);
  };
  f32x4 acc[TW][TF];
#pragma unroll
  for (int i = 0; i < TW; ++i)
#pragma unroll
    for (int j = 0; j < TF; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  auto mm = [&](const bf16x8 *a, const bf16x8 *b) {
#pragma unroll
    for (int i = 0; i < TW; ++i)
#pragma unroll
      for (int j = 0; j < TF; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
  };

  bf16x8 a0[2][TW], b0[2][TF], a1[TW], b1[TF], a2[TW], b2[TF];
#pragma unroll
  for (int t = 0; t < S; ++t) issue(t);
  wait_vmcnt<(S - 1) * NQ>();
  __builtin_amdgcn_s_barrier();
  rd(smem, 0, a0[0], b0[0]);

  // Step kt reads stage kt % S: planes 1 and 2 before its barrier (plane 0
  // was read at the end of step kt-1), so once every wave has drained its
  // LDS reads (lgkmcnt(0)) and passed the barrier the stage is free and tile
  // kt+S is issued into it -- S-1 steps ahead of its first read.  RAW: tile
  // kt+1 is read (plane 0) right after the barrier; every wave's
  // vmcnt((S-2) NQ) before it retired all but the newest S-2 issues (tiles
  // kt+2 .. kt+S-1), i.e. tile kt+1.
  // In the last steps the issued tile is clamped to ktiles-1: a refetch of
  // the last tile into the stage it already occupies, writing the bytes it
  // holds, so any read of that stage sees the same values; it keeps one
  // issue per step, which the vmcnt count relies on.  The plane-0 read of
  // the nonexistent tile ktiles is never used.
  auto body = [&](int kt, auto cc) {
    constexpr int c = decltype(cc)::value;
    const char *st = smem + (kt % S) * STAGE;
    rd(st, 1, a1, b1);
    mm(a0[c], b0[c]);
    rd(st, 2, a2, b2);
    mm(a0[c], b1);
    mm(a1, b0[c]);
    mm(a1, b1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    wait_vmcnt<(S - 2) * NQ>();
    __builtin_amdgcn_s_barrier();
    issue(kt + S);
    rd(smem + ((kt + 1) % S) * STAGE, 0, a0[c ^ 1], b0[c ^ 1]);
    mm(a0[c], b2);
    mm(a2, b0[c]);
  };
  int kt = 0;
  for (; kt + 1 < ktiles; kt += 2) {
    body(kt, std::integral_constant<int, 0>());
    body(kt + 1, std::integral_constant<int, 1>());
  }
  if (kt < ktiles) body(kt, std::integral_constant<int, 0>());
  wait_vmcnt<0>();  // drain the tail refetches before the block ends

  x6_epilogue<TW, TF, OUT16>(p, acc, n0 + wrow, f0 + frow, lane);
}

// First layer: the spliced, zero-padded block (splice_pad_kernel's output)
// written directly as three bf16 planes.  out row r = [plane0 | plane1 |
// plane2], each `po` wide; columns nseg*din .. po-1 are zero.
__global__ __launch_bounds__(256) void splice_pad_split_kernel(const float *__restrict__ in, int ld_in, int rows,
                                                               int din, int nseg, SpliceIdx8 idx,
                                                               const int *__restrict__ row_map,
                                                               uint16_t *__restrict__ out, int po) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  uint16_t *o = out + (int64_t)r * 3 * po;
  for (int c = lane; c < po; c += 64) {
    const int s = c / din;
    float v = 0.0f;
    if (s < nseg) {
      int src = clampi(r + idx.v[s], 0, rows - 1);
      if (row_map) src = row_map[src];
      v = in[(int64_t)src * ld_in + (c - s * din)];
    }
    uint16_t h, m, l;
    split3(v, &h, &m, &l);
    o[c] = h;
    o[po + c] = m;
    o[2 * po + c] = l;
  }
}

}  // namespace

int launch_gemm_bf16x6(hipStream_t s, const X6Gemm &a) {
  if (a.m <= 0 || a.n <= 0) return CE_GPU_OK;
  // a first layer gathered in the loader (row_map, or segments that are not
  // whole K-tiles) needs the direct-weight kernel and din % 8 == 0
  const bool first = a.row_map != nullptr || a.din % 32 != 0;
  if (a.kpad % 32 != 0 || a.din % (first ? 8 : 32) != 0 || a.din <= 0 || a.nseg < 1 || a.nseg > 8 ||
      a.nseg * a.din > a.kpad)
    return fail(CE_GPU_EINVAL, "gemm_bf16x6: bad K geometry");
  if (first && (!a.xf || !a.wd))
    return fail(CE_GPU_EINVAL, "gemm_bf16x6: a gathered first layer needs fp32 input and the direct-weight kernel");
  if (a.n % 4 != 0 || a.ldy % 4 != 0 || (a.y16 && a.py % 4 != 0))
    return fail(CE_GPU_EINVAL, "gemm_bf16x6: output width must be a multiple of 4");
  const bool f32in = a.xf != nullptr;
  if (f32in) {
    if (!a.wf || !(a.y32 || a.y16) || a.ldw % 4 || a.ldx % 4 || (reinterpret_cast<uintptr_t>(a.wf) & 15) ||
        (reinterpret_cast<uintptr_t>(a.xf) & 15))
      return fail(CE_GPU_EINVAL, "gemm_bf16x6: fp32 operands must be 16-byte aligned, output fp32");
    // the kernel forms row * ld element offsets in 32 bits
    if ((int64_t)a.n * a.ldw >= ((int64_t)1 << 31) || (int64_t)a.m * a.ldx >= ((int64_t)1 << 31) ||
        (int64_t)a.m * a.ldy >= ((int64_t)1 << 31))
      return fail(CE_GPU_EINVAL, "gemm_bf16x6: operand beyond 2^31 elements");
  } else {
    if (a.ldw % 8 || a.pw % 8 || a.ldx % 8 || a.px % 8 || (reinterpret_cast<uintptr_t>(a.w) & 15) ||
        (reinterpret_cast<uintptr_t>(a.x) & 15))
      return fail(CE_GPU_EINVAL, "gemm_bf16x6: operands must be 16-byte aligned");
    if ((int64_t)a.n * a.ldw * 2 >= ((int64_t)1 << 32) || (int64_t)a.m * a.ldx * 2 >= ((int64_t)1 << 32))
      return fail(CE_GPU_EINVAL, "gemm_bf16x6: operand beyond 4 GiB");
  }
  if (a.npost > 4) return fail(CE_GPU_EINVAL, "gemm_bf16x6: too many post ops");
  X6Args p;
  CE_TRY(x6_args(a, &p));
#ifdef CATEARS_EXPERIMENTS
  // the experiments library: a CATEARS_X6_* switch off its default, or the
  // plane chain's operands (gemm_bf16x6_exp.hip)
  if (x6_exp_takes(a)) return launch_gemm_bf16x6_exp(s, a);
#endif
  // 1. plane operands (CE_GPU_GEMM_BF16X6_PLANES): the q kernel
  if (!f32in) {
    if (a.wd) return fail(CE_GPU_EINVAL, "gemm_bf16x6: plane input with the fragment image is the experiments library's");
    using Q = X6Cfg<128, 128, 4, 2, 3>;
    return x6_launch<Q>(s, a.y16 ? gemm_bf16x6q_kernel<Q, true, 0> : gemm_bf16x6q_kernel<Q, false, 0>, p);
  }
  // fp32 activations: the weights come from the fragment image
  if (!a.wd) return fail(CE_GPU_EINVAL, "gemm_bf16x6: fp32 input needs the weight fragment image");
  if (a.wd_kt * 32 < a.kpad || (reinterpret_cast<uintptr_t>(a.wd) & 15))
    return fail(CE_GPU_EINVAL, "gemm_bf16x6: weight fragment image does not cover K");
  if (a.y16) return fail(CE_GPU_EINVAL, "gemm_bf16x6: fp32 input with split output is the experiments library's");
  // 2. the gathered first layer (K of a few tiles: prologue and epilogue
  // bound) on 128 x 128 tiles -- twice the blocks; every layer so with
  // ce_gpu_ctx_set_wide_tiles (a batch scored while no other is in flight
  // then fills all CUs)
  if (first) return x6_launch<X6D128>(s, gemm_bf16x6d_kernel<X6D128, true>, p);
  if (a.wide) return x6_launch<X6D128>(s, gemm_bf16x6d_kernel<X6D128>, p);
  // 3. 512-unit tiles: each block splits and stages its activation rows once
  // for 512 units and each wave reads its B fragments once for 128 units --
  // half the activation path and LDS reads per product of 256 x 128
  //  -- when the layer has enough of them to spread over the
  // chip beside the other streams' batches (a 4096-row batch's hidden layer:
  // 64) and the fragment image (units padded to 256) covers the last tile
  if (x6w_fits<X6W512>(p, kX6WideMinTiles)) {
    p.group = x6w_group((p.n + X6W512::BW - 1) / X6W512::BW);
    return x6_launch<X6W512>(s, gemm_bf16x6w_kernel<X6W512, true, 4>, p);
  }
  // 4. otherwise (a 70-row streaming chunk: 2 tiles) 256 x 128 tiles
  return x6_launch<X6D256>(s, gemm_bf16x6d_kernel<X6D256>, p);
}

int launch_splice_pad_split(hipStream_t s, const float *in, int ld_in, int rows, int din, int nseg, const int *off,
                            const int *row_map, uint16_t *out, int po) {
  if (nseg < 1 || nseg > 8 || nseg * din > po) return fail(CE_GPU_EINVAL, "splice_pad_split: bad geometry");
  SpliceIdx8 idx = {};
  for (int i = 0; i < nseg; ++i) idx.v[i] = off[i];
  if (rows > 0)
    hipLaunchKernelGGL(splice_pad_split_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, in, ld_in, rows, din, nseg,
                       idx, row_map, out, po);
  CE_HIP(hipGetLastError());
  return CE_GPU_OK;
}

}  // namespace catears
