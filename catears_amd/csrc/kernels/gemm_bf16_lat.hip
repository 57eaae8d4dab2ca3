// gemm_bf16_lat.hip -- latency mode of the plain bf16 GEMM (CE_GPU_GEMM_BF16
// on a context with ce_gpu_ctx_set_latency, up to kB16LatMaxRows rows).
//
// The same contraction as gemm_bf16_kernel (kernels/gemm_bf16.hip, where the
// mode is defined), to the bit: one v_mfma_f32_16x16x32_bf16 per (16-unit
// block, 16-frame fragment, K-tile), the K-tiles in ascending order into one
// fp32 accumulator, then gemm_bf16_kernels.h's b16_epilogue.  No split-K: what
// differs is only who computes an output and how its operands reach the MFMA.
//
// gemm_bf16_kernel on 32 x 32 tiles walks a 3072-wide layer as 96 K-tiles
// behind one barrier each; with 70 rows that is 96 blocks of two waves, bound
// by the latency of a K-tile's trip through the LDS ring.  Here a wave owns
// 16 units x 16 TF frames, so a 70-row block of a 1024-wide layer is 64 x 5
// waves (TF = 1), and it needs neither LDS nor a barrier, because both
// operands already lie in memory as the MFMA wants them:
//   weights  fragment (u, t) is the contiguous 1 KB at ((u wd_kt + t) 3) 1024
//            bytes of the fragment image (plane 0), lane l's 16 bytes at 16 l
//   acts     lane l's 16 bytes of row clamp(f0 + 16 j + (l & 15) + shift(seg),
//            0, m - 1) at column col0 + 8 (l >> 4) of the row-major bf16 block
// Each is one 16-byte global load per lane into a register ring of D K-tiles:
// the wave keeps D tiles of loads in flight, consumes the oldest and refills
// its slot.  The ring's slots are named at compile time (the batch of D steps
// is unrolled), and the compiler counts vmcnt per slot.
//
// Every load address is in range by construction:
//   weights  u < round_up(n, kX6DirUnits) / 16: the image's units are zero
//            padded to kX6DirUnits = 256 and a wave without a unit below n
//            returns before it loads (with several waves per block, NW
//            divides 16); t is clamped to ktiles - 1
//            (the loader's cursor stops on the last tile), ktiles <= wd_kt
//   acts     the row is clamped to [0, m - 1]; col0 + 8 (l >> 4) + 8 <= din <=
//            ldx since col0 <= din - 32 (din % 32 == 0, cursor as above)
// Loads past the last K-tile refetch the last one (as gemm_bf16_kernel's tail
// refetch does) and are never fed to an MFMA.
//
// No plain store before the epilogue, no atomics, no communication between
// blocks, no LDS-DMA (see gemm_bf16.hip on mixing it with register loads).
//
// The shape -- TF, the ring depth D, the waves per block NW and which waves
// share a block -- was chosen by measurement: launch_gemm_bf16_lat below.
#include <hip/hip_runtime.h>

#include <atomic>

#include "../gemm_bf16_kernels.h"
#include "../internal.h"
#include "../lds_dma.h"

namespace catears {
namespace {

using dma::clampi;

// SHAREW: the NW waves of a block take neighbouring frame groups of one unit
// block (they share the weight cache lines) instead of neighbouring unit
// blocks of one frame group (they share the activations')
template <int TF_, int D_, int NW_, bool SHAREW_ = false>
struct L16Cfg {
  static constexpr int TF = TF_, D = D_, NW = NW_;
  static constexpr bool SHAREW = SHAREW_;
  static_assert(TF >= 1 && D >= 2 && NW >= 1 && (SHAREW || 16 % NW == 0), "bad bf16 latency shape");
  static_assert((1 + TF) * 4 * D + 4 * TF <= 400, "the ring must stay in registers");
};

template <class C, bool OUT16>
__global__ __launch_bounds__(64 * C::NW) void gemm_bf16_lat_kernel(B16Args p) {
  constexpr int TF = C::TF, D = C::D;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // unit groups fastest: the blocks that read one weight fragment (one per
  // frame group) are tiles_n apart
  const int ug = blockIdx.x % p.tiles_n, fg = blockIdx.x / p.tiles_n;
  const int u = C::SHAREW ? ug : ug * C::NW + wave;
  const int f0 = (C::SHAREW ? fg * C::NW + wave : fg) * 16 * TF;
  if (u * 16 >= p.n || f0 >= p.m) return;  // a whole wave of padding (no barrier in this kernel)
  const int ktiles = p.kpad / 32;
  const char *wl = reinterpret_cast<const char *>(p.wd) + (size_t)u * p.wd_kt * 3072 + lane * 16;
  const char *xl = reinterpret_cast<const char *>(p.x) + 16 * (lane >> 4);
  int frow[TF];
#pragma unroll
  for (int j = 0; j < TF; ++j) frow[j] = f0 + 16 * j + (lane & 15);

  // the loader's cursor: K-tile lt lies in segment lseg at column lcol; it
  // stops on the last tile
  int lt = 0, lseg = 0, lcol = 0;
  auto load = [&](bf16x8 &a, bf16x8(&b)[TF]) {
    a = *reinterpret_cast<const bf16x8 *>(wl + (size_t)lt * 3072);
    const int shift = (int)(signed char)(p.off_packed >> (8 * lseg));
#pragma unroll
    for (int j = 0; j < TF; ++j)
      b[j] = *reinterpret_cast<const bf16x8 *>(xl + (size_t)(clampi(frow[j] + shift, 0, p.m - 1) * p.ldx + lcol) * 2);
    if (lt + 1 < ktiles) {
      ++lt;
      lcol += 32;
      if (lcol == p.din) lcol = 0, ++lseg;
    }
  };

  f32x4 acc[1][TF];
#pragma unroll
  for (int j = 0; j < TF; ++j) acc[0][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  bf16x8 a[D], b[D][TF];
#pragma unroll
  for (int d = 0; d < D; ++d) load(a[d], b[d]);
  int t = 0;
  for (; t + D <= ktiles; t += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
#pragma unroll
      for (int j = 0; j < TF; ++j) acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[d], b[d][j], acc[0][j], 0, 0, 0);
      load(a[d], b[d]);
    }
  }
  // the last ktiles - t < D tiles sit in slots 0 ..; the slots behind them
  // hold refetches of the last tile and are not used
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (t + d < ktiles) {
#pragma unroll
      for (int j = 0; j < TF; ++j) acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[d], b[d][j], acc[0][j], 0, 0, 0);
    }
  }
  b16_epilogue<1, TF, OUT16>(p, acc, u * 16, f0, lane);
}

std::atomic<int64_t> g_launches{0};

template <class C>
int launch_l16(hipStream_t s, B16Args p, bool out16) {
  const int nwn = C::SHAREW ? 1 : C::NW, nwm = C::SHAREW ? C::NW : 1;
  p.tiles_n = ((p.n + 15) / 16 + nwn - 1) / nwn;
  p.tiles_m = (p.m + 16 * C::TF * nwm - 1) / (16 * C::TF * nwm);
  dim3 grid(p.tiles_m * p.tiles_n), block(64 * C::NW);
  if (out16)
    hipLaunchKernelGGL((gemm_bf16_lat_kernel<C, true>), grid, block, 0, s, p);
  else
    hipLaunchKernelGGL((gemm_bf16_lat_kernel<C, false>), grid, block, 0, s, p);
  CE_HIP(hipGetLastError());
  g_launches.fetch_add(1, std::memory_order_relaxed);
  return CE_GPU_OK;
}

}  // namespace

int b16_lat_max_rows() {
  static const int v = CE_KNOB("CATEARS_B16_LAT_MAXROWS", kB16LatMaxRows);
  return v;
}

int64_t b16_lat_launch_count() { return g_launches.load(std::memory_order_relaxed); }

// The shape: TF = 1, D = 12, one wave per block.  TDNN-S, 70 rows, p50 per
// ce_gpu_nnet_propagate call and per hidden 3072 -> 1024 layer, one run of
// the experiments library per shape (gemm_bf16_kernel in the same runs:
// 114.5 us, 22.4 us per hidden layer):
//   TF  D  NW  block's waves share        call us   hidden layer us
//    1 12   1  --                           71.0       13.3   (adopted)
//    1 16   1  --                           73.2       13.3
//    1 24   1  --                           77.5       13.6
//    1 32   1  --                           84.2       14.1
//    2 16   1  --                           83.6       15.4
//    1 16   2  activations                  74.0       13.3
//    1 16   2  weights                      73.3       13.4
//    1 16   4  activations                 104.5       19.6
//    1 16   4  weights                     102.3       19.7
//    1 16   5  weights                     113.1       22.0
//    1 24   4  activations                 110.2       20.8
//    1  8   4  activations                 131.3       25.9
//    2  8   2  activations                 133.8       26.6
//    2 16   4  activations                 162.5       31.7
//    5  8   4  activations                 289.7       57.7
// The fewer waves share a CU the better, whatever they share: 320 one-wave
// blocks reach every CU, and a deeper ring than 12 K-tiles buys nothing (the
// hidden layer stays at 13.3 us from D = 12 to 24) while its registers cost
// the 1080-wave output layer its second wave per SIMD (10.7 us at D = 12,
// 12.3 at 16, 14.8 at 24).
int launch_gemm_bf16_lat(hipStream_t s, const X6Gemm &a) {
  if (a.m <= 0 || a.n <= 0) return CE_GPU_OK;
  B16Args p;
  CE_TRY(b16_fill_args(a, &p));
  const bool out16 = a.y16 != nullptr;
#ifdef CATEARS_EXPERIMENTS
  // CATEARS_B16_LAT_SHAPE: the other shapes of the measurement (the same bits)
  static const int shape = CE_KNOB("CATEARS_B16_LAT_SHAPE", 11);
  switch (shape) {
    case 1: return launch_l16<L16Cfg<1, 8, 4>>(s, p, out16);
    case 2: return launch_l16<L16Cfg<2, 16, 4>>(s, p, out16);
    case 3: return launch_l16<L16Cfg<1, 16, 1>>(s, p, out16);
    case 4: return launch_l16<L16Cfg<5, 8, 4>>(s, p, out16);
    case 5: return launch_l16<L16Cfg<1, 24, 4>>(s, p, out16);
    case 6: return launch_l16<L16Cfg<2, 8, 2>>(s, p, out16);
    case 7: return launch_l16<L16Cfg<1, 16, 2>>(s, p, out16);
    case 8: return launch_l16<L16Cfg<1, 32, 1>>(s, p, out16);
    case 9: return launch_l16<L16Cfg<1, 16, 5, true>>(s, p, out16);
    case 10: return launch_l16<L16Cfg<1, 16, 2, true>>(s, p, out16);
    case 0: return launch_l16<L16Cfg<1, 16, 4>>(s, p, out16);
    case 12: return launch_l16<L16Cfg<1, 24, 1>>(s, p, out16);
    case 13: return launch_l16<L16Cfg<2, 16, 1>>(s, p, out16);
    case 14: return launch_l16<L16Cfg<1, 16, 4, true>>(s, p, out16);
    default: break;
  }
#endif
  return launch_l16<L16Cfg<1, 12, 1>>(s, p, out16);
}

}  // namespace catears
