// plan_expand.hip -- the device side of ce_gpu_plan_assign (plans.cc): one
// launch turns an assignment's descriptor -- sample_off and frame_off
// (n_utt + 1 int64 each) and one PlanSeg per packed segment -- into the six
// tables of a ce_gpu_plan, word for word what ce_gpu_plan_create's host loops
// (capi.cc) build and upload for the same lengths:
//
//   sample_off, frame_off   copied;
//   block_utt[b]            the utterance of frame b * kFramesPerBlock: the
//                           first u with frame_off[u + 1] > b * fpb (the host's
//                           skip loop over zero-frame utterances), found by
//                           binary search; block_utt[0] = 0 for no block;
//   row_src / row_dst / row_edge   packed row r belongs to the last segment
//                           whose base is <= r (binary search over the
//                           ascending bases); with j = r - base it reads
//                           frame clamp(t - L + j, 0, T - 1) of its utterance,
//                           is output row frame_off[utt] + t + j - L when
//                           L <= j < L + n and -1 on a context row, and keeps
//                           row_edge_word(j, n + L + R - 1 - j).
//
// One thread per table index, integer arithmetic only, no LDS: the
// descriptor is O(n_utt + segments) words that every wave re-reads from L2.
// The tables are sized for the plan's capacity; the launch writes exactly the
// words the assignment uses and no launch of that assignment reads another.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../internal.h"

namespace catears {
namespace {

constexpr int kExpandThreads = 256;

// row_edge_word (internal.h, host) for the device: the rows to the segment's
// first and last row, each saturated at 0xffff.
__device__ __forceinline__ uint32_t edge_word(int64_t to_start, int64_t to_end) {
  const uint32_t dl = (uint32_t)(to_start < 0xffff ? to_start : 0xffff), dr = (uint32_t)(to_end < 0xffff ? to_end : 0xffff);
  return dl | (dr << 16);
}

__global__ __launch_bounds__(kExpandThreads) void plan_expand_kernel(
    const int64_t *__restrict__ sample_off, const int64_t *__restrict__ frame_off, const PlanSeg *__restrict__ segs,
    int n_utt, int n_seg, int fb_blocks, int fpb, int packed, int left, int right, int64_t *__restrict__ d_sample_off,
    int64_t *__restrict__ d_frame_off, int32_t *__restrict__ d_block_utt, int32_t *__restrict__ d_row_src,
    int32_t *__restrict__ d_row_dst, uint32_t *__restrict__ d_row_edge) {
  const int i = blockIdx.x * kExpandThreads + threadIdx.x;
  if (i <= n_utt) {
    d_sample_off[i] = sample_off[i];
    d_frame_off[i] = frame_off[i];
  }
  if (i < fb_blocks) {
    // first u in [0, n_utt) with frame_off[u + 1] > x; it exists because
    // x < frame_off[n_utt] for every block
    const int64_t x = (int64_t)i * fpb;
    int lo = 0, hi = n_utt - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (frame_off[mid + 1] > x)
        hi = mid;
      else
        lo = mid + 1;
    }
    d_block_utt[i] = lo;
  } else if (i == 0) {
    d_block_utt[0] = 0;
  }
  if (i < packed) {
    // last segment with base <= i (segs[0].base == 0)
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (segs[mid].base <= i)
        lo = mid;
      else
        hi = mid - 1;
    }
    const PlanSeg sg = segs[lo];
    const int64_t f0 = frame_off[sg.utt], T = frame_off[sg.utt + 1] - f0;
    const int64_t j = i - sg.base, seg_rows = (int64_t)sg.n + left + right;
    int64_t fr = (int64_t)sg.t - left + j;
    fr = fr < 0 ? 0 : (fr > T - 1 ? T - 1 : fr);
    d_row_src[i] = (int32_t)(f0 + fr);
    d_row_dst[i] = j >= left && j < left + sg.n ? (int32_t)(f0 + sg.t + j - left) : -1;
    d_row_edge[i] = edge_word(j, seg_rows - 1 - j);
  }
}

}  // namespace

int launch_plan_expand(hipStream_t s, const void *d_desc, int n_utt, int64_t n_seg, int64_t fb_blocks, int64_t packed,
                       int left, int right, int64_t *d_sample_off, int64_t *d_frame_off, int32_t *d_block_utt,
                       int32_t *d_row_src, int32_t *d_row_dst, uint32_t *d_row_edge) {
  if (!d_desc || !d_sample_off || !d_frame_off || !d_block_utt || n_utt < 0 || n_seg < 0 || fb_blocks < 0 ||
      packed < 0 || (packed > 0 && (n_seg == 0 || !d_row_src || !d_row_dst || !d_row_edge)))
    return fail(CE_GPU_EINVAL, "plan expand: bad argument");
  const int64_t items = std::max<int64_t>(std::max<int64_t>(n_utt + 1, fb_blocks), packed);
  if (items >= (int64_t)INT32_MAX - kExpandThreads || n_seg >= INT32_MAX)
    return fail(CE_GPU_EINVAL, "plan expand: too many rows");
  const char *d = static_cast<const char *>(d_desc);
  const int64_t *soff = reinterpret_cast<const int64_t *>(d);
  const int64_t *foff = soff + (n_utt + 1);
  const PlanSeg *segs = reinterpret_cast<const PlanSeg *>(d + plan_desc_seg_offset(n_utt));
  const int grid = (int)((items + kExpandThreads - 1) / kExpandThreads);
  hipLaunchKernelGGL(plan_expand_kernel, dim3(grid), dim3(kExpandThreads), 0, s, soff, foff, segs, n_utt, (int)n_seg,
                     (int)fb_blocks, fbank_frames_per_block(), (int)packed, left, right, d_sample_off, d_frame_off,
                     d_block_utt, d_row_src, d_row_dst, d_row_edge);
  CE_HIP(hipGetLastError());
  return CE_GPU_OK;
}

}  // namespace catears
