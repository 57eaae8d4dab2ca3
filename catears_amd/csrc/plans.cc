// plans.cc -- reusable batch plans: ce_gpu_plan_create_reusable reserves,
// once, every device table of a ce_gpu_plan for a capacity, and
// ce_gpu_plan_assign replaces the lengths with no allocation, release or
// synchronization.  The host keeps what its own launches need (sample_off,
// frame_off, the chunk list), writes a descriptor of O(n_utt + segments)
// words into the next of kPlanRing pinned buffers, and enqueues one
// asynchronous copy and one plan_expand_kernel launch
// (kernels/plan_expand.hip) that writes the tables -- the per-row maps never
// cross PCIe and no host loop runs over packed rows.  The copy and the
// launch go on the context's stream, so they run behind everything already
// enqueued with the previous lengths and ahead of everything enqueued later;
// the host waits only for a ring entry whose copy of kPlanRing assigns ago is
// still in flight (the rule of the sessions' descriptor ring, sessions.cc).
// The immutable ce_gpu_plan_create stays in capi.cc.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <new>
#include <vector>

#include "internal.h"
#include "model_io.h"

using namespace catears;

namespace {

// The most frames, segments and packed rows of any assignment of at most
// max_utts utterances and max_total_samples samples in all.
//
// Frames.  frames(n) = 0 for n < 400, else 1 + (n - 400) / 160, and
// frames(a) + frames(b) <= frames(a + b): a second utterance spends 400
// samples on its first frame where a longer first one would spend 160.  So
// F = frames(max_total_samples) bounds the total, reached by one utterance.
//
// Segments.  With room0 = max_rows - L - R, ce_gpu_plan_create's packing
// loop gives an utterance of T > 0 frames ceil(T / room0) segments: either
// the whole utterance fits the room left in the open chunk (one segment, and
// then T <= room0), or it starts in a fresh chunk and every segment but the
// last fills its chunk with room0 frames -- behind a full chunk the room is
// -(L + R), so the next segment always opens a chunk.  A sum of k ceilings
// is at most floor(sum of the arguments) + k, and at most
// k <= min(max_utts, F, max_total_samples / 400) utterances have a frame, so
//   segments <= F / room0 + k.
// Every chunk holds at least one segment, which bounds the chunk list too.
//
// Packed rows.  A segment of n frames packs n + L + R rows, so
//   packed <= F + segments * (L + R).
// All three bounds grow with F, hence the use of the largest F.
struct PlanBounds {
  int64_t frames = 0, segs = 0, packed = 0;
};

PlanBounds plan_bounds(int max_utts, int64_t max_total_samples, int max_rows, int left, int right, bool model) {
  PlanBounds b;
  b.frames = ce_gpu_fbank_num_frames(max_total_samples);
  if (!model) return b;
  const int64_t room0 = (int64_t)max_rows - left - right;
  const int64_t k = std::min<int64_t>(std::min<int64_t>(max_utts, b.frames), max_total_samples / kWinLen);
  b.segs = b.frames / room0 + k;
  b.packed = b.frames + b.segs * ((int64_t)left + right);
  return b;
}

}  // namespace

namespace catears {

void plan_release_ring(ce_gpu_plan *p) {
  if (!p->reusable) return;
  (void)hipSetDevice(p->device);
  for (ce_gpu_plan::RingEntry &re : p->ring) {
    if (re.copied) {
      // the copy out of the pinned buffer may still be queued
      if (re.in_use) (void)hipEventSynchronize(re.copied);
      (void)hipEventDestroy(re.copied);
      count_device_free();
    }
    if (re.host) {
      (void)hipHostFree(re.host);
      count_device_free();
    }
  }
  p->ring.clear();
}

}  // namespace catears

extern "C" {

int ce_gpu_plan_capacity(int max_utts, int64_t max_total_samples, int max_rows, int left, int right,
                         int64_t *max_frames, int64_t *max_segments, int64_t *max_packed_rows) {
  if (max_utts <= 0 || max_total_samples <= 0 || left < 0 || right < 0)
    return fail(CE_GPU_EINVAL, "plan_capacity: max_utts and max_total_samples must be positive");
  if (max_rows <= 0) max_rows = 4096;
  if (max_rows < left + right + 1) return fail(CE_GPU_EINVAL, "max_rows smaller than the nnet context");
  const PlanBounds b = plan_bounds(max_utts, max_total_samples, max_rows, left, right, true);
  if (max_frames) *max_frames = b.frames;
  if (max_segments) *max_segments = b.segs;
  if (max_packed_rows) *max_packed_rows = b.packed;
  return CE_GPU_OK;
}

int ce_gpu_plan_create_reusable(ce_gpu_ctx *ctx, const ce_gpu_model *model, int max_utts, int64_t max_total_samples,
                                int max_rows, ce_gpu_plan **out) {
  if (!out) return fail(CE_GPU_EINVAL, "out is NULL");
  *out = nullptr;
  if (!ctx) return fail(CE_GPU_EINVAL, "ctx is NULL");
  if (max_utts <= 0) return fail(CE_GPU_EINVAL, fmt("plan_create_reusable: max_utts %d is not positive", max_utts));
  if (max_total_samples <= 0)
    return fail(CE_GPU_EINVAL, fmt("plan_create_reusable: max_total_samples %lld is not positive",
                                   (long long)max_total_samples));
  if (max_rows <= 0) max_rows = 4096;
  const int L = model ? model->left : 0, R = model ? model->right : 0;
  if (model && max_rows < L + R + 1) return fail(CE_GPU_EINVAL, "max_rows smaller than the nnet context");
  const PlanBounds b = plan_bounds(max_utts, max_total_samples, max_rows, L, R, model != nullptr);
  // the kernels index frames and packed rows with 32 bits
  if (b.frames >= (int64_t)INT32_MAX / 2 || b.packed >= (int64_t)INT32_MAX / 2)
    return fail(CE_GPU_EINVAL, "plan_create_reusable: max_total_samples gives too many frames for one plan");
  CE_HIP(hipSetDevice(ctx->device));
  std::unique_ptr<ce_gpu_plan, int (*)(ce_gpu_plan *)> p(new (std::nothrow) ce_gpu_plan(), ce_gpu_plan_destroy);
  if (!p) return fail(CE_GPU_ENOMEM, "out of host memory");
  p->reusable = true;
  p->ctx = ctx;
  p->device = ctx->device;
  p->max_utts = max_utts;
  p->max_total_samples = max_total_samples;
  p->max_rows = max_rows;
  p->max_segs = b.segs;
  p->max_packed = b.packed;
  p->has_model = model != nullptr;
  p->left = L;
  p->right = R;
  // the empty assignment
  p->sample_off.reserve((size_t)max_utts + 1);
  p->frame_off.reserve((size_t)max_utts + 1);
  p->sample_off.assign(1, 0);
  p->frame_off.assign(1, 0);
  p->chunks.reserve((size_t)b.segs);
  p->next_chunks.reserve((size_t)b.segs);
  const int fpb = fbank_frames_per_block();
  const int64_t blocks = std::max<int64_t>((b.frames + fpb - 1) / fpb, 1);
  CE_TRY(p->d_sample_off.alloc(8 * ((size_t)max_utts + 1)));
  CE_TRY(p->d_frame_off.alloc(8 * ((size_t)max_utts + 1)));
  CE_TRY(p->d_block_utt.alloc(4 * (size_t)blocks));
  if (b.packed > 0) {
    CE_TRY(p->d_row_src.alloc(4 * (size_t)b.packed));
    CE_TRY(p->d_row_dst.alloc(4 * (size_t)b.packed));
    CE_TRY(p->d_row_edge.alloc(4 * (size_t)b.packed));
  }
  p->desc_bytes = plan_desc_bytes(max_utts, b.segs);
  CE_TRY(p->d_desc.alloc(p->desc_bytes));
  p->ring.resize(kPlanRing);
  for (ce_gpu_plan::RingEntry &re : p->ring) {
    CE_HIP(hipHostMalloc(&re.host, p->desc_bytes, hipHostMallocDefault));
    count_device_alloc();
    CE_HIP(hipEventCreateWithFlags(&re.copied, hipEventDisableTiming));
    count_device_alloc();
  }
  // the tables of the empty assignment (sample_off[0] = frame_off[0] =
  // block_utt[0] = 0), as ce_gpu_plan_create uploads them for n_utt = 0
  CE_TRY(ce_gpu_plan_assign(p.get(), nullptr, 0));
  *out = p.release();
  return CE_GPU_OK;
}

int ce_gpu_plan_assign(ce_gpu_plan *p, const int64_t *h_num_samples, int n_utt) {
  if (!p) return fail(CE_GPU_EINVAL, "plan is NULL");
  if (!p->reusable)
    return fail(CE_GPU_EINVAL, "plan_assign: the plan is immutable (ce_gpu_plan_create); use ce_gpu_plan_create_reusable");
  if (n_utt < 0 || (n_utt > 0 && !h_num_samples)) return fail(CE_GPU_EINVAL, "plan_assign: bad argument");
  if (n_utt > p->max_utts)
    return fail(CE_GPU_EINVAL, fmt("plan_assign: %d utterances, the plan's max_utts is %d", n_utt, p->max_utts));
  // 1. the checks, before anything of the plan changes
  int64_t total = 0;
  for (int u = 0; u < n_utt; ++u) {
    if (h_num_samples[u] < 0) return fail(CE_GPU_EINVAL, "plan_assign: negative sample count");
    // both terms are at most max_total_samples here: the sum cannot overflow
    if (h_num_samples[u] > p->max_total_samples || (total += h_num_samples[u]) > p->max_total_samples)
      return fail(CE_GPU_EINVAL, fmt("plan_assign: more than the plan's max_total_samples (%lld) samples",
                                     (long long)p->max_total_samples));
  }

  // 2. the descriptor image in the next pinned buffer
  CE_HIP(hipSetDevice(p->device));
  ce_gpu_plan::RingEntry &re = p->ring[p->ring_at];
  if (re.in_use && hipEventQuery(re.copied) != hipSuccess) CE_HIP(hipEventSynchronize(re.copied));
  (void)hipGetLastError();  // hipErrorNotReady from the query
  char *h = static_cast<char *>(re.host);
  int64_t *soff = reinterpret_cast<int64_t *>(h), *foff = soff + (n_utt + 1);
  PlanSeg *segs = reinterpret_cast<PlanSeg *>(h + plan_desc_seg_offset(n_utt));
  soff[0] = foff[0] = 0;
  for (int u = 0; u < n_utt; ++u) {
    soff[u + 1] = soff[u] + h_num_samples[u];
    foff[u + 1] = foff[u] + ce_gpu_fbank_num_frames(h_num_samples[u]);
  }
  const int64_t total_frames = foff[n_utt];
  const int fpb = fbank_frames_per_block();
  const int64_t blocks = (total_frames + fpb - 1) / fpb;
  // the segments and the chunk list by ce_gpu_plan_create's packing rule, one
  // step per segment.  The chunk list is built aside: the plan keeps its
  // previous assignment until this one is enqueued.
  int64_t n_seg = 0, packed = 0;
  int max_chunk_rows = 0;
  std::vector<ce_gpu_plan::Chunk> &chunks = p->next_chunks;
  chunks.clear();
  if (p->has_model) {
    const int L = p->left, R = p->right;
    ce_gpu_plan::Chunk cur;
    auto close = [&]() {
      if (cur.rows > 0) {
        max_chunk_rows = std::max(max_chunk_rows, cur.rows);
        chunks.push_back(cur);
      }
      cur = ce_gpu_plan::Chunk();
      cur.map_base = packed;
    };
    for (int u = 0; u < n_utt; ++u) {
      const int64_t T = foff[u + 1] - foff[u];
      int64_t t = 0;
      while (t < T) {
        int64_t room = p->max_rows - cur.rows - L - R;
        if (room < T - t && cur.rows > 0) {  // start the utterance in a fresh chunk
          close();
          room = p->max_rows - L - R;
        }
        const int64_t n = std::min(T - t, room);
        // plan_bounds rules this out; the tables and the descriptor end here
        if (n_seg >= p->max_segs || packed + n + L + R > p->max_packed)
          return fail(CE_GPU_EINVAL, "plan_assign: internal: capacity bound exceeded");
        PlanSeg &sg = segs[n_seg++];
        sg.utt = u;
        sg.t = (int32_t)t;
        sg.n = (int32_t)n;
        sg.base = (int32_t)packed;
        packed += n + L + R;
        cur.rows += (int)(n + L + R);
        t += n;
      }
    }
    close();
  }

  // 3. one copy, one launch
  hipStream_t st = p->ctx->stream;
  CE_HIP(hipMemcpyAsync(p->d_desc.ptr, h, plan_desc_bytes(n_utt, n_seg), hipMemcpyHostToDevice, st));
  CE_HIP(hipEventRecord(re.copied, st));
  re.in_use = true;
  p->ring_at = (p->ring_at + 1) % kPlanRing;
  CE_TRY(launch_plan_expand(st, p->d_desc.ptr, n_utt, n_seg, blocks, packed, p->left, p->right,
                            p->d_sample_off.as<int64_t>(), p->d_frame_off.as<int64_t>(), p->d_block_utt.as<int32_t>(),
                            p->d_row_src.as<int32_t>(), p->d_row_dst.as<int32_t>(), p->d_row_edge.as<uint32_t>()));

  // 4. the host's side of the assignment
  p->n_utt = n_utt;
  p->sample_off.assign(soff, soff + n_utt + 1);
  p->frame_off.assign(foff, foff + n_utt + 1);
  p->total_samples = soff[n_utt];
  p->total_frames = total_frames;
  p->fbank_blocks = (int)blocks;
  p->chunks.swap(chunks);
  p->max_chunk_rows = max_chunk_rows;
  p->packed = packed;
  return CE_GPU_OK;
}

int ce_gpu_debug_plan_tables(const ce_gpu_plan *p, int which, void *h_out, int64_t capacity_bytes, int64_t *bytes) {
  if (!p || !bytes) return fail(CE_GPU_EINVAL, "debug_plan_tables: NULL argument");
  const int64_t packed = p->reusable ? p->packed : (int64_t)(p->d_row_src.bytes / 4);
  const void *src = nullptr;
  int64_t n = 0;
  switch (which) {
    case 0: src = p->d_sample_off.ptr, n = 8 * ((int64_t)p->n_utt + 1); break;
    case 1: src = p->d_frame_off.ptr, n = 8 * ((int64_t)p->n_utt + 1); break;
    case 2: src = p->d_block_utt.ptr, n = 4 * std::max<int64_t>(p->fbank_blocks, 1); break;
    case 3: src = p->d_row_src.ptr, n = 4 * packed; break;
    case 4: src = p->d_row_dst.ptr, n = 4 * packed; break;
    case 5: src = p->d_row_edge.ptr, n = 4 * packed; break;
    default: return fail(CE_GPU_EINVAL, "debug_plan_tables: tables are numbered 0 .. 5");
  }
  *bytes = n;
  if (n == 0 || !h_out) return CE_GPU_OK;  // h_out == NULL asks for the length alone
  if (capacity_bytes < n)
    return fail(CE_GPU_EINVAL, fmt("debug_plan_tables: capacity %lld < %lld bytes", (long long)capacity_bytes, (long long)n));
  CE_HIP(hipSetDevice(p->device));
  if (p->ctx) CE_HIP(hipStreamSynchronize(p->ctx->stream));
  CE_HIP(hipMemcpy(h_out, src, (size_t)n, hipMemcpyDeviceToHost));
  return CE_GPU_OK;
}

}  // extern "C"
