// sessions.cc -- ce_gpu_sessions: n_slots live audio streams whose state (the
// unconsumed sample tail, the CMVN carry and window, the nnet's left context)
// stays in HBM between pushes.  One push advances any subset of the slots:
//
//   stage (new samples behind each tail) -> fbank (the whole-utterance
//   kernel, reading the staging regions as its utterances) -> carry (the
//   remainder to the front) -> cmvn_resume (into the slots' rings) -> the
//   nnet over packed rows gathered from the rings -> finalize into d_loglik.
//
// The host keeps every count (samples, frames, rows emitted per slot) by its
// own arithmetic and never reads device state back.  What the kernels need
// per push -- the push list, the fbank descriptor, the row maps -- is written
// into one of kRing pinned buffers and copied with one hipMemcpyAsync; the
// host waits for a ring entry only if its copy of kRing pushes ago is still
// in flight.  Nothing is allocated, freed or synchronized on the way.
//
// An incremental set (CE_GPU_SESSIONS_INCREMENTAL) packs fewer rows.  With
// every Linear's splice offsets re-based to off[s] - max(off) the nnet is a
// chain of causal layers over the padded frame sequence (L copies of frame 0,
// the frames, R copies of the last one at EOS): position p gives the output
// row of time p - L - R.  A slot keeps, per Linear, the last c rows of that
// layer's input (c = the span of its offsets), so a push that feeds it k
// positions packs a block of H lead rows (H = the largest c) and k new rows
// instead of k + L + R; session_ctx_exchange_kernel moves the cached rows in
// and out per chunk and layer (score_packed_rows with an IncrChunk).
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

constexpr int kRing = 8;          // pinned descriptor buffers
constexpr int kMaxRows = 4096;    // packed rows per nnet chunk (ce_gpu_plan_create's default)
constexpr int kWindow = 600;      // PK_ONLINECMVN_WINDOW: frames the raw ring keeps behind a push

size_t align16(size_t n) { return (n + 15) / 16 * 16; }

struct Slot {
  int64_t samples = 0;  // since the last reset
  int64_t frames = 0;   // ce_gpu_fbank_num_frames(samples): computed so far
  int64_t rows = 0;     // log-likelihood rows emitted so far
  bool eos = false;
};

struct RingEntry {
  void *host = nullptr;
  hipEvent_t copied = nullptr;
  bool in_use = false;
};

struct Chunk {
  int rows = 0;
  int64_t map_base = 0;
  int blk_base = 0, n_blocks = 0;  // incremental: its blocks in the push's block list
};

// The padded frames (positions) a slot has fed the nnet: nothing before its
// first frame, then the L copies of frame 0 with it, the R copies of the last
// frame with the EOS.
int64_t positions(const Slot &s, int L, int R) { return s.frames == 0 ? 0 : L + s.frames + (s.eos ? R : 0); }

}  // namespace

struct ce_gpu_sessions {
  ce_gpu_ctx *ctx = nullptr;
  const ce_gpu_model *m = nullptr;
  const float *gstats = nullptr;
  bool static_int8 = false;    // the model's form at create
  int gemm = 0;                // ... its GEMM mode (checked by an incremental set only)
  bool incremental = false;    // CE_GPU_SESSIONS_INCREMENTAL
  int H = 0;                   // incremental: lead rows per block
  int64_t max_blocks = 0;      // incremental: most blocks of one push
  std::vector<IncrLayer> layers;  // incremental: one per Linear
  DevBuf cache, cache_sums;       // ... their rows and row sums, all slots
  int64_t n_pushes = 0, n_packed = 0, n_chunks = 0;  // ce_gpu_sessions_stats
  int n_slots = 0, max_chunk = 0, L = 0, R = 0;
  int max_frames = 0;          // most frames one push of one slot can complete
  int raw_cap = 0, norm_cap = 0;
  int64_t stride = 0;          // floats per staging region
  int64_t max_packed = 0;      // most packed rows (map entries) of one push
  std::vector<Slot> slots;
  std::vector<int64_t> seen;   // push stamp per slot (distinctness)
  int64_t stamp = 0;
  std::vector<Slot> next;      // the pushed slots' states after the push
  std::vector<Chunk> chunks;
  DevBuf stage, raw, norm, carry, tmp, desc;
  size_t desc_bytes = 0;
  RingEntry ring[kRing];
  int ring_at = 0;
};

namespace {

template <typename Sample>
int push_t(ce_gpu_sessions *s, int n, const int32_t *h_slot, const int32_t *h_num_samples, const int32_t *h_flags,
           const Sample *d_pcm, float *d_loglik, int64_t capacity_rows, int32_t *h_rows_out) {
  if (!s || n < 0 || (n > 0 && (!h_slot || !h_num_samples || !h_rows_out)))
    return fail(CE_GPU_EINVAL, "sessions_push: bad argument");
  if (n == 0) return CE_GPU_OK;
  if (n > s->n_slots) return fail(CE_GPU_EINVAL, "sessions_push: more pushes than slots");
  const ce_gpu_model *m = s->m;
  if (m->int8 && !m->int8_static)
    return fail(CE_GPU_ENOTSUP, "sessions_push: the model was quantized (int8 rows depend on the batch)");
  // the workspaces were sized for the form the model had at sessions_create
  if (m->int8_static != s->static_int8)
    return fail(CE_GPU_EINVAL, "sessions_push: the model was quantized after sessions_create");
  // an incremental set's caches hold rows in the representation of that form
  if (s->incremental && !m->int8_static && m->gemm != s->gemm)
    return fail(CE_GPU_EINVAL, "sessions_push: the model's GEMM mode changed after sessions_create_ex");
  const int L = s->L, R = s->R;

  // 1. every count of the push, by arithmetic alone
  ++s->stamp;
  int64_t total_samples = 0, total_frames = 0, total_rows = 0;
  int max_new = 0;
  for (int i = 0; i < n; ++i) {
    const int k = h_slot[i], ns = h_num_samples[i];
    if (k < 0 || k >= s->n_slots) return fail(CE_GPU_EINVAL, fmt("sessions_push: no slot %d", k));
    if (s->seen[k] == s->stamp) return fail(CE_GPU_EINVAL, fmt("sessions_push: slot %d pushed twice", k));
    s->seen[k] = s->stamp;
    if (ns < 0 || ns > s->max_chunk)
      return fail(CE_GPU_EINVAL, fmt("sessions_push: %d samples for slot %d (max_chunk_samples %d)", ns, k, s->max_chunk));
    const Slot &cur = s->slots[k];
    if (cur.eos) return fail(CE_GPU_EINVAL, fmt("sessions_push: slot %d ended its utterance; reset it first", k));
    Slot nx = cur;
    nx.samples += ns;
    nx.frames = ce_gpu_fbank_num_frames(nx.samples);
    nx.eos = h_flags && (h_flags[i] & CE_GPU_SESSION_EOS);
    nx.rows = nx.eos ? nx.frames : std::max<int64_t>(0, nx.frames - R);
    if (nx.frames >= INT32_MAX - 2 * kMaxRows) return fail(CE_GPU_EINVAL, "sessions_push: utterance too long");
    s->next[i] = nx;
    h_rows_out[i] = (int32_t)(nx.rows - cur.rows);
    total_samples += ns;
    total_frames += nx.frames - cur.frames;
    total_rows += nx.rows - cur.rows;
    max_new = std::max(max_new, ns);
  }
  if (total_rows > capacity_rows)
    return fail(CE_GPU_EINVAL, fmt("sessions_push: %lld rows, capacity %lld", (long long)total_rows,
                                   (long long)capacity_rows));
  if ((total_samples > 0 && !d_pcm) || (total_rows > 0 && !d_loglik))
    return fail(CE_GPU_EINVAL, "sessions_push: NULL device buffer");

  // 2. the descriptor image in the next pinned buffer
  ce_gpu_ctx *ctx = s->ctx;
  RingEntry &re = s->ring[s->ring_at];
  if (re.in_use && hipEventQuery(re.copied) != hipSuccess) CE_HIP(hipEventSynchronize(re.copied));
  (void)hipGetLastError();  // hipErrorNotReady from the query
  char *h = static_cast<char *>(re.host);
  const int fpb = fbank_frames_per_block();
  const int64_t fb_blocks = (total_frames + fpb - 1) / fpb;
  const size_t o_push = 0;
  const size_t o_soff = align16(o_push + sizeof(SessionPush) * n);
  const size_t o_foff = align16(o_soff + 8 * (size_t)(n + 1));
  const size_t o_butt = align16(o_foff + 8 * (size_t)(n + 1));
  const size_t o_maps = align16(o_butt + 4 * (size_t)std::max<int64_t>(fb_blocks, 1));
  SessionPush *push = reinterpret_cast<SessionPush *>(h + o_push);
  int64_t *soff = reinterpret_cast<int64_t *>(h + o_soff), *foff = reinterpret_cast<int64_t *>(h + o_foff);
  int32_t *butt = reinterpret_cast<int32_t *>(h + o_butt);
  {
    int64_t pcm_at = 0;
    foff[0] = 0;
    for (int i = 0; i < n; ++i) {
      const Slot &cur = s->slots[h_slot[i]], &nx = s->next[i];
      SessionPush &p = push[i];
      p.pcm_off = pcm_at;
      p.slot = h_slot[i];
      p.tail = (int32_t)(cur.samples - kShift * cur.frames);
      p.n_new = h_num_samples[i];
      p.frames = (int32_t)(nx.frames - cur.frames);
      p.t0 = (int32_t)cur.frames;
      p.tmp_row = (int32_t)foff[i];
      soff[i] = (int64_t)h_slot[i] * s->stride;
      foff[i + 1] = foff[i] + p.frames;
      pcm_at += p.n_new;
    }
    soff[n] = 0;
    int u = 0;
    for (int64_t b = 0; b < fb_blocks; ++b) {
      while (foff[u + 1] <= b * fpb) ++u;
      butt[b] = u;
    }
  }
  // the row maps: each slot's new rows with their L + R context rows, packed
  // into chunks by ce_gpu_plan_create's rule (a block that does not fit the
  // chunk's remaining room starts a fresh chunk; a block larger than a chunk
  // is split into segments overlapping by L + R)
  int32_t *src = reinterpret_cast<int32_t *>(h + o_maps);
  int64_t packed = 0, n_blocks = 0;
  s->chunks.clear();
  const int H = s->H;
  // incremental: every block of the push in order -- f(push i, starts a new
  // chunk, first row in its chunk, first position, positions).  A block that
  // does not fit the chunk's remaining room starts a new chunk; one larger
  // than a chunk is cut into blocks that each fill their chunk, so a chunk
  // never holds two blocks of one slot (the second's lead rows come from the
  // cache the first one leaves, and chunks run in stream order).
  auto each_block = [&](auto &&f) {
    int cur_rows = 0;
    for (int i = 0; i < n; ++i) {
      int64_t p = positions(s->slots[h_slot[i]], L, R);
      const int64_t p1 = positions(s->next[i], L, R);
      while (p < p1) {
        int64_t room = kMaxRows - cur_rows - H;
        const bool fresh_chunk = room < p1 - p && cur_rows > 0;
        if (fresh_chunk) {
          cur_rows = 0;
          room = kMaxRows - H;
        }
        const int64_t k = std::min(p1 - p, room);
        f(i, fresh_chunk, cur_rows, p, k);
        cur_rows += (int)(H + k);
        p += k;
      }
    }
  };
  if (s->incremental) {
    each_block([&](int, bool, int, int64_t, int64_t k) {
      packed += H + k;
      ++n_blocks;
    });
  } else {
    // first pass over the geometry only: the three maps are laid out behind
    // one another, so their length must be known before they are written
    int cur_rows = 0;
    for (int i = 0; i < n; ++i) {
      int64_t left = h_rows_out[i];
      while (left > 0) {
        int64_t room = kMaxRows - cur_rows - L - R;
        if (room < left && cur_rows > 0) {
          cur_rows = 0;
          room = kMaxRows - L - R;
        }
        const int64_t k = std::min(left, room);
        cur_rows += (int)(k + L + R);
        packed += k + L + R;
        left -= k;
      }
    }
  }
  if (packed > s->max_packed) return fail(CE_GPU_EINVAL, "sessions_push: internal: map bound exceeded");
  int32_t *dst = src + packed;
  uint32_t *edge = reinterpret_cast<uint32_t *>(dst + packed);
  const size_t o_blocks = align16(o_maps + 12 * (size_t)packed);
  const size_t used = s->incremental ? o_blocks + sizeof(SessionBlock) * (size_t)n_blocks : o_maps + 12 * (size_t)packed;
  if (used > s->desc_bytes || n_blocks > s->max_blocks)
    return fail(CE_GPU_EINVAL, "sessions_push: internal: descriptor bound exceeded");
  if (s->incremental) {
    // block row j holds position p - H + j: the frame of that position from
    // the ring (clamped to [0, last], which is the padding), an output row
    // for the new rows at positions >= L + R
    SessionBlock *blk = reinterpret_cast<SessionBlock *>(h + o_blocks);
    Chunk cur;
    int64_t at = 0, nb = 0, out_base = 0;
    int out_of = 0;
    each_block([&](int i, bool fresh_chunk, int row0, int64_t p, int64_t k) {
      if (fresh_chunk) {
        s->chunks.push_back(cur);
        cur = Chunk();
        cur.map_base = at;
        cur.blk_base = (int)nb;
      }
      const Slot &was = s->slots[h_slot[i]], &nx = s->next[i];
      for (; out_of < i; ++out_of) out_base += h_rows_out[out_of];  // the rows of the pushes before i
      const int64_t ring_base = (int64_t)h_slot[i] * s->norm_cap, last = nx.frames - 1;
      const int64_t seg_rows = H + k;
      for (int64_t j = 0; j < seg_rows; ++j, ++at) {
        const uint32_t dl = (uint32_t)std::min<int64_t>(j, 0xffff), dr = (uint32_t)std::min<int64_t>(seg_rows - 1 - j, 0xffff);
        edge[at] = dl | (dr << 16);
        const int64_t q = p - H + j;
        int64_t fr = q - L;
        fr = fr < 0 ? 0 : (fr > last ? last : fr);
        src[at] = (int32_t)(ring_base + fr % s->norm_cap);
        dst[at] = j >= H && q >= L + R ? (int32_t)(out_base + (q - L - R - was.rows)) : -1;
      }
      SessionBlock &b = blk[nb++];
      b.slot = h_slot[i];
      b.row0 = row0;
      b.k = (int32_t)k;
      b.fresh = p == 0;
      cur.rows += (int)seg_rows;
      ++cur.n_blocks;
    });
    if (cur.rows > 0) s->chunks.push_back(cur);
  } else {
    Chunk cur;
    int64_t at = 0, out_base = 0;
    auto close = [&]() {
      if (cur.rows > 0) s->chunks.push_back(cur);
      cur = Chunk();
      cur.map_base = at;
    };
    for (int i = 0; i < n; ++i) {
      const Slot &was = s->slots[h_slot[i]], &nx = s->next[i];
      const int64_t ring_base = (int64_t)h_slot[i] * s->norm_cap;
      const int64_t last = nx.frames - 1;  // right context clamps here (only an EOS push reaches it)
      int64_t t = was.rows;
      while (t < nx.rows) {
        int64_t room = kMaxRows - cur.rows - L - R;
        if (room < nx.rows - t && cur.rows > 0) {
          close();
          room = kMaxRows - L - R;
        }
        const int64_t k = std::min(nx.rows - t, room), seg_rows = k + L + R;
        for (int64_t j = 0; j < seg_rows; ++j, ++at) {
          const uint32_t dl = (uint32_t)std::min<int64_t>(j, 0xffff), dr = (uint32_t)std::min<int64_t>(seg_rows - 1 - j, 0xffff);
          edge[at] = dl | (dr << 16);
          int64_t fr = t - L + j;
          fr = fr < 0 ? 0 : (fr > last ? last : fr);
          src[at] = (int32_t)(ring_base + fr % s->norm_cap);
          dst[at] = j >= L && j < L + k ? (int32_t)(out_base + (t - was.rows) + (j - L)) : -1;
        }
        cur.rows += (int)seg_rows;
        t += k;
      }
      out_base += nx.rows - was.rows;
    }
    close();
  }
  hipStream_t st = ctx->stream;
  CE_HIP(hipMemcpyAsync(s->desc.ptr, h, used, hipMemcpyHostToDevice, st));
  CE_HIP(hipEventRecord(re.copied, st));
  re.in_use = true;
  s->ring_at = (s->ring_at + 1) % kRing;

  // 3. the launches
  const char *d = static_cast<const char *>(s->desc.ptr);
  const SessionPush *d_push = reinterpret_cast<const SessionPush *>(d + o_push);
  float *stage = s->stage.as<float>();
  if (total_samples > 0) {
    if (std::is_same<Sample, int16_t>::value)
      CE_TRY(launch_session_stage_s16(st, d_push, n, max_new, reinterpret_cast<const int16_t *>(d_pcm), stage, s->stride));
    else
      CE_TRY(launch_session_stage(st, d_push, n, max_new, reinterpret_cast<const float *>(d_pcm), stage, s->stride));
  }
  if (total_frames > 0) {
    {
      ProfScope prof(ctx, CE_GPU_PROF_FBANK);
      const FbankTables *tab = ctx->d_tables.as<FbankTables>();
      const int64_t *d_soff = reinterpret_cast<const int64_t *>(d + o_soff);
      const int64_t *d_foff = reinterpret_cast<const int64_t *>(d + o_foff);
      const int *d_butt = reinterpret_cast<const int *>(d + o_butt);
      CE_TRY(ctx->fbank_mode == CE_GPU_FBANK_FAST
                 ? launch_fbank_fma(st, tab, d_soff, d_foff, d_butt, total_frames, stage, s->tmp.as<float>(), nullptr)
                 : launch_fbank(st, tab, d_soff, d_foff, d_butt, total_frames, stage, s->tmp.as<float>(), nullptr));
    }
    CE_TRY(launch_session_carry(st, d_push, n, stage, s->stride));
    ProfScope prof(ctx, CE_GPU_PROF_CMVN);
    CE_TRY(launch_session_cmvn(st, d_push, n, (int)total_frames, s->gstats, s->tmp.as<float>(), s->raw.as<float>(),
                               s->raw_cap, s->norm.as<float>(), s->norm_cap, s->carry.as<float>()));
  }
  const int *d_src = reinterpret_cast<const int *>(d + o_maps);
  const int *d_dst = d_src + packed;
  const uint32_t *d_edge = reinterpret_cast<const uint32_t *>(d_dst + packed);
  IncrChunk inc;
  inc.lead = H;
  inc.layers = s->layers.data();
  inc.n_layers = (int)s->layers.size();
  for (const Chunk &c : s->chunks) {
    inc.blocks = reinterpret_cast<const SessionBlock *>(d + o_blocks) + c.blk_base;
    inc.n_blocks = c.n_blocks;
    CE_TRY(score_packed_rows(ctx, m, s->norm.as<float>(), c.rows, d_src + c.map_base, d_edge + c.map_base,
                             d_dst + c.map_base, d_loglik, s->incremental ? &inc : nullptr));
  }
  for (int i = 0; i < n; ++i) s->slots[h_slot[i]] = s->next[i];
  ++s->n_pushes;
  s->n_packed += packed;
  s->n_chunks += (int64_t)s->chunks.size();
  return CE_GPU_OK;
}

// The caches of an incremental set: per Linear after the first, c rows per
// slot of the widest representation its input can have (fp32), and their row
// sums; H = the largest c of any Linear.
int create_caches(ce_gpu_sessions *s) {
  const ce_gpu_model *m = s->m;
  if (!m->int8_static && m->gemm != CE_GPU_GEMM_FP32 && m->gemm != CE_GPU_GEMM_BF16X6 && m->gemm != CE_GPU_GEMM_BF16)
    return fail(CE_GPU_ENOTSUP, "sessions_create_ex: incremental sets take GEMM modes fp32, bf16x6 and bf16");
  int sum_hi = 0, sum_lo = 0, prev_n = 0;
  size_t bytes = 0, words = 0;
  for (const Step &st : m->steps) {
    if (!st.is_gemm) continue;
    const GemmLayer &g = st.gemm;
    int lo = g.off[0], hi = g.off[0];
    for (int i = 1; i < g.nseg; ++i) lo = std::min(lo, g.off[i]), hi = std::max(hi, g.off[i]);
    // the loaders carry a splice offset as a signed byte
    if (lo - hi < -127) return fail(CE_GPU_ENOTSUP, "sessions_create_ex: a layer's splice span exceeds 127 rows");
    sum_lo += lo, sum_hi += hi;
    IncrLayer l;
    l.c = hi - lo;
    s->H = std::max(s->H, l.c);
    if (!s->layers.empty() && l.c > 0) {
      if (g.din != prev_n) return fail(CE_GPU_ENOTSUP, "sessions_create_ex: a layer's input is not the previous layer's output");
      l.row_cap = (size_t)((g.din + 31) / 32 * 32) * sizeof(float);
      bytes += (size_t)s->n_slots * l.c * l.row_cap;
      words += (size_t)s->n_slots * l.c;
    }
    s->layers.push_back(l);
    prev_n = g.n;
  }
  // position p = output time p - L - R only if the offsets add up to the context
  if (-sum_lo != s->L || sum_hi != s->R)
    return fail(CE_GPU_ENOTSUP, "sessions_create_ex: the layers' splice offsets do not add up to the model's context");
  if (s->H >= kMaxRows) return fail(CE_GPU_EINVAL, "sessions_create_ex: nnet context too large");
  if (bytes == 0) return CE_GPU_OK;
  CE_TRY(s->cache.alloc(bytes));
  CE_TRY(s->cache_sums.alloc(words * sizeof(int32_t)));
  char *at = s->cache.as<char>();
  int32_t *sums = s->cache_sums.as<int32_t>();
  for (size_t i = 1; i < s->layers.size(); ++i) {
    IncrLayer &l = s->layers[i];
    if (l.c == 0) continue;
    l.cache = at;
    l.sums = sums;
    at += (size_t)s->n_slots * l.c * l.row_cap;
    sums += (size_t)s->n_slots * l.c;
  }
  return CE_GPU_OK;
}

}  // namespace

extern "C" {

int ce_gpu_sessions_create(ce_gpu_ctx *ctx, const ce_gpu_model *m, const float *d_global_stats, int n_slots,
                           int max_chunk_samples, ce_gpu_sessions **out) {
  return ce_gpu_sessions_create_ex(ctx, m, d_global_stats, n_slots, max_chunk_samples, 0, out);
}

int ce_gpu_sessions_create_ex(ce_gpu_ctx *ctx, const ce_gpu_model *m, const float *d_global_stats, int n_slots,
                              int max_chunk_samples, unsigned flags, ce_gpu_sessions **out) {
  if (!out) return fail(CE_GPU_EINVAL, "out is NULL");
  *out = nullptr;
  if (!ctx || !m || n_slots < 1 || n_slots > 65535 || max_chunk_samples < 1)
    return fail(CE_GPU_EINVAL, "sessions_create: bad argument");
  if (flags & ~CE_GPU_SESSIONS_INCREMENTAL) return fail(CE_GPU_EINVAL, "sessions_create_ex: unknown flag");
  // a static int8 model (frozen activation parameters) scores a row from its
  // own input rows alone, like the fp32 forms
  if (m->int8 && !m->int8_static)
    return fail(CE_GPU_ENOTSUP, "sessions_create: an int8 model's rows depend on the batch they are scored in");
  if (m->input_dim != kMel) return fail(CE_GPU_EINVAL, "sessions_create: nnet input is not 40-dim fbank");
  if (!m->log_prior.ptr) return fail(CE_GPU_EINVAL, "sessions_create: needs a model loaded with a prior");
  if (m->left != m->net_left || m->right != m->net_right)
    return fail(CE_GPU_EINVAL, "sessions_create: model context differs from its network's");
  if (m->left + m->right + 1 > kMaxRows) return fail(CE_GPU_EINVAL, "sessions_create: nnet context too large");
  if (ctx->sessions) return fail(CE_GPU_EINVAL, "sessions_create: the context already has a session set");
  CE_HIP(hipSetDevice(ctx->device));
  std::unique_ptr<ce_gpu_sessions> s(new (std::nothrow) ce_gpu_sessions());
  if (!s) return fail(CE_GPU_ENOMEM, "out of host memory");
  s->ctx = ctx;
  s->m = m;
  s->static_int8 = m->int8_static;
  s->gemm = m->gemm;
  s->incremental = (flags & CE_GPU_SESSIONS_INCREMENTAL) != 0;
  s->gstats = d_global_stats;
  s->n_slots = n_slots;
  s->max_chunk = max_chunk_samples;
  const int L = s->L = m->left, R = s->R = m->right;
  const int64_t max_frames = ce_gpu_fbank_num_frames((int64_t)kWinLen - 1 + max_chunk_samples);
  s->max_frames = (int)max_frames;
  s->raw_cap = (int)(kWindow + max_frames);
  s->norm_cap = (int)(L + R + max_frames + 1);
  // [tail | new chunk], every region 16-byte aligned
  s->stride = ((int64_t)kWinLen - 1 + max_chunk_samples + 3) / 4 * 4;
  if ((int64_t)n_slots * s->norm_cap >= INT32_MAX || (int64_t)n_slots * max_frames >= INT32_MAX)
    return fail(CE_GPU_EINVAL, "sessions_create: n_slots x max_chunk_samples too large");
  // a slot's push emits at most max_frames + R rows (EOS releases the R held back)
  const int64_t rows_max = max_frames + R, segs = rows_max / (kMaxRows - L - R) + 2;
  s->max_packed = (int64_t)n_slots * (rows_max + segs * (L + R));
  if (s->incremental) {
    CE_TRY(create_caches(s.get()));
    // a slot's push feeds at most L + max_frames + R positions, every block
    // of them behind H lead rows
    const int64_t pos_max = L + max_frames + R, blocks = pos_max / (kMaxRows - s->H) + 2;
    s->max_blocks = (int64_t)n_slots * blocks;
    s->max_packed = (int64_t)n_slots * (pos_max + blocks * s->H);
  }
  s->slots.assign(n_slots, Slot());
  s->next.assign(n_slots, Slot());
  s->seen.assign(n_slots, 0);
  s->chunks.reserve((size_t)(s->max_packed / (kMaxRows / 2) + n_slots + 2));
  const int fpb = fbank_frames_per_block();
  s->desc_bytes = align16(sizeof(SessionPush) * n_slots) + 2 * align16(8 * (size_t)(n_slots + 1)) +
                  align16(4 * (size_t)((int64_t)n_slots * max_frames / fpb + 2)) + 12 * (size_t)s->max_packed + 64 +
                  sizeof(SessionBlock) * (size_t)s->max_blocks;
  const size_t f = sizeof(float);
  CE_TRY(s->stage.alloc((size_t)n_slots * s->stride * f));
  CE_TRY(s->tmp.alloc((size_t)n_slots * max_frames * kMel * f));
  CE_TRY(s->norm.alloc((size_t)n_slots * s->norm_cap * kMel * f));
  if (d_global_stats) {
    CE_TRY(s->raw.alloc((size_t)n_slots * s->raw_cap * kMel * f));
    CE_TRY(s->carry.alloc((size_t)n_slots * kMel * f));
  }
  CE_TRY(s->desc.alloc(s->desc_bytes));
  for (RingEntry &re : s->ring) {
    CE_HIP(hipHostMalloc(&re.host, s->desc_bytes, hipHostMallocDefault));
    count_device_alloc();
    CE_HIP(hipEventCreateWithFlags(&re.copied, hipEventDisableTiming));
    count_device_alloc();
  }
  // everything a chunk of packed rows needs, in every mode the model and the
  // context can be switched to
  CE_TRY(reserve_packed_rows(ctx, m, (int)std::min<int64_t>(kMaxRows, s->max_packed)));
  ctx->sessions = s.get();
  *out = s.release();
  return CE_GPU_OK;
}

int ce_gpu_sessions_destroy(ce_gpu_sessions *s) {
  if (!s) return CE_GPU_OK;
  (void)hipSetDevice(s->ctx->device);
  (void)hipStreamSynchronize(s->ctx->stream);  // pushes still in flight read the buffers freed below
  for (RingEntry &re : s->ring) {
    if (re.copied) {
      (void)hipEventDestroy(re.copied);
      count_device_free();
    }
    if (re.host) {
      (void)hipHostFree(re.host);
      count_device_free();
    }
  }
  if (s->ctx->sessions == s) s->ctx->sessions = nullptr;
  delete s;
  return CE_GPU_OK;
}

int ce_gpu_sessions_stats(const ce_gpu_sessions *s, int *lead_rows, int64_t *pushes, int64_t *packed_rows,
                          int64_t *chunks) {
  if (!s) return fail(CE_GPU_EINVAL, "sessions_stats: bad argument");
  if (lead_rows) *lead_rows = s->incremental ? s->H : 0;
  if (pushes) *pushes = s->n_pushes;
  if (packed_rows) *packed_rows = s->n_packed;
  if (chunks) *chunks = s->n_chunks;
  return CE_GPU_OK;
}

int ce_gpu_sessions_reset(ce_gpu_sessions *s, int slot) {
  if (!s || slot < 0 || slot >= s->n_slots) return fail(CE_GPU_EINVAL, "sessions_reset: bad argument");
  // the device state needs no touch: a slot at frame 0 with an empty tail
  // reads neither its carry nor its rings before it has rewritten them (nor,
  // in an incremental set, its caches: at position 0 its blocks are fresh)
  s->slots[slot] = Slot();
  return CE_GPU_OK;
}

int ce_gpu_debug_fill_sessions(ce_gpu_sessions *s, uint32_t word, int n, const int32_t *h_slots) {
  if (!s || n < 0 || (n > 0 && !h_slots)) return fail(CE_GPU_EINVAL, "debug_fill_sessions: bad argument");
  for (int i = 0; i < n; ++i)
    if (h_slots[i] < 0 || h_slots[i] >= s->n_slots) return fail(CE_GPU_EINVAL, fmt("debug_fill_sessions: no slot %d", h_slots[i]));
  CE_HIP(hipSetDevice(s->ctx->device));
  hipStream_t st = s->ctx->stream;
  // per-push scratch: a push writes what it reads of both
  CE_TRY(debug_fill(st, s->tmp.ptr, s->tmp.bytes, word));
  CE_TRY(debug_fill(st, s->desc.ptr, s->desc.bytes, word));
  const size_t f = sizeof(float);
  for (int i = 0; i < n; ++i) {
    const size_t k = (size_t)h_slots[i];
    CE_TRY(debug_fill(st, s->stage.as<float>() + k * s->stride, (size_t)s->stride * f, word));
    CE_TRY(debug_fill(st, s->norm.as<float>() + k * s->norm_cap * kMel, (size_t)s->norm_cap * kMel * f, word));
    if (s->raw.ptr) CE_TRY(debug_fill(st, s->raw.as<float>() + k * s->raw_cap * kMel, (size_t)s->raw_cap * kMel * f, word));
    if (s->carry.ptr) CE_TRY(debug_fill(st, s->carry.as<float>() + k * kMel, kMel * f, word));
    // incremental: the slot's c rows of every cached layer (IncrLayer)
    for (const IncrLayer &l : s->layers) {
      if (!l.cache) continue;
      CE_TRY(debug_fill(st, l.cache + k * l.c * l.row_cap, (size_t)l.c * l.row_cap, word));
      CE_TRY(debug_fill(st, l.sums + k * l.c, (size_t)l.c * sizeof(int32_t), word));
    }
  }
  return CE_GPU_OK;
}

int ce_gpu_sessions_push(ce_gpu_sessions *s, int n, const int32_t *h_slot, const int32_t *h_num_samples,
                         const int32_t *h_flags, const float *d_pcm, float *d_loglik, int64_t capacity_rows,
                         int32_t *h_rows_out) {
  return push_t(s, n, h_slot, h_num_samples, h_flags, d_pcm, d_loglik, capacity_rows, h_rows_out);
}

int ce_gpu_sessions_push_s16(ce_gpu_sessions *s, int n, const int32_t *h_slot, const int32_t *h_num_samples,
                             const int32_t *h_flags, const int16_t *d_pcm, float *d_loglik, int64_t capacity_rows,
                             int32_t *h_rows_out) {
  return push_t(s, n, h_slot, h_num_samples, h_flags, d_pcm, d_loglik, capacity_rows, h_rows_out);
}

}  // extern "C"
