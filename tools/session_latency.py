"""Wall time per tick of a serving loop on TDNN-S in latency mode: N live
streams, each delivering 1600 samples (100 ms) per tick, without CMVN.

  sessions  one ce_gpu_sessions_push for all N slots (state on the device);
  legacy    what a caller does today per stream and chunk through the rest
            of the ABI: the sample tail carried on the host, a
            ce_gpu_plan_create + ce_gpu_fbank for the chunk, the last L + R
            feature rows carried (here on the device, the cheaper way) and a
            ce_gpu_nnet_propagate over [context | new frames].

Both legs start from the tick's PCM in host memory and end in a device
synchronise; a host clock brackets each tick.  Per N the two legs alternate
in blocks of `ticks` ticks, `rounds` times, after a warm-up block of each;
reported are the median and the 10th / 90th percentile over all timed ticks.
Both legs compute the same rows (checked once per N, bit for bit).

  python tools/session_latency.py [ticks] [rounds]      -> JSON lines
  python tools/session_latency.py --static-int8 --renorm [ticks] [rounds] [--slots N] [--tick-ms T]
      the relu-renorm model in static int8, incremental and plain sets, see
      incremental()
  python tools/session_latency.py --static-int8 [ticks] [rounds]
      the 64-stream push only: the bf16x6 latency-mode model beside a static
      int8 model (ce_gpu_model_quantize_static) on a throughput context and
      on a latency-mode context, see static_int8()
  python tools/session_latency.py --incremental [--slots N] [--tick-ms T] [ticks] [rounds]
      an incremental set (CE_GPU_SESSIONS_INCREMENTAL) beside a plain one,
      in three forms of the model, see incremental()
  python tools/session_latency.py --incremental --bf16 [--slots N] [--tick-ms T] [ticks] [rounds]
      the same for the plain bf16 model alone, on a throughput context (form
      bf16) and on a latency context (form bf16_latency: pushes that pack at
      most ce_gpu_bf16_latency_max_rows rows run on the latency kernel)"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from catears_amd import gpu, synth  # noqa: E402

CHUNK = 1600


class Legacy:
    """One stream through plan_create + fbank + nnet_propagate."""

    def __init__(self, ctx, model):
        self.ctx, self.model = ctx, model
        self.tail = np.zeros(0, np.float32)
        self.feats = None  # rows not yet scored with their left context, on the device
        self.frames = 0

    def push(self, pcm):
        L, R = self.model.left, self.model.right
        x = np.concatenate([self.tail, pcm])
        n = gpu.num_frames(len(x))
        if n == 0:
            self.tail = x
            return None
        self.tail = x[160 * n:]
        plan = gpu.Plan(self.ctx, [len(x)])
        new = gpu.fbank(self.ctx, plan, torch.from_numpy(x).cuda())
        plan.close()
        if self.feats is None:  # left context of the utterance: frame 0, L times
            self.feats = torch.cat([new[:1].expand(L, 40), new])
        else:
            self.feats = torch.cat([self.feats, new])
        out = None
        if self.feats.shape[0] > L + R:
            out = gpu.nnet_propagate(self.ctx, self.model, self.feats.contiguous(), subtract_prior=True)
            self.feats = self.feats[self.feats.shape[0] - L - R:]
        return out


def pct(v, q):
    return float(np.percentile(np.asarray(v), q))


def main(ticks=100, rounds=3):
    mdir = os.path.join(tempfile.gettempdir(), f"catears_bench_{os.getuid()}")
    conf = synth.write_model(mdir, "tdnn-s")
    ctx = gpu.Context(0)
    ctx.set_latency(True)
    model = gpu.Model(ctx, conf)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "model": "tdnn-s", "mode": "latency",
                      "chunk_samples": CHUNK, "ticks": ticks, "rounds": rounds, "version":
                      gpu.lib().ce_gpu_version().decode()}), flush=True)
    for n in (1, 16, 64):
        total = CHUNK * ticks * (rounds + 1)
        waves = [synth.pcm(3000 + s, total) for s in range(n)]
        sess = gpu.Sessions(ctx, model, n, CHUNK)
        legacy = [Legacy(ctx, model) for _ in range(n)]
        out = torch.empty((n * 16, model.num_pdfs), dtype=torch.float32, device="cuda")
        slots = list(range(n))
        t_sess, t_leg = [], []
        rows_sess = [[] for _ in range(n)]
        rows_leg = [[] for _ in range(n)]

        def sess_tick(t, keep):
            at = t * CHUNK
            pcm = np.concatenate([w[at:at + CHUNK] for w in waves])
            t0 = time.perf_counter()
            o, rows = sess.push(slots, torch.from_numpy(pcm).cuda(), [CHUNK] * n, out=out)
            ctx.synchronize()
            dt = time.perf_counter() - t0
            if keep:
                h, k = o.cpu().numpy(), 0
                for s in range(n):
                    rows_sess[s].append(h[k:k + rows[s]])
                    k += rows[s]
            return dt

        def leg_tick(t, keep):
            at = t * CHUNK
            t0 = time.perf_counter()
            outs = [legacy[s].push(waves[s][at:at + CHUNK]) for s in range(n)]
            ctx.synchronize()
            dt = time.perf_counter() - t0
            if keep:
                for s in range(n):
                    if outs[s] is not None:
                        rows_leg[s].append(outs[s].cpu().numpy())
            return dt

        # every block continues the streams where the last one stopped, so
        # both legs see the same audio at the same tick
        for r in range(rounds + 1):
            first = r * ticks
            a = [sess_tick(first + i, r == 0) for i in range(ticks)]
            b = [leg_tick(first + i, r == 0) for i in range(ticks)]
            if r:  # block 0 is the warm-up
                t_sess += a
                t_leg += b
        same = all(np.array_equal(np.concatenate(rows_sess[s]).view(np.uint32),
                                  np.concatenate(rows_leg[s]).view(np.uint32)) for s in range(n))
        sess.close()
        rec = {"slots": n, "timed_ticks": len(t_sess), "rows_identical": bool(same)}
        for name, v in (("sessions", t_sess), ("legacy", t_leg)):
            rec[name] = {"median_us": round(pct(v, 50) * 1e6, 1), "p10_us": round(pct(v, 10) * 1e6, 1),
                         "p90_us": round(pct(v, 90) * 1e6, 1)}
        rec["legacy_over_sessions"] = round(pct(t_leg, 50) / pct(t_sess, 50), 2)
        print(json.dumps(rec), flush=True)


def static_int8(ticks=100, rounds=3, n=64):
    """The n-stream push with a static int8 model (calibrated on 12 s of the
    synthetic audio, no CMVN) beside the bf16x6 latency-mode push of main(),
    and the same static int8 model on a latency-mode context (the split-K
    int8 pair where the slice rule gives it the push's row count, the
    throughput kernel above the crossover: same rows, checked on the last
    tick): three contexts, one session set each, alternating blocks of
    `ticks` ticks."""
    mdir = os.path.join(tempfile.gettempdir(), f"catears_bench_{os.getuid()}")
    conf = synth.write_model(mdir, "tdnn-s")
    ctx_x6 = gpu.Context(0)
    ctx_x6.set_latency(True)
    ctx_i8 = gpu.Context(0)
    m_x6, m_i8 = gpu.Model(ctx_x6, conf), gpu.Model(ctx_i8, conf)
    cal = [synth.pcm(2900 + i, 48000) for i in range(4)]
    plan = gpu.Plan(ctx_i8, [len(w) for w in cal], m_i8)
    ranges = m_i8.calibrate(ctx_i8, plan, gpu.fbank(ctx_i8, plan, torch.from_numpy(np.concatenate(cal)).cuda()))
    m_i8.quantize_static(ctx_i8, ranges)
    ctx_i8l = gpu.Context(0)
    ctx_i8l.set_latency(True)
    m_i8l = gpu.Model(ctx_i8l, conf).quantize_static(ctx_i8l, ranges)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "model": "tdnn-s", "chunk_samples": CHUNK,
                      "slots": n, "ticks": ticks, "rounds": rounds, "legs": ["bf16x6 latency", "static int8", "static int8 latency"],
                      "version": gpu.lib().ce_gpu_version().decode()}), flush=True)
    total = CHUNK * ticks * (rounds + 1)
    waves = [synth.pcm(3000 + s, total) for s in range(n)]
    legs = [(ctx_x6, gpu.Sessions(ctx_x6, m_x6, n, CHUNK)), (ctx_i8, gpu.Sessions(ctx_i8, m_i8, n, CHUNK)),
            (ctx_i8l, gpu.Sessions(ctx_i8l, m_i8l, n, CHUNK))]
    out = torch.empty((n * 16, m_x6.num_pdfs), dtype=torch.float32, device="cuda")
    slots, times = list(range(n)), ([], [], [])
    counters = None
    last = [None, None, None]
    lat0 = gpu.debug_i8_latency_launches()
    for r in range(rounds + 1):
        for k, (ctx, sess) in enumerate(legs):
            for t in range(r * ticks, (r + 1) * ticks):
                pcm = np.concatenate([w[t * CHUNK:(t + 1) * CHUNK] for w in waves])
                t0 = time.perf_counter()
                o, _ = sess.push(slots, torch.from_numpy(pcm).cuda(), [CHUNK] * n, out=out)
                ctx.synchronize()
                if r:  # block 0 is the warm-up
                    times[k].append(time.perf_counter() - t0)
            last[k] = o.cpu().numpy().copy()
        if r == 0:
            counters = gpu.debug_counters()
    rec = {"slots": n, "timed_ticks": len(times[0]), "pushes_allocated_nothing": gpu.debug_counters() == counters,
           "static_int8_rows_identical": bool(np.array_equal(last[1].view(np.uint32), last[2].view(np.uint32))),
           "i8_latency_gemm_launches": gpu.debug_i8_latency_launches() - lat0}
    for name, v in (("bf16x6_latency", times[0]), ("static_int8", times[1]), ("static_int8_latency", times[2])):
        rec[name] = {"median_us": round(pct(v, 50) * 1e6, 1), "p10_us": round(pct(v, 10) * 1e6, 1),
                     "p90_us": round(pct(v, 90) * 1e6, 1)}
    rec["static_int8_over_bf16x6"] = round(pct(times[1], 50) / pct(times[0], 50), 2)
    rec["static_int8_latency_over_static_int8"] = round(pct(times[2], 50) / pct(times[1], 50), 2)
    print(json.dumps(rec), flush=True)
    for _, sess in legs:
        sess.close()


def renorm_image():
    """The TDNN-S shape with every BatchNorm replaced by Normalize (the
    relu-renorm TDNN of tools/row_ops.py): (NN02 image, prior)."""
    from catears_amd import formats
    spec = synth.MODELS["tdnn-s"]
    layers, left, right, prior = synth.tdnn_layers(spec["hidden"], spec["pdfs"])
    layers = [{"kind": "normalize"} if L["kind"] == "batchnorm" else L for L in layers]
    return formats.nnet_bytes(layers, left, right), prior


def incremental(ticks=100, rounds=3, n=64, tick_ms=100, forms=("static_int8_latency", "bf16", "bf16x6_latency"),
                renorm=False):
    """N running streams, tick_ms of audio per slot and push, no CMVN: an
    incremental set and a plain (flags = 0) set of the same model on two
    contexts, in alternating blocks of `ticks` pushes, for static int8 and
    bf16x6 (both on latency-mode contexts) and plain bf16.  The tick's PCM is
    already on the device (the same buffer every tick: 13 MB a tick at 2048
    slots would otherwise be most of what is timed); a host clock brackets
    push + synchronise.  Packed rows per push from ce_gpu_sessions_stats; the
    last tick's rows of the two sets are compared bit for bit.
    renorm (--static-int8 --renorm): the relu-renorm model, whose row steps
    write the next layer's bytes, in the static int8 forms only -- latency
    mode on and off; time one library per process (CATEARS_HIP_LIB)."""
    mdir = os.path.join(tempfile.gettempdir(), f"catears_bench_{os.getuid()}")
    conf = synth.write_model(mdir, "tdnn-s")
    image, prior = renorm_image() if renorm else (None, None)
    chunk = 16 * tick_ms
    print(json.dumps({"device": torch.cuda.get_device_name(0), "model": "tdnn-s renorm" if renorm else "tdnn-s",
                      "library": os.path.relpath(gpu.LIB_PATH), "slots": n, "tick_ms": tick_ms,
                      "ticks": ticks, "rounds": rounds, "legs": ["incremental", "plain"],
                      "version": gpu.lib().ce_gpu_version().decode()}), flush=True)
    cal = [synth.pcm(2900 + i, 48000) for i in range(4)]
    base = np.stack([synth.pcm(3000 + s, 4000 + chunk) for s in range(8)])
    lead = torch.from_numpy(np.concatenate([np.roll(base[s % 8], 5 * s)[:4000] for s in range(n)])).cuda()
    tick = torch.from_numpy(np.concatenate([np.roll(base[s % 8], 5 * s)[4000:] for s in range(n)])).cuda()
    slots = list(range(n))
    for form in forms:
        legs = []
        for inc in (True, False):
            ctx = gpu.Context(0)
            model = gpu.Model(ctx, image=image, prior=prior) if renorm else gpu.Model(ctx, conf)
            if form not in ("bf16", "static_int8"):
                ctx.set_latency(True)
            if form in ("bf16", "bf16_latency"):
                model.set_gemm("bf16")
            if form in ("static_int8_latency", "static_int8"):
                plan = gpu.Plan(ctx, [len(w) for w in cal], model)
                model.quantize_static(ctx, model.calibrate(
                    ctx, plan, gpu.fbank(ctx, plan, torch.from_numpy(np.concatenate(cal)).cuda())))
                plan.close()
            sess = gpu.Sessions(ctx, model, n, 4000, incremental=inc)
            sess.push(slots, lead, [4000] * n)  # every slot running: 23 frames, 13 rows out
            legs.append((ctx, model, sess))
        out = torch.empty((n * (chunk // 160 + 1), legs[0][1].num_pdfs), dtype=torch.float32, device="cuda")
        times, packed, last = ([], []), [0, 0], [None, None]
        counters = None
        # absent from libraries older than the bf16 latency mode (A/B runs)
        b16_launches = getattr(gpu, "debug_bf16_latency_launches", lambda: 0)
        b16_0 = b16_launches()
        for r in range(rounds + 1):
            for k, (ctx, _, sess) in enumerate(legs):
                before = sess.stats()
                for _ in range(ticks):
                    t0 = time.perf_counter()
                    o, _rows = sess.push(slots, tick, [chunk] * n, out=out)
                    ctx.synchronize()
                    if r:  # block 0 is the warm-up
                        times[k].append(time.perf_counter() - t0)
                after = sess.stats()
                packed[k] = (after["packed_rows"] - before["packed_rows"]) // ticks
                chunks = (after["chunks"] - before["chunks"]) // ticks
                last[k] = (o.cpu().numpy().copy(), chunks)
            if r == 0:
                counters = gpu.debug_counters()
        rec = {"form": form, "slots": n, "tick_ms": tick_ms, "timed_pushes": len(times[0]),
               "lead_rows": legs[0][2].stats()["lead_rows"],
               "pushes_allocated_nothing": gpu.debug_counters() == counters,
               "bf16_latency_gemm_launches": b16_launches() - b16_0,
               "rows_identical": bool(np.array_equal(last[0][0].view(np.uint32), last[1][0].view(np.uint32)))}
        for k, name in enumerate(("incremental", "plain")):
            v = times[k]
            rec[name] = {"packed_rows_per_push": packed[k], "chunks_per_push": last[k][1],
                         "median_us": round(pct(v, 50) * 1e6, 1), "p10_us": round(pct(v, 10) * 1e6, 1),
                         "p90_us": round(pct(v, 90) * 1e6, 1)}
        rec["plain_over_incremental"] = round(pct(times[1], 50) / pct(times[0], 50), 3)
        print(json.dumps(rec), flush=True)
        for _, _, sess in legs:
            sess.close()


def flag(name, default):
    argv = sys.argv[1:]
    return int(argv[argv.index(name) + 1]) if name in argv else default


if __name__ == "__main__":
    argv = sys.argv[1:]
    valued = {i + 1 for i, v in enumerate(argv) if v in ("--slots", "--tick-ms")}
    nums = [int(v) for i, v in enumerate(argv) if not v.startswith("--") and i not in valued][:2]
    if "--static-int8" in argv and "--renorm" in argv:
        incremental(*(nums + [100, 3][len(nums):]), n=flag("--slots", 64), tick_ms=flag("--tick-ms", 100),
                    forms=("static_int8_latency", "static_int8"), renorm=True)
    elif "--incremental" in argv and "--bf16" in argv:
        incremental(*(nums + [100, 3][len(nums):]), n=flag("--slots", 64), tick_ms=flag("--tick-ms", 100),
                    forms=("bf16", "bf16_latency"))
    elif "--incremental" in argv:
        incremental(*(nums + [100, 3][len(nums):]), n=flag("--slots", 64), tick_ms=flag("--tick-ms", 100))
    elif "--static-int8" in sys.argv[1:]:
        static_int8(*nums)
    else:
        main(*nums)
