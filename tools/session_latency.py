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

  python tools/session_latency.py [ticks] [rounds]      -> JSON lines"""
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


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:3]])
