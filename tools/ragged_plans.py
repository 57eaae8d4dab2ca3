"""What a reusable plan buys a server that scores ragged batches (the C4 shape)
whose composition is new on every call, on one MI355X: one JSON object on
stdout.
   python tools/ragged_plans.py [passes] [utterances]

The stream: the first `utterances` (default 240) utterances of the C4 length
mix (catears_amd.shard.c4_corpus: 2-18 s, 10 s on average) packed into batches
of at most 4096 rows as bench.py packs them, int16 PCM resident on the device,
TDNN-S, CMVN on.  The batches go round-robin to 1 and to 4 contexts, each on a
stream of its own, issued by one host thread; nothing waits for the device
until the pass ends.  Two ways to describe a batch to the library:

  create   ce_gpu_plan_create + ce_gpu_score_s16 + ce_gpu_plan_destroy per
           batch (six allocations with a null-stream copy each, six releases);
  assign   ce_gpu_plan_assign on the context's reusable plan + ce_gpu_score_s16
           (a library without reusable plans runs the create legs only).

Per context count the legs run create / assign / assign / create; a leg is
`passes` passes over the stream after one warm-up pass.  Reported per leg: the
median over its passes of the wall time per batch (us), the 10th and 90th
percentile, the median host time of describing one batch (create + destroy
against assign) and a digest of the last pass's rows -- create and assign must
agree.  One process times one library (CATEARS_HIP_LIB, or the tree the tool
is run from): run this library and the parent's as processes in A B B A
order and compare the create legs across them."""
import hashlib
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from catears_amd import gpu, synth  # noqa: E402
from catears_amd.shard import c4_corpus, num_frames, pack_batches  # noqa: E402


def pct(v, q):
    return round(float(np.percentile(v, q)), 1)


def main(passes=5, utts=240):
    mdir = os.path.join(tempfile.gettempdir(), f"catears_bench_{os.getuid()}")
    conf = synth.write_model(mdir, "tdnn-s")
    reusable = hasattr(gpu.Plan, "reusable")
    streams = [torch.cuda.Stream() for _ in range(4)]
    ctxs = [gpu.Context(0, s) for s in streams]
    model = gpu.Model(ctxs[0], conf)
    L, R, pdfs = model.left, model.right, model.num_pdfs
    samples = c4_corpus(utts)
    frames = [num_frames(int(n)) for n in samples]
    batches = pack_batches(frames, L, R, 4096)
    lengths = [[int(samples[u]) for u in b] for b in batches]
    rows = [sum(frames[u] for u in b) for b in batches]
    P, plen = 8, int(samples.max())
    pool = torch.from_numpy(np.stack([synth.pcm(600000 + i, plen) for i in range(P)]).astype(np.int16)).cuda()
    pcm, bstart, at = torch.empty(int(samples.sum()), dtype=torch.int16, device="cuda"), [], 0
    for b in batches:
        bstart.append(at)
        for u in b:
            n = int(samples[u])
            pcm[at:at + n].copy_(pool[u % P, :n])
            at += n
    gstats = torch.from_numpy(synth.cmvn_stats_synthetic()).cuda()
    maxf = max(rows)
    ws = [torch.empty((2 * maxf * 40 + 1,), dtype=torch.float32, device="cuda") for _ in ctxs]
    outs = [torch.empty((maxf, pdfs), dtype=torch.float32, device="cuda") for _ in batches]
    plans = [gpu.Plan.reusable(c, max(len(ls) for ls in lengths), max(sum(ls) for ls in lengths), model, 4096)
             for c in ctxs] if reusable else None
    res = {"version": gpu.lib().ce_gpu_version().decode(), "device": torch.cuda.get_device_name(0),
           "library": os.path.relpath(gpu.LIB_PATH), "reusable_plans": reusable, "passes": passes,
           "utterances": int(utts), "batches": len(batches), "frames": int(sum(rows)),
           "utterances_per_batch": round(utts / len(batches), 2), "legs": {}}

    def one_pass(leg, n_ctx, host):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, ls in enumerate(lengths):
            k = i % n_ctx
            view = pcm[bstart[i]:bstart[i] + sum(ls)]
            with torch.cuda.stream(streams[k]):
                h0 = time.perf_counter()
                if leg == "create":
                    plan = gpu.Plan(ctxs[k], ls, model, max_rows=4096)
                else:
                    plan = plans[k].assign(ls)
                h1 = time.perf_counter()
                gpu.score(ctxs[k], model, plan, view, gstats, ws=ws[k], out=outs[i])
                if leg == "create":
                    h2 = time.perf_counter()
                    plan.close()
                    h1 += time.perf_counter() - h2
                host.append((h1 - h0) * 1e6)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / len(lengths)

    legs = ["create", "assign", "assign", "create"] if reusable else ["create", "create"]
    for n_ctx in (1, 4):
        for run, leg in enumerate(legs):
            one_pass(leg, n_ctx, [])
            host, per = [], [one_pass(leg, n_ctx, host) for _ in range(passes)]
            digest = hashlib.sha1()
            for i, n in enumerate(rows):
                digest.update(outs[i][:n].cpu().numpy().tobytes())
            rec = {"us_per_batch_p50": pct(per, 50), "us_per_batch_p10": pct(per, 10), "us_per_batch_p90": pct(per, 90),
                   "host_describe_us_p50": pct(host, 50), "host_describe_us_p90": pct(host, 90),
                   "rows_sha1": digest.hexdigest()[:16]}
            res["legs"][f"{leg}/{n_ctx}ctx/run{run}"] = rec
            print(f"{leg:7s} {n_ctx} ctx run {run}: {rec['us_per_batch_p50']:8.1f} us/batch "
                  f"[{rec['us_per_batch_p10']:.1f}, {rec['us_per_batch_p90']:.1f}]  describe "
                  f"{rec['host_describe_us_p50']:7.1f} us  rows {rec['rows_sha1']}", file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:3]])
