"""Per-call latency of ce_gpu_nnet_propagate on TDNN-S (one stream, calls back
to back, HIP events), default (throughput) mode vs latency mode
(ce_gpu_ctx_set_latency): the streaming AcousticModel chunk (chunk_size 50 +
20 context rows), a 250-frame chunk, one 10 s utterance (1018 rows) and the
bench's 4072-row batch.   python tools/latency.py [calls]
(LAT_MODES=latency LAT_ROWS=70 restrict the modes and row counts)

  python tools/latency.py --static-int8 [calls]
      the static int8 leg (ce_gpu_model_quantize_static, calibrated on 12 s of
      the synthetic audio): the 70-row chunk per call (LAT_ROWS for a sweep)
      with latency mode off and on, beside the bf16x6 latency mode, see
      static_int8()

  python tools/latency.py --fbank-stream [calls]
      the drop-in Fbank::Process per 512-sample piece, alone and beside 4
      concurrent AM lanes, see fbank_stream()"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from catears_amd import gpu, synth  # noqa: E402


def main(calls=200):
    mdir = os.path.join(tempfile.gettempdir(), f"catears_bench_{os.getuid()}")
    conf = synth.write_model(mdir, "tdnn-s")
    res = {}
    modes = os.environ.get("LAT_MODES", "throughput,latency").split(",")
    sizes = [int(v) for v in os.environ.get("LAT_ROWS", "70,270,1018,4072").split(",")]
    for mode in modes:
        ctx = gpu.Context(0)
        ctx.set_latency(mode == "latency")
        model = gpu.Model(ctx, conf)
        for rows in sizes:
            x = torch.from_numpy(np.random.default_rng(rows).normal(0, 3, size=(rows, 40)).astype(np.float32)).cuda()
            out = gpu.nnet_propagate(ctx, model, x)
            for _ in range(20):
                gpu.nnet_propagate(ctx, model, x, out=out)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                gpu.nnet_propagate(ctx, model, x, out=out)
            b.record()
            torch.cuda.synchronize()
            us = a.elapsed_time(b) * 1e3 / calls
            frames = rows - model.left - model.right
            digest = hashlib.sha1(out.cpu().numpy().tobytes()).hexdigest()[:12]
            res[f"{mode}/{rows}"] = {"us_per_call": round(us, 1), "frames_per_s": round(frames / us * 1e6),
                                     "sha1": digest}
            print(f"{mode:10s} rows {rows:5d}: {us:8.1f} us/call  {frames / us * 1e6 / 1e6:7.3f} M frames/s"
                  f"  out {digest}", flush=True)
    if os.environ.get("LAT_GRAPH"):
        # the same calls captured once in a HIP graph (fixed input / output
        # buffers) and replayed: the launch cost of a serving loop that stages
        # each chunk into the captured input
        for mode in modes:
            s = torch.cuda.Stream()
            ctx = gpu.Context(0, s)
            ctx.set_latency(mode == "latency")
            model = gpu.Model(ctx, conf)
            for rows in sizes:
                x = torch.from_numpy(np.random.default_rng(rows).normal(0, 3, size=(rows, 40))
                                     .astype(np.float32)).cuda()
                with torch.cuda.stream(s):
                    out = gpu.nnet_propagate(ctx, model, x)
                    for _ in range(3):
                        gpu.nnet_propagate(ctx, model, x, out=out)
                s.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    gpu.nnet_propagate(ctx, model, x, out=out)
                for _ in range(20):
                    g.replay()
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(calls):
                    g.replay()
                b.record()
                torch.cuda.synchronize()
                us = a.elapsed_time(b) * 1e3 / calls
                frames = rows - model.left - model.right
                digest = hashlib.sha1(out.cpu().numpy().tobytes()).hexdigest()[:12]
                res[f"graph-{mode}/{rows}"] = {"us_per_call": round(us, 1), "frames_per_s": round(frames / us * 1e6),
                                               "sha1": digest}
                print(f"graph {mode:10s} rows {rows:5d}: {us:8.1f} us/call  {frames / us * 1e6 / 1e6:7.3f} M frames/s"
                      f"  out {digest}", flush=True)
    print(json.dumps(res))


def per_call_us(fn, calls):
    """Event-bracketed device time of each of `calls` back-to-back calls."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) * 1e3 for a, b in ev])


def static_int8(calls=200):
    """TDNN-S as static int8, one nnet_propagate per call: latency mode off
    (the throughput int8 kernel) and on (the split-K pair up to the crossover
    of ce_gpu_i8_latency_plan), and the bf16x6 latency mode of the fp32 model
    in the same run.  Per leg and row count: the median and the 10th / 90th
    percentile of the per-call device times, the mean of the calls back to
    back, and the output digest (off and on must agree).  The legs alternate
    off / on / bf16x6 / on / off, so each int8 leg is measured twice."""
    mdir = os.path.join(tempfile.gettempdir(), f"catears_bench_{os.getuid()}")
    conf = synth.write_model(mdir, "tdnn-s")
    sizes = [int(v) for v in os.environ.get("LAT_ROWS", "70").split(",")]
    ctxs = {"off": gpu.Context(0), "on": gpu.Context(0), "bf16x6": gpu.Context(0)}
    ctxs["on"].set_latency(True)
    ctxs["bf16x6"].set_latency(True)
    cal = [synth.pcm(2900 + i, 48000) for i in range(4)]
    m0 = gpu.Model(ctxs["off"], conf)
    plan = gpu.Plan(ctxs["off"], [len(w) for w in cal], m0)
    ranges = m0.calibrate(ctxs["off"], plan, gpu.fbank(ctxs["off"], plan, torch.from_numpy(np.concatenate(cal)).cuda()))
    models = {"off": m0.quantize_static(ctxs["off"], ranges),
              "on": gpu.Model(ctxs["on"], conf).quantize_static(ctxs["on"], ranges),
              "bf16x6": gpu.Model(ctxs["bf16x6"], conf)}
    # absent from libraries older than the int8 latency mode (A/B runs)
    launches = getattr(gpu, "debug_i8_latency_launches", lambda: 0)
    res = {"version": gpu.lib().ce_gpu_version().decode(), "device": torch.cuda.get_device_name(0), "calls": calls}
    for rows in sizes:
        x = torch.from_numpy(np.random.default_rng(rows).normal(9, 3, size=(rows, 40)).astype(np.float32)).cuda()
        for i, leg in enumerate(["off", "on", "bf16x6", "on", "off"]):
            ctx, model = ctxs[leg], models[leg]
            out = gpu.nnet_propagate(ctx, model, x)
            for _ in range(20):
                gpu.nnet_propagate(ctx, model, x, out=out)
            n0 = launches()
            us = per_call_us(lambda: gpu.nnet_propagate(ctx, model, x, out=out), calls)
            n1 = launches()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                gpu.nnet_propagate(ctx, model, x, out=out)
            b.record()
            torch.cuda.synchronize()
            digest = hashlib.sha1(out.cpu().numpy().tobytes()).hexdigest()[:12]
            name = "bf16x6_latency" if leg == "bf16x6" else f"static_int8_latency_{leg}"
            rec = {"p50_us": round(float(np.percentile(us, 50)), 1), "p10_us": round(float(np.percentile(us, 10)), 1),
                   "p90_us": round(float(np.percentile(us, 90)), 1),
                   "back_to_back_us": round(a.elapsed_time(b) * 1e3 / calls, 1), "sha1": digest,
                   "i8_latency_gemms_per_call": (n1 - n0) / calls}
            res[f"{name}/{rows}/run{i}"] = rec
            print(f"{name:24s} rows {rows:5d}: p50 {rec['p50_us']:7.1f} us  [{rec['p10_us']:.1f}, {rec['p90_us']:.1f}]"
                  f"  back to back {rec['back_to_back_us']:7.1f} us  split-K GEMMs/call {rec['i8_latency_gemms_per_call']:.0f}"
                  f"  out {digest}", flush=True)
    print(json.dumps(res))


def layer_us(ctx, model, x, out, calls=50):
    """Median launch interval (us) of each GEMM of one nnet_propagate call
    (ce_gpu_ctx_profile, class GEMM: the Linears behind the first one's
    splice_pad launch and the first one itself, in program order)."""
    ctx.profile(True, classes=[0])  # CE_GPU_PROF_GEMM
    gpu.profile_anchor(0, torch.cuda.current_stream(0))
    for _ in range(calls):
        gpu.nnet_propagate(ctx, model, x, out=out)
    iv = np.array(ctx.profile_intervals(0))
    ctx.profile(False)
    per = (iv[:, 1] - iv[:, 0]).reshape(calls, -1) * 1e3
    return [round(float(v), 1) for v in np.median(per, axis=0)]


def bf16(calls=300):
    """TDNN-S in plain bf16 mode, one nnet_propagate per call: latency mode off
    (gemm_bf16_kernel on 32 x 32 tiles) and on (gemm_bf16_lat_kernel up to
    ce_gpu_bf16_latency_max_rows rows), beside the bf16x6 latency mode of the
    fp32 model and the static int8 latency mode in the same run.  Per leg and
    row count (LAT_ROWS, default 70) as static_int8(); the bf16 legs also give
    their per-layer GEMM launch intervals, and off and on must agree in their
    digests.  The legs alternate off / on / bf16x6 / int8 / on / off, so each
    bf16 leg is measured twice.  LAT_LEGS restricts the legs."""
    mdir = os.path.join(tempfile.gettempdir(), f"catears_bench_{os.getuid()}")
    conf = synth.write_model(mdir, "tdnn-s")
    sizes = [int(v) for v in os.environ.get("LAT_ROWS", "70").split(",")]
    legs = os.environ.get("LAT_LEGS", "off,on,bf16x6,int8,on,off").split(",")
    ctxs = {k: gpu.Context(0) for k in ("off", "on", "bf16x6", "int8")}
    for k in ("on", "bf16x6", "int8"):
        ctxs[k].set_latency(True)
    models = {"off": gpu.Model(ctxs["off"], conf).set_gemm("bf16"), "on": gpu.Model(ctxs["on"], conf).set_gemm("bf16"),
              "bf16x6": gpu.Model(ctxs["bf16x6"], conf)}
    if "int8" in legs:
        cal = [synth.pcm(2900 + i, 48000) for i in range(4)]
        m0 = gpu.Model(ctxs["int8"], conf)
        plan = gpu.Plan(ctxs["int8"], [len(w) for w in cal], m0)
        ranges = m0.calibrate(ctxs["int8"], plan,
                              gpu.fbank(ctxs["int8"], plan, torch.from_numpy(np.concatenate(cal)).cuda()))
        models["int8"] = m0.quantize_static(ctxs["int8"], ranges)
    # absent from libraries older than the bf16 latency mode (A/B runs)
    launches = getattr(gpu, "debug_bf16_latency_launches", lambda: 0)
    max_rows = getattr(gpu, "bf16_latency_max_rows", lambda: 0)()
    res = {"version": gpu.lib().ce_gpu_version().decode(), "device": torch.cuda.get_device_name(0), "calls": calls,
           "bf16_latency_max_rows": max_rows}
    names = {"off": "bf16_latency_off", "on": "bf16_latency_on", "bf16x6": "bf16x6_latency",
             "int8": "static_int8_latency_on"}
    for rows in sizes:
        x = torch.from_numpy(np.random.default_rng(rows).normal(9, 3, size=(rows, 40)).astype(np.float32)).cuda()
        for i, leg in enumerate(legs):
            ctx, model = ctxs[leg], models[leg]
            out = gpu.nnet_propagate(ctx, model, x)
            for _ in range(20):
                gpu.nnet_propagate(ctx, model, x, out=out)
            n0 = launches()
            us = per_call_us(lambda: gpu.nnet_propagate(ctx, model, x, out=out), calls)
            n1 = launches()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                gpu.nnet_propagate(ctx, model, x, out=out)
            b.record()
            torch.cuda.synchronize()
            digest = hashlib.sha1(out.cpu().numpy().tobytes()).hexdigest()[:12]
            rec = {"p50_us": round(float(np.percentile(us, 50)), 1), "p10_us": round(float(np.percentile(us, 10)), 1),
                   "p90_us": round(float(np.percentile(us, 90)), 1),
                   "back_to_back_us": round(a.elapsed_time(b) * 1e3 / calls, 1), "sha1": digest,
                   "bf16_latency_gemms_per_call": (n1 - n0) / calls}
            if leg in ("off", "on"):
                rec["gemm_layer_us"] = layer_us(ctx, model, x, out)
            res[f"{names[leg]}/{rows}/run{i}"] = rec
            print(f"{names[leg]:24s} rows {rows:5d}: p50 {rec['p50_us']:7.1f} us  [{rec['p10_us']:.1f}, {rec['p90_us']:.1f}]"
                  f"  back to back {rec['back_to_back_us']:7.1f} us  latency GEMMs/call "
                  f"{rec['bf16_latency_gemms_per_call']:.0f}  out {digest}  {rec.get('gemm_layer_us', '')}", flush=True)
    print(json.dumps(res))


def fbank_stream(calls=400):
    """The drop-in Fbank::Process on a live stream: the host time of one call
    on a 512-sample piece (32 ms of audio, the reference's ce_stt_process
    read), through the native driver tests/native/pk_fbank_stream.cc (`make
    host` builds catears_amd/lib/pk_fbank_stream).  Legs, one driver process
    each, alone / beside / beside / alone: the fbank stream by itself, and
    beside 4 threads that each stream frames through AcousticModel::Process
    (TDNN-S, the config's chunk size) on lanes of their own (CATEARS_LANES=8,
    so the fbank call never waits for a lane).  Per leg the median and the
    10th / 90th percentile of the per-call wall time, the AM batches scored
    meanwhile and what the library allocated and released during the timed
    calls (ce_gpu_debug_counters).  One run times one drop-in library: the
    directory of the driver and its libraries is CATEARS_PK_DIR (default:
    this tree's catears_amd/lib); run this library and the parent's in
    A B B A order."""
    import subprocess
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    pk_dir = os.path.abspath(os.environ.get("CATEARS_PK_DIR") or os.path.join(root, "catears_amd", "lib"))
    driver = os.path.join(pk_dir, "pk_fbank_stream")
    mdir = os.path.join(tempfile.gettempdir(), f"catears_bench_{os.getuid()}")
    conf = synth.write_model(mdir, "tdnn-s")
    pcm_path = os.path.join(mdir, "fbank_stream.f32")
    synth.pcm(7, 512 * (calls + 1)).tofile(pcm_path)
    env = {**os.environ, "CATEARS_LANES": "8", "LD_LIBRARY_PATH": pk_dir + ":" + os.environ.get("LD_LIBRARY_PATH", "")}
    res = {"driver": os.path.relpath(driver), "piece_samples": 512, "calls": calls}
    for run, am_threads in enumerate((0, 4, 4, 0)):
        r = subprocess.run([driver, "time", pcm_path, "512", str(calls + 1), conf, str(am_threads)],
                           capture_output=True, text=True, env=env, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"{driver} failed ({r.returncode}): {r.stderr[-2000:]}")
        rec = json.loads(r.stdout.strip().splitlines()[-1])
        name = "alone" if am_threads == 0 else f"beside_{am_threads}_am_lanes"
        res[f"fbank_process_512/{name}/run{run}"] = rec
        print(f"Fbank::Process 512 samples {name:18s}: p50 {rec['p50_us']:7.1f} us  [{rec['p10_us']:.1f}, "
              f"{rec['p90_us']:.1f}]  AM batches meanwhile {rec['am_batches_meanwhile']}  allocations "
              f"{rec['device_allocs']} releases {rec['device_frees']}", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    nums = [int(v) for v in sys.argv[1:] if not v.startswith("--")]
    if "--fbank-stream" in sys.argv[1:]:
        fbank_stream(*nums[:1])
    elif "--bf16" in sys.argv[1:]:
        bf16(*nums[:1])
    elif "--static-int8" in sys.argv[1:]:
        static_int8(*nums[:1])
    else:
        main(*nums[:1])
