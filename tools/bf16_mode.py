"""The plain bf16 GEMM mode (CE_GPU_GEMM_BF16) beside bf16x6 and static int8
on one MI355X: time and accuracy of TDNN-S nnet_propagate blocks, one JSON
object on stdout.   python tools/bf16_mode.py [calls]

Timing: a 4072-row block and a 70-row block, the three models in one process
in ABBA order (bf16x6, bf16, int8, int8, bf16, bf16x6), warm; per leg the
median / 10th / 90th percentile of the event-bracketed per-call device time
and the mean of the calls back to back; per layer the median GEMM launch time
from ce_gpu_ctx_profile (a separate, profiled pass: the events cost time).
Compare legs of one run only.

Accuracy: bf16 and static int8 against the fp32 mode on the same rows (max
abs, p99.9, argmax agreement), bf16x6 for scale; the rows are fbank features
of held-out synthetic audio, the kind the int8 ranges are calibrated on."""
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from catears_amd import gpu, synth  # noqa: E402

ROWS = (4072, 70)
LEGS = ("bf16x6", "bf16", "static_int8", "static_int8", "bf16", "bf16x6")


def per_call_us(fn, calls):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) * 1e3 for a, b in ev])


def layer_us(ctx, model, x, out, calls):
    """Median launch time per GEMM layer (first-layer gather / quantize passes
    are other classes and not included)."""
    ctx.profile(True, [ctx.PROF_GEMM])
    gpu.profile_anchor(0, torch.cuda.current_stream())
    for _ in range(calls):
        gpu.nnet_propagate(ctx, model, x, out=out)
    iv = ctx.profile_intervals(ctx.PROF_GEMM)
    ctx.profile(False)
    assert len(iv) == calls * model.num_linear, (len(iv), calls, model.num_linear)
    d = np.array([(b - a) * 1e3 for a, b in iv]).reshape(calls, model.num_linear)
    return [round(float(v), 1) for v in np.median(d, axis=0)]


def main(calls=100):
    mdir = os.path.join(tempfile.gettempdir(), f"catears_bench_{os.getuid()}")
    conf = synth.write_model(mdir, "tdnn-s")
    ctx = gpu.Context(0)
    cal = [synth.pcm(2900 + i, 48000) for i in range(4)]
    m0 = gpu.Model(ctx, conf)
    plan = gpu.Plan(ctx, [len(w) for w in cal], m0)
    ranges = m0.calibrate(ctx, plan, gpu.fbank(ctx, plan, torch.from_numpy(np.concatenate(cal)).cuda()))
    models = {"fp32": gpu.Model(ctx, conf).set_gemm("fp32"), "bf16x6": m0,
              "bf16": gpu.Model(ctx, conf).set_gemm("bf16"),
              "static_int8": gpu.Model(ctx, conf).quantize_static(ctx, ranges)}
    res = {"version": gpu.lib().ce_gpu_version().decode(), "device": torch.cuda.get_device_name(0), "calls": calls,
           "model": "tdnn-s", "timing": {}, "accuracy": {}}
    for rows in ROWS:
        # features-like input: the static int8 ranges were calibrated on fbank rows
        x = torch.from_numpy(np.random.default_rng(rows).normal(9, 3, size=(rows, 40)).astype(np.float32)).cuda()
        for i, leg in enumerate(LEGS):
            model = models[leg]
            out = gpu.nnet_propagate(ctx, model, x)
            for _ in range(20):
                gpu.nnet_propagate(ctx, model, x, out=out)
            us = per_call_us(lambda: gpu.nnet_propagate(ctx, model, x, out=out), calls)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                gpu.nnet_propagate(ctx, model, x, out=out)
            b.record()
            torch.cuda.synchronize()
            rec = {"p50_us": round(float(np.percentile(us, 50)), 1), "p10_us": round(float(np.percentile(us, 10)), 1),
                   "p90_us": round(float(np.percentile(us, 90)), 1),
                   "back_to_back_us": round(a.elapsed_time(b) * 1e3 / calls, 1),
                   "gemm_layer_us": layer_us(ctx, model, x, out, min(calls, 50))}
            res["timing"][f"{leg}/{rows}/run{i}"] = rec
            print(f"{leg:12s} rows {rows:5d}: p50 {rec['p50_us']:7.1f} us [{rec['p10_us']:.1f}, {rec['p90_us']:.1f}] "
                  f"back to back {rec['back_to_back_us']:7.1f} us  layers {rec['gemm_layer_us']}", file=sys.stderr, flush=True)
        # accuracy on fbank rows of held-out synthetic audio (what the int8
        # ranges were calibrated for), the same row count
        wave = synth.pcm(2950 + rows, 160 * (rows - 1) + 400)
        p1 = gpu.Plan(ctx, [len(wave)])
        feats = gpu.fbank(ctx, p1, torch.from_numpy(wave).cuda())
        assert feats.shape[0] == rows
        ref = gpu.nnet_propagate(ctx, models["fp32"], feats).cpu().numpy().astype(np.float64)
        for leg in ("bf16x6", "bf16", "static_int8"):
            got = gpu.nnet_propagate(ctx, models[leg], feats).cpu().numpy().astype(np.float64)
            e = np.abs(got - ref)
            res["accuracy"][f"{leg}/{rows}"] = {
                "max_abs": float(e.max()), "p99.9": float(np.quantile(e, 0.999)),
                "argmax_agreement": float((got.argmax(axis=1) == ref.argmax(axis=1)).mean())}
    print(json.dumps(res))


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:2]])
