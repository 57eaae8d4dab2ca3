"""What ce_gpu_model_pad_widths buys a model outside the matrix-core
envelope, on one MI355X: a TDNN-S-shaped synthetic model with hidden width
650 and 3449 pdfs (the widths a converted Kaldi model typically has), one JSON
object on stdout.   python tools/pad_widths.py [calls]

Legs, on one context, in A B B A order per row count (4072 and 70):
  A  the model as loaded: fp32 mode, the only one it takes;
  B  the model padded (650 -> 672, 3449 -> 3452), three sub-legs: bf16x6,
     bf16x6 with the context's latency mode on, bf16.
Per leg the median / 10th / 90th percentile of the event-bracketed device
time of one ce_gpu_nnet_propagate, warm, and the mean of the calls back to
back.  Compare legs of one run only.

Accuracy: the max and p99.9 absolute log-likelihood difference of each B leg
against A on the same rows (fbank features of synthetic audio)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from catears_amd import formats, gpu, synth  # noqa: E402

HIDDEN, PDFS = 650, 3449
ROWS = (4072, 70)
B_LEGS = (("padded bf16x6", "bf16x6", False), ("padded bf16x6 + latency", "bf16x6", True),
          ("padded bf16", "bf16", False))


def per_call_us(fn, calls):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) * 1e3 for a, b in ev])


def time_leg(ctx, model, x, calls):
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
    return {"p50_us": round(float(np.percentile(us, 50)), 1), "p10_us": round(float(np.percentile(us, 10)), 1),
            "p90_us": round(float(np.percentile(us, 90)), 1),
            "back_to_back_us": round(a.elapsed_time(b) * 1e3 / calls, 1)}


def main(calls=100):
    layers, left, right, prior = synth.tdnn_layers(HIDDEN, PDFS)
    image = formats.nnet_bytes(layers, left, right)
    ctx = gpu.Context(0)
    loaded = gpu.Model(ctx, image=image, prior=prior)
    assert loaded.gemm == "fp32", loaded.gemm
    padded = gpu.Model(ctx, image=image, prior=prior).pad_widths(ctx)
    true_w, pad_w = padded.padded_widths()
    res = {"version": gpu.lib().ce_gpu_version().decode(), "device": torch.cuda.get_device_name(0), "calls": calls,
           "model": f"tdnn-s shape, hidden {HIDDEN}, {PDFS} pdfs", "widths": true_w.tolist(),
           "padded_widths": pad_w.tolist(), "timing": {}, "accuracy": {}}

    def run_leg(name, rows, x, run):
        if name == "loaded fp32":
            model = loaded
            ctx.set_latency(False)
        else:
            _, gemm, lat = next(b for b in B_LEGS if b[0] == name)
            model = padded.set_gemm(gemm)
            ctx.set_latency(lat)
        rec = time_leg(ctx, model, x, calls)
        ctx.set_latency(False)
        res["timing"][f"{name}/{rows}/run{run}"] = rec
        print(f"{name:24s} rows {rows:5d}: p50 {rec['p50_us']:7.1f} us [{rec['p10_us']:.1f}, {rec['p90_us']:.1f}] "
              f"back to back {rec['back_to_back_us']:7.1f} us", file=sys.stderr, flush=True)

    for rows in ROWS:
        x = torch.from_numpy(np.random.default_rng(rows).normal(9, 3, size=(rows, 40)).astype(np.float32)).cuda()
        b_names = [b[0] for b in B_LEGS]
        for run, name in enumerate(["loaded fp32"] + b_names + b_names[::-1] + ["loaded fp32"]):
            run_leg(name, rows, x, run)
        wave = synth.pcm(3950 + rows, 160 * (rows - 1) + 400)
        plan = gpu.Plan(ctx, [len(wave)])
        feats = gpu.fbank(ctx, plan, torch.from_numpy(wave).cuda())
        assert feats.shape[0] == rows
        ref = gpu.nnet_propagate(ctx, loaded, feats, subtract_prior=True).cpu().numpy().astype(np.float64)
        for name, gemm, lat in B_LEGS:
            ctx.set_latency(lat)
            got = gpu.nnet_propagate(ctx, padded.set_gemm(gemm), feats, subtract_prior=True).cpu().numpy()
            ctx.set_latency(False)
            assert got.shape == ref.shape == (rows - left - right, PDFS)
            e = np.abs(got.astype(np.float64) - ref)
            res["accuracy"][f"{name}/{rows}"] = {
                "max_abs": float(e.max()), "p99.9": float(np.quantile(e, 0.999)),
                "argmax_agreement": float((got.argmax(axis=1) == ref.argmax(axis=1)).mean())}
    print(json.dumps(res))


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:2]])
