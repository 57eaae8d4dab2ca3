"""What ce_gpu_model_admit_row_ops buys a model with row steps of its own,
on one MI355X: the TDNN-S shape with every BatchNorm replaced by Normalize
(the relu-renorm TDNN), one JSON object on stdout.
   python tools/row_ops.py [calls]
   python tools/row_ops.py --static-int8 [calls]     the same net in static int8, see static_int8()

Legs, on one context, in A B B A order per row count (4072 and 70):
  A  the model as loaded: fp32 mode, the only one it takes;
  B  the model admitted, three sub-legs: bf16x6, bf16x6 with the context's
     latency mode on, bf16.
Per leg the median / 10th / 90th percentile of the event-bracketed device
time of one ce_gpu_nnet_propagate, warm, and the mean of the calls back to
back.  Compare legs of one run only.

Accuracy: the max and p99.9 absolute log-likelihood difference of each B leg
against A on the same rows (fbank features of synthetic audio).

The row kernel alone, in the same run: ReLU + Normalize on 4072 x 1024 as one
rowop_chain launch against ce_gpu_rowwise's two launches (A B B A), and the
chain with the bf16 store."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from catears_amd import formats, gpu, synth  # noqa: E402

ROWS = (4072, 70)
B_LEGS = (("admitted bf16x6", "bf16x6", False), ("admitted bf16x6 + latency", "bf16x6", True),
          ("admitted bf16", "bf16", False))


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
    spec = synth.MODELS["tdnn-s"]
    hidden, pdfs = spec["hidden"], spec["pdfs"]
    layers, left, right, prior = synth.tdnn_layers(hidden, pdfs)
    layers = [{"kind": "normalize"} if L["kind"] == "batchnorm" else L for L in layers]
    image = formats.nnet_bytes(layers, left, right)
    ctx = gpu.Context(0)
    loaded = gpu.Model(ctx, image=image, prior=prior)
    assert loaded.gemm == "fp32", loaded.gemm
    admitted = gpu.Model(ctx, image=image, prior=prior).admit_row_ops(ctx)
    assert admitted.gemm == "bf16x6", admitted.gemm
    res = {"version": gpu.lib().ce_gpu_version().decode(), "device": torch.cuda.get_device_name(0), "calls": calls,
           "model": f"tdnn-s shape, hidden {hidden}, {pdfs} pdfs, every BatchNorm replaced by Normalize",
           "widths": admitted.padded_widths()[0].tolist(), "timing": {}, "accuracy": {}, "row_kernel": {}}

    def run_leg(name, rows, x, run):
        if name == "loaded fp32":
            model = loaded
            ctx.set_latency(False)
        else:
            _, gemm, lat = next(b for b in B_LEGS if b[0] == name)
            model = admitted.set_gemm(gemm)
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
            got = gpu.nnet_propagate(ctx, admitted.set_gemm(gemm), feats, subtract_prior=True).cpu().numpy()
            ctx.set_latency(False)
            assert got.shape == ref.shape == (rows - left - right, pdfs)
            e = np.abs(got.astype(np.float64) - ref)
            res["accuracy"][f"{name}/{rows}"] = {
                "max_abs": float(e.max()), "p99.9": float(np.quantile(e, 0.999)),
                "argmax_agreement": float((got.argmax(axis=1) == ref.argmax(axis=1)).mean())}
    row_kernel(ctx, res, calls)
    print(json.dumps(res))


def row_kernel(ctx, res, calls, rows=4072, dim=1024):
    """ReLU + Normalize on rows x dim: two ce_gpu_rowwise launches (A) against
    one rowop_chain launch (B), A B B A; then the chain storing bf16."""
    x0 = torch.from_numpy(np.random.default_rng(7).normal(0, 2, size=(rows, dim)).astype(np.float32)).cuda()
    x, out16 = x0.clone(), torch.empty((rows, dim), dtype=torch.int16, device="cuda")

    def two():
        gpu.rowwise(ctx, "relu", x)
        gpu.rowwise(ctx, "normalize", x)

    legs = {"rowwise x 2": two, "rowop_chain": lambda: gpu.rowop_chain(ctx, ("relu", "normalize"), x),
            "rowop_chain -> bf16": lambda: gpu.rowop_chain(ctx, ("relu", "normalize"), x, out16=out16)}
    a = x0.clone()
    gpu.rowwise(ctx, "relu", a)
    gpu.rowwise(ctx, "normalize", a)
    b = gpu.rowop_chain(ctx, ("relu", "normalize"), x0.clone())
    res["row_kernel"]["same_bits"] = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
    for run, name in enumerate(["rowwise x 2", "rowop_chain", "rowop_chain -> bf16", "rowop_chain -> bf16",
                                "rowop_chain", "rowwise x 2"]):
        x.copy_(x0)
        for _ in range(20):
            legs[name]()
        us = per_call_us(legs[name], calls)
        rec = {"p50_us": round(float(np.percentile(us, 50)), 1), "p10_us": round(float(np.percentile(us, 10)), 1),
               "p90_us": round(float(np.percentile(us, 90)), 1)}
        res["row_kernel"][f"{name}/{rows}x{dim}/run{run}"] = rec
        print(f"{name:24s} {rows} x {dim}: p50 {rec['p50_us']:7.1f} us [{rec['p10_us']:.1f}, {rec['p90_us']:.1f}]",
              file=sys.stderr, flush=True)


def static_int8(calls=100):
    """--static-int8: the same net calibrated and switched to static int8
    (ce_gpu_model_quantize_static), whose row steps write the next Linear's
    bytes.  One JSON object: per leg -- 70 rows, 70 rows with the context's
    latency mode on, 4072 rows -- the p50 / p10 / p90 of the event-bracketed
    device time of one ce_gpu_nnet_propagate and a checksum of its rows, and
    what the program enqueued per call (ce_gpu_debug_i8_static_launches, where
    the library has it).  One process times one library (CATEARS_HIP_LIB): run
    the baseline library and this one as processes in A B B A order.  With
    the experiments library CATEARS_I8_FUSED=0 is the unfused program (the
    chain in place, then the quantize pass).
    Then the row kernel alone, A B B A in this process: ReLU + Normalize on
    4072 x 1024 ending in the byte store, against the chain in place followed
    by a quantize-only launch of the same kernel (no entry runs the model's
    quantize pass on caller buffers), and that launch alone."""
    import hashlib
    spec = synth.MODELS["tdnn-s"]
    hidden, pdfs = spec["hidden"], spec["pdfs"]
    layers, left, right, prior = synth.tdnn_layers(hidden, pdfs)
    layers = [{"kind": "normalize"} if L["kind"] == "batchnorm" else L for L in layers]
    image = formats.nnet_bytes(layers, left, right)
    ctx = gpu.Context(0)
    model = gpu.Model(ctx, image=image, prior=prior)
    cal = [synth.pcm(2900 + i, 48000) for i in range(4)]
    plan = gpu.Plan(ctx, [len(w) for w in cal], model)
    ranges = model.calibrate(ctx, plan, gpu.fbank(ctx, plan, torch.from_numpy(np.concatenate(cal)).cuda()))
    model.quantize_static(ctx, ranges)
    counts = getattr(gpu, "debug_i8_static_launches", None)
    if counts is not None and not hasattr(gpu.lib(), "ce_gpu_debug_i8_static_launches"):
        counts = None
    res = {"version": gpu.lib().ce_gpu_version().decode(), "device": torch.cuda.get_device_name(0), "calls": calls,
           "library": os.path.relpath(gpu.LIB_PATH), "CATEARS_I8_FUSED": os.environ.get("CATEARS_I8_FUSED"),
           "model": f"tdnn-s shape, hidden {hidden}, {pdfs} pdfs, every BatchNorm replaced by Normalize, static int8",
           "timing": {}, "row_kernel": {}}
    for rows, lat in ((70, False), (70, True), (4072, False)):
        wave = synth.pcm(3950 + rows, 160 * (rows - 1) + 400)
        p = gpu.Plan(ctx, [len(wave)])
        x = gpu.fbank(ctx, p, torch.from_numpy(wave).cuda())
        assert x.shape[0] == rows
        ctx.set_latency(lat)
        rec = time_leg(ctx, model, x, calls)
        if counts is not None:
            before = counts()
            gpu.nnet_propagate(ctx, model, x)
            rec["quantize_passes, row_launches, row_launches_q"] = [a - b for a, b in zip(counts(), before)]
        out = gpu.nnet_propagate(ctx, model, x).cpu().numpy()
        ctx.set_latency(False)
        rec["rows_sha1"] = hashlib.sha1(out.tobytes()).hexdigest()[:16]
        rec["finite"] = bool(np.isfinite(out).all())
        name = f"static int8{' + latency' if lat else ''}/{rows}"
        res["timing"][name] = rec
        print(f"{name:28s}: p50 {rec['p50_us']:7.1f} us [{rec['p10_us']:.1f}, {rec['p90_us']:.1f}] "
              f"back to back {rec['back_to_back_us']:7.1f} us", file=sys.stderr, flush=True)
    if hasattr(gpu.lib(), "ce_gpu_debug_rowop_chain_q") and hasattr(gpu, "debug_rowop_chain_q"):
        row_kernel_q(ctx, res, calls)
    print(json.dumps(res))


def row_kernel_q(ctx, res, calls, rows=4072, dim=1024):
    x0 = torch.from_numpy(np.random.default_rng(7).normal(0, 2, size=(rows, dim)).astype(np.float32)).cuda()
    x = x0.clone()
    q = [torch.empty((rows, dim), dtype=torch.int8, device="cuda") for _ in range(2)]
    rs = [torch.empty((rows,), dtype=torch.int32, device="cuda") for _ in range(2)]
    zero = torch.empty((rows,), dtype=torch.int32, device="cuda")
    s, z = gpu.quant_params_from_range(-4.0, 4.0)
    ops = ("relu", "normalize")

    def fused():
        gpu.debug_rowop_chain_q(ctx, ops, x0, s, z, q[0], rs[0], zero)

    def quantize_only():
        gpu.debug_rowop_chain_q(ctx, (), x, s, z, q[1], rs[1], zero)

    def in_place():
        gpu.rowop_chain(ctx, ops, x)

    def two():
        in_place()
        quantize_only()

    fused()
    two()
    res["row_kernel"]["same_bits"] = bool(torch.equal(q[0], q[1]) and torch.equal(rs[0], rs[1]))
    legs = {"chain in place + quantize-only launch": two, "chain -> bytes": fused, "chain in place": in_place,
            "quantize-only launch": quantize_only}
    order = ["chain in place + quantize-only launch", "chain -> bytes", "chain -> bytes",
             "chain in place + quantize-only launch", "chain in place", "quantize-only launch"]
    for run, name in enumerate(order):
        x.copy_(x0)
        for _ in range(20):
            legs[name]()
        us = per_call_us(legs[name], calls)
        rec = {"p50_us": round(float(np.percentile(us, 50)), 1), "p10_us": round(float(np.percentile(us, 10)), 1),
               "p90_us": round(float(np.percentile(us, 90)), 1)}
        res["row_kernel"][f"{name}/{rows}x{dim}/run{run}"] = rec
        print(f"{name:40s} {rows} x {dim}: p50 {rec['p50_us']:7.1f} us [{rec['p10_us']:.1f}, {rec['p90_us']:.1f}]",
              file=sys.stderr, flush=True)


if __name__ == "__main__":
    nums = [int(v) for v in sys.argv[1:] if not v.startswith("--")][:1]
    if "--static-int8" in sys.argv[1:]:
        static_int8(*nums)
    else:
        main(*nums)
