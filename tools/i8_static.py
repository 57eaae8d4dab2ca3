"""Dynamic against static int8 on the C5 block: TDNN-S, one 8192-row block
through ce_gpu_nnet_propagate, timed with HIP events in one process.

  A  dynamic        ce_gpu_model_quantize: per layer min/max fold + quantize
                    pass + GEMM (the parameters reduced over the block)
  B  static unfused ce_gpu_model_quantize_static, CATEARS_I8_FUSED=0: frozen
                    parameters, a quantize pass before every GEMM
  C  static fused   the same model, the hidden GEMMs' epilogues write the next
                    layer's bytes (the default)

Legs run in A B C C B A order, `iters` calls each after a warm-up; B and C
are one model, switched through the experiments library's per-call switch.
A second pass times the launch classes of each leg (ce_gpu_ctx_profile):
quantize passes (min/max fold included) and GEMMs, per launch.

  python tools/i8_static.py [iters] [rows]      -> JSON lines"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
EXP = os.path.join(ROOT, "catears_amd", "lib", "libcatears_hip_exp.so")
if not os.path.exists(EXP):
    sys.exit("libcatears_hip_exp.so missing: make EXPERIMENTS=1 lib")
os.environ.setdefault("CATEARS_HIP_LIB", EXP)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT)
from catears_amd import formats, gpu, synth  # noqa: E402


def main(iters=50, rows=8192):
    layers, left, right, _ = synth.tdnn_layers(1024, 3456, seed=7)
    image = formats.nnet_bytes(layers, left, right)
    ctx = gpu.Context(0)
    rng = np.random.default_rng(rows)
    x = torch.from_numpy(rng.normal(9.0, 3.0, size=(rows, 40)).astype(np.float32)).cuda()
    # calibrate on another block of the same distribution, as one utterance
    frames = 2000
    cal = torch.from_numpy(rng.normal(9.0, 3.0, size=(frames, 40)).astype(np.float32)).cuda()
    m_static = gpu.Model(ctx, image=image)
    plan = gpu.Plan(ctx, [400 + 160 * (frames - 1)], m_static)
    ranges = m_static.calibrate(ctx, plan, cal)
    m_static.quantize_static(ctx, ranges)
    m_dyn = gpu.Model(ctx, image=image).quantize(ctx)
    out = torch.empty((rows - left - right, m_dyn.num_pdfs), dtype=torch.float32, device="cuda")
    legs = {"A": ("dynamic", m_dyn, None), "B": ("static_unfused", m_static, "0"), "C": ("static_fused", m_static, "1")}

    def run(leg, n):
        _, model, fused = legs[leg]
        if fused is not None:
            os.environ["CATEARS_I8_FUSED"] = fused
        for _ in range(n):
            gpu.nnet_propagate(ctx, model, x, out=out)

    print(json.dumps({"device": torch.cuda.get_device_name(0), "model": "tdnn-s", "rows": rows, "iters": iters,
                      "order": "A B C C B A", "version": gpu.lib().ce_gpu_version().decode()}), flush=True)
    sums = {}
    for leg in "ABC":
        run(leg, 3)
        torch.cuda.synchronize()
        sums[leg] = float(out.double().sum().item())
    times = {k: [] for k in legs}
    for leg in "ABCCBA":
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        run(leg, 3)
        torch.cuda.synchronize()
        a.record()
        run(leg, iters)
        b.record()
        torch.cuda.synchronize()
        times[leg].append(a.elapsed_time(b) * 1e3 / iters)
    for leg, (name, _, _) in legs.items():
        t = times[leg]
        print(json.dumps({"leg": leg, "name": name, "us_per_block": [round(v, 1) for v in t],
                          "mean_us": round(sum(t) / len(t), 1), "frames_per_s": round(rows / (sum(t) / len(t)) * 1e6),
                          "checksum": sums[leg]}), flush=True)
    # launch classes per leg (event pairs around every launch: not the times above)
    for leg, (name, _, _) in legs.items():
        ctx.profile(True, classes=[gpu.Context.PROF_GEMM, gpu.Context.PROF_QUANT])
        run(leg, 10)
        q_ms, q_n = ctx.profile_read(gpu.Context.PROF_QUANT)
        g_ms, g_n = ctx.profile_read(gpu.Context.PROF_GEMM)
        ctx.profile(False)
        print(json.dumps({"leg": leg, "name": name, "per_block": {
            "quant_launch_groups": q_n // 10, "quant_us": round(q_ms * 100, 1),
            "gemm_launches": g_n // 10, "gemm_us": round(g_ms * 100, 1)}}), flush=True)
    d, u, f = (sum(times[k]) / len(times[k]) for k in "ABC")
    print(json.dumps({"static_fused_over_dynamic": round(f / d, 3), "static_unfused_over_dynamic": round(u / d, 3),
                      "fused_over_unfused": round(f / u, 3), "static_not_slower_than_dynamic": bool(f <= d)}),
          flush=True)


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:3]])
