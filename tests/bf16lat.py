"""Latency mode of the plain bf16 GEMM (kernels/gemm_bf16_lat.hip), restated
for tests/test_bf16_latency.py (CPU) and tests/test_gpu_bf16_latency.py.

The dispatch rule (launch_gemm_bf16): on a latency context a Linear of a bf16
model runs on gemm_bf16_lat_kernel when its block has at most kB16LatMaxRows
rows -- a function of the row count only; every Linear of a chunk sees the
same row count (output rows + left + right), so a call makes either one
latency launch per Linear or none.

The accumulator model: the mode sums K in tiles of 32, each tile's 32 exact
products added to one running fp32 value in ascending order.  A kernel that
split K, or walked it in another order, would round differently;
accumulate() restates both so the CPU test can show how often that is
visible on the operands the GPU test uses.
"""
import os
import re

import numpy as np

import bf16ref
import netgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source(name):
    return open(os.path.join(ROOT, "catears_amd", "csrc", name)).read()


def max_rows_in_source():
    """kB16LatMaxRows as internal.h states it."""
    (v,) = re.findall(r"constexpr int kB16LatMaxRows = (\d+);", source("internal.h"))
    return int(v)


MAX_ROWS = max_rows_in_source()


def kernel(latency, m):
    """The kernel family of one bf16 Linear on a block of m rows."""
    return "b16_lat" if latency and m <= MAX_ROWS else "b16"


def latency_launches(layers, out_rows, latency=True):
    """gemm_bf16_lat_kernel launches of one call that returns out_rows rows."""
    left, right = netgen.context(layers)
    return sum(kernel(latency, out_rows + left + right) == "b16_lat" for _ in netgen.linears(layers))


def accumulate(a16, w16, halves=False):
    """(rows x K) @ (K x n) of bf16-valued float32 operands, K a multiple of
    32 (of 64 with halves): per K-tile the exact sum of its 32 products
    (float64 holds it: 16-bit significands, 32 terms) added to the running
    float32 value and rounded, tiles ascending.  halves: the same over each
    half of the K-tiles on its own, the two partials added at the end -- a
    two-slice split-K."""
    a, w = np.asarray(a16, np.float64), np.asarray(w16, np.float64)
    kt = a.shape[1] // 32
    assert a.shape[1] == kt * 32 == w.shape[0]

    def run(t0, t1):
        acc = np.zeros((a.shape[0], w.shape[1]), np.float32)
        for t in range(t0, t1):
            tile = a[:, 32 * t:32 * t + 32] @ w[32 * t:32 * t + 32]
            acc = (acc.astype(np.float64) + tile).astype(np.float32)
        return acc

    if not halves:
        return run(0, kt)
    return (run(0, kt // 2).astype(np.float64) + run(kt // 2, kt).astype(np.float64)).astype(np.float32)


def order_cases():
    """{K: (a16, w16)}: 70 rows of bf16-rounded N(0, 1) activations against 96
    columns of bf16-rounded N(0, 0.1) weights, at the K of the real-valued GPU
    cases' Linears (geometry A: 200 padded to 224, 288, 800; ONE_LINEAR: 3072)
    and one small K."""
    out = {}
    for k in (64, 224, 288, 800, 3072):
        rng = np.random.default_rng(9000 + k)
        a = bf16ref.rne_bf16(rng.normal(0.0, 1.0, size=(70, k)).astype(np.float32))
        w = bf16ref.rne_bf16(rng.normal(0.0, 0.1, size=(k, 96)).astype(np.float32))
        out[k] = (a, w)
    return out


def exact_input(layers, name, rows, seed):
    """Integer input rows for an exact case of netgen.one_plane_mode_cases,
    under the amplitude its recipe is exact at (netgen.exact_cases); the
    binade-shifted forms scale it as netgen.binade_shift does."""
    recipe, _, shift = name.partition("*2^")
    x = netgen.int_input(layers, rows, seed, amax=1023 if recipe == "two-planes" else 7)
    return np.ldexp(x, int(shift)).astype(np.float32) if shift else x
