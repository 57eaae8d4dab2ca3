"""Latency mode of the plain bf16 GEMM, on the CPU: the two ABI entries, the
crossover constant, and the evidence that the GPU test's real-valued cases
would show a reordered or split K sum (tests/bf16lat.py).  The GPU side is
tests/test_gpu_bf16_latency.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import bf16lat
import bf16ref
import netgen
from conftest import ROOT

ENTRIES = ("ce_gpu_bf16_latency_max_rows", "ce_gpu_debug_bf16_latency_launches")


def test_entries_are_declared_and_bound():
    from catears_amd import gpu
    header = open(os.path.join(ROOT, "include", "catears_gpu.h")).read()
    assert re.search(r"int ce_gpu_bf16_latency_max_rows\(int \*max_rows\);", header)
    assert re.search(r"int ce_gpu_debug_bf16_latency_launches\(int64_t \*gemms\);", header)
    for name in ENTRIES:
        assert name in gpu.ABI and hasattr(gpu.lib(), name), name
        assert getattr(gpu.lib(), name).argtypes is not None
    assert gpu.debug_bf16_latency_launches() >= 0
    # host only: NULL is refused, and nothing here touched a device
    assert gpu.lib().ce_gpu_bf16_latency_max_rows(None) == -2
    assert b"NULL" in gpu.lib().ce_gpu_last_error()
    assert gpu.lib().ce_gpu_debug_bf16_latency_launches(None) == 0


def test_crossover_is_the_constant_in_the_source_and_covers_the_streaming_chunk():
    """The TDNN-S streaming chunk (chunk_size 50 + 20 context rows) is what
    the mode is for: a crossover below 70 rows would leave it on the
    throughput kernel."""
    from catears_amd import gpu
    assert gpu.bf16_latency_max_rows() == bf16lat.MAX_ROWS >= 70
    # the product library compiles the constant in; only the experiments
    # library reads the override
    lat = bf16lat.source("kernels/gemm_bf16_lat.hip")
    assert 'CE_KNOB("CATEARS_B16_LAT_MAXROWS", kB16LatMaxRows)' in lat
    data = open(os.path.join(ROOT, "catears_amd", "lib", "libcatears_hip.so"), "rb").read()
    assert b"CATEARS_B16_LAT" not in data and b"gemm_bf16_lat_kernel" in data


def test_the_rule_reads_the_row_count_only():
    R = bf16lat.MAX_ROWS
    assert [bf16lat.kernel(True, m) for m in (1, 70, R, R + 1)] == ["b16_lat"] * 3 + ["b16"]
    assert {bf16lat.kernel(False, m) for m in (1, 70, R, R + 1)} == {"b16"}
    in_d, widths, splices, post = netgen.GEOMETRIES["A"]
    layers = netgen.real_net(in_d, widths, splices, post, 1)
    c = sum(netgen.context(layers))
    assert bf16lat.latency_launches(layers, R - c) == 3 and bf16lat.latency_launches(layers, R - c + 1) == 0
    assert bf16lat.latency_launches(layers, 70, latency=False) == 0
    # what the rule rests on, in the sources: the launcher's test and the
    # program's flag
    assert "if (a.lat && a.m <= b16_lat_max_rows()) return launch_gemm_bf16_lat(s, a);" in \
        bf16lat.source("kernels/gemm_bf16.hip")
    assert "a.lat = ctx->latency != 0;" in bf16lat.source("nnet_programs.cc")


def test_both_kernels_share_one_epilogue():
    """The epilogue and the argument fill exist once, in the shared header."""
    for name in ("kernels/gemm_bf16.hip", "kernels/gemm_bf16_lat.hip"):
        src = bf16lat.source(name)
        assert '#include "../gemm_bf16_kernels.h"' in src and "b16_epilogue<" in src, name
        assert "void b16_epilogue(" not in src and "struct B16Args" not in src, name
    assert bf16lat.source("gemm_bf16_kernels.h").count("void b16_epilogue(") == 1


@pytest.mark.parametrize("k", sorted(bf16lat.order_cases()))
def test_real_valued_operands_show_a_split_sum(k):
    """Ascending tiles into one accumulator against two half-K partials added
    at the end: the two differ in at least one output in four for every K from
    224 up, so equal bits on the GPU rule out a split or reordered sum.
    (Mutation: accumulate(halves=True) against itself differs nowhere, and the
    ascending sum equals the fp64 product only to rounding.)"""
    a, w = bf16lat.order_cases()[k]
    one = bf16lat.accumulate(a, w)
    two = bf16lat.accumulate(a, w, halves=True)
    frac = float((one.view(np.uint32) != two.view(np.uint32)).mean())
    print(f"K = {k}: {frac:.3f} of the outputs differ between one accumulator and two half-K partials")
    assert np.array_equal(two, bf16lat.accumulate(a, w, halves=True))
    exact = a.astype(np.float64) @ w.astype(np.float64)
    assert np.abs(one - exact).max() <= 2.0 ** -20 * np.abs(exact).max() * (k // 32)
    if k >= 224:
        assert frac >= 0.25, (k, frac)
    else:
        assert frac > 0.0


@pytest.mark.parametrize("geom", ["A", "B", "C", "D", "F4100", "G9", "G20", "G25"])
def test_exact_inputs_stay_inside_the_exact_budget(geom):
    """The GPU test scores the exact-integer nets on inputs of its own (up to
    kB16LatMaxRows + 1 rows): every partial sum of every order is an integer
    below 2^24, so the fp64 walk is a zero-tolerance oracle there too."""
    for name, layers, _ in netgen.one_plane_mode_cases(geom):
        c = sum(netgen.context(layers))
        x = bf16lat.exact_input(layers, name, bf16lat.MAX_ROWS + 1 - c, 9100)
        assert x.shape[0] == bf16lat.MAX_ROWS + 1
        bounds = bf16ref.exact_bounds(layers, x)
        assert max(bounds) < 24.0, (geom, name, bounds)
