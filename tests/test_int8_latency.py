"""Latency mode of static int8 (kernels/nnet_i8_lat.hip): on a context with
ce_gpu_ctx_set_latency, a static int8 Linear on a small row block runs as a
split-K pair (i8_lat_gemm_kernel + i8_lat_reduce_kernel) instead of the
throughput kernel.  The accumulators are integers modulo 2^32, so the bar is
bit for bit: against static_oracle (tests/test_int8_static.py), and against
the same model with the mode off.

CPU: the two new ABI entries and the slice rule (ce_gpu_i8_latency_plan).
GPU: bits, the dispatch (ce_gpu_debug_i8_latency_launches) and sessions.
"""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_int8_static import (FLT_MIN, NETS, _inputs, _static_model, _tdnn, bits, central_half, dev, fp32_ranges,
                              same, static_oracle)

KPADS = [128, 256, 384, 1152, 3072]
WIDTHS = [96, 97, 100, 1024, 3456]
ROWS = [1, 21, 70, 81, 640, 1024]


def crossover(G):
    """The largest row count the slice rule still gives the split-K pair
    (kI8LatMaxRows), found through the ABI."""
    r = 1
    while G.i8_latency_plan(1024, 1024, r + 1)[0] > 0:
        r += 1
        assert r < 1 << 16
    return r


# ------------------------------------------------------------------- CPU ----

def test_abi_lists_the_latency_entries():
    from catears_amd import gpu
    text = open(os.path.join(ROOT, "include", "catears_gpu.h")).read()
    for name in ("ce_gpu_i8_latency_plan", "ce_gpu_debug_i8_latency_launches"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in gpu.ABI and hasattr(gpu.lib(), name)
    assert gpu.debug_i8_latency_launches() >= 0
    with pytest.raises(gpu.CatearsError) as e:
        gpu.i8_latency_plan(0, 96, 70)
    assert e.value.code == -2


def test_plan_covers_k_exactly():
    """slices >= 1 implies (slices - 1) * per < kpad / 64 <= slices * per: no
    slice is empty and none is missing; rows above the crossover and an
    ineligible K give 0."""
    from catears_amd import gpu
    top = crossover(gpu)
    assert top >= 70
    taken = 0
    for kpad in KPADS:
        for n in WIDTHS:
            for rows in ROWS:
                slices, per = gpu.i8_latency_plan(kpad, n, rows)
                if rows > top:
                    assert slices == 0, (kpad, n, rows)
                    continue
                assert slices >= 1 and per >= 1, (kpad, n, rows)
                assert (slices - 1) * per < kpad // 64 <= slices * per, (kpad, n, rows, slices, per)
                taken += 1
    assert taken >= len(KPADS) * len(WIDTHS) * 3
    for rows in ROWS:
        assert gpu.i8_latency_plan(192, 1024, rows)[0] == 0
    assert gpu.i8_latency_plan(1024, 1024, top)[0] > 0 and gpu.i8_latency_plan(1024, 1024, top + 1)[0] == 0


def test_plan_fills_the_chip_on_tdnn_s():
    """TDNN-S's three big shapes at the 70-row streaming chunk: blocks per
    launch (slices x row tiles x 64-column tiles; one row tile at 70 rows)
    within a factor of two of one per CU on 256 CUs."""
    from catears_amd import gpu
    for kpad, n in ((3072, 1024), (1024, 1024), (1024, 3456)):
        slices, _ = gpu.i8_latency_plan(kpad, n, 70)
        blocks = slices * ((n + 63) // 64)
        assert 128 <= blocks <= 512, (kpad, n, slices, blocks)


# ------------------------------------------------------------------- GPU ----

on_gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def G():
    from catears_amd import gpu
    gpu.lib()
    return gpu


@pytest.fixture(scope="module")
def ctx(torch, G):
    """The throughput context (latency off)."""
    return G.Context(0)


@pytest.fixture(scope="module")
def lctx(torch, G):
    c = G.Context(0)
    c.set_latency(True)
    return c


@pytest.fixture(scope="module")
def nets(oracle):
    out = {}
    for hidden, pdfs in NETS:
        layers, left, right = _tdnn(hidden, pdfs)
        out[(hidden, pdfs)] = (layers, left, right, fp32_ranges(oracle, layers, _inputs(300, 4242)))
    return out


@pytest.fixture(scope="module")
def wants(oracle, nets):
    """(net, rows) -> static_oracle's rows, computed once."""
    cache = {}

    def get(net, rows):
        if (net, rows) not in cache:
            layers, _, _, ranges = nets[net]
            cache[(net, rows)] = static_oracle(oracle, layers, _inputs(rows, rows), ranges)
        return cache[(net, rows)]
    return get


def linear_shapes(layers):
    """(kpad, n) of every Linear: K padded to the int8 K-tile of 128."""
    return [((L["W"].shape[0] + 127) // 128 * 128, L["W"].shape[1]) for L in layers if L["kind"] == "linear"]


def planned(G, layers, rows):
    return sum(G.i8_latency_plan(kpad, n, rows)[0] > 0 for kpad, n in linear_shapes(layers))


CASES = [(net, rows) for net in NETS for rows in (21, 70, 81, 300)] + [((384, 100), 1100)]


@on_gpu
@pytest.mark.parametrize("net,rows", CASES)
def test_latency_block_bit_exact(torch, G, lctx, nets, wants, net, rows):
    layers, left, right, ranges = nets[net]
    model = _static_model(G, lctx, layers, left, right, ranges)
    before = G.debug_i8_latency_launches()
    got = G.nnet_propagate(lctx, model, dev(torch, _inputs(rows, rows))).cpu().numpy()
    assert G.debug_i8_latency_launches() - before == planned(G, layers, rows)
    want = wants(net, rows)
    assert got.shape == want.shape == (rows - left - right, net[1])
    diff = np.flatnonzero(bits(got) != bits(want))
    assert diff.size == 0, f"{diff.size} elements differ, first at {np.unravel_index(diff[0], got.shape)}"


@pytest.fixture(scope="module")
def xs_pair(torch, G, ctx, lctx, xs_config):
    """Calibrated static TDNN-XS (as test_int8_static's xs_static); the model
    serves both contexts (same device)."""
    from catears_amd import synth
    m = G.Model(ctx, xs_config)
    waves = [synth.pcm(60 + i, 16000 * 3) for i in range(3)]
    plan = G.Plan(ctx, [len(w) for w in waves], m)
    feats = G.fbank(ctx, plan, dev(torch, np.concatenate(waves)))
    ranges = m.calibrate(ctx, plan, feats)
    return m.quantize_static(ctx, ranges), ranges


@on_gpu
def test_latency_on_equals_off_on_tdnn_xs(torch, G, ctx, lctx, xs_pair):
    """score (LogSoftmax and prior included) of one 3 s utterance, and
    propagate_blocks of 70 / 33 / 151 rows against each block alone."""
    from catears_amd import synth
    model, _ = xs_pair
    wave = dev(torch, synth.pcm(81, 16000 * 3))
    off = G.score(ctx, model, G.Plan(ctx, [wave.shape[0]], model), wave).cpu().numpy()
    before = G.debug_i8_latency_launches()
    on = G.score(lctx, model, G.Plan(lctx, [wave.shape[0]], model), wave).cpu().numpy()
    assert np.isfinite(off).all() and same(on, off)
    rng = np.random.default_rng(77)
    sizes = [70, 33, 151]
    blocks = [rng.normal(9.0 + 4 * i, 1.0 + 2 * i, size=(n, 40)).astype(np.float32) for i, n in enumerate(sizes)]
    got = G.nnet_propagate_blocks(lctx, model, dev(torch, np.concatenate(blocks)), sizes).cpu().numpy()
    assert same(got, G.nnet_propagate_blocks(ctx, model, dev(torch, np.concatenate(blocks)), sizes).cpu().numpy())
    at = 0
    for b in blocks:
        alone = G.nnet_propagate(lctx, model, dev(torch, b)).cpu().numpy()
        assert same(alone, G.nnet_propagate(ctx, model, dev(torch, b)).cpu().numpy())
        assert same(got[at:at + len(alone)], alone)
        at += len(alone)
    assert at == len(got)
    assert G.debug_i8_latency_launches() > before


@on_gpu
def test_latency_clamps_both_ends(torch, G, lctx, oracle, nets):
    layers, left, right, ranges = nets[(384, 100)]
    half = central_half(ranges)
    x = _inputs(70, 300)
    taps = []
    want = static_oracle(oracle, layers, x, half, taps)
    assert len(taps) == len(half)
    for i, q in enumerate(taps):
        assert (q == 0).any() and (q == 255).any() and ((q > 0) & (q < 255)).any(), i
    model = _static_model(G, lctx, layers, left, right, half)
    before = G.debug_i8_latency_launches()
    got = G.nnet_propagate(lctx, model, dev(torch, x)).cpu().numpy()
    assert G.debug_i8_latency_launches() - before == planned(G, layers, 70)
    assert same(got, want)


@on_gpu
def test_latency_dead_layer_range(torch, G, lctx, oracle):
    """test_static_edge_ranges' dead_layer recipe at hidden 128: the next
    Linear's range is [0, FLT_MIN], its scale a denormal, and every quotient
    of the reduce's requantize the division fallback's."""
    layers, left, right = _tdnn(128, 96)
    lin = [i for i, L in enumerate(layers) if L["kind"] == "linear"]
    i = lin[1]
    layers[i] = dict(layers[i], W=np.zeros_like(layers[i]["W"]), b=np.full_like(layers[i]["b"], -1.0))
    bn = next(j for j in range(i, len(layers)) if layers[j]["kind"] == "batchnorm")
    layers[bn] = dict(layers[bn], offset=np.zeros_like(layers[bn]["offset"]))
    ranges = fp32_ranges(oracle, layers, _inputs(300, 4242))
    assert tuple(ranges[2]) == (np.float32(0.0), FLT_MIN)
    model = _static_model(G, lctx, layers, left, right, ranges)
    x = _inputs(70, 5)
    before = G.debug_i8_latency_launches()
    got = G.nnet_propagate(lctx, model, dev(torch, x)).cpu().numpy()
    assert G.debug_i8_latency_launches() - before == planned(G, layers, 70)
    assert same(got, static_oracle(oracle, layers, x, ranges))


@on_gpu
def test_latency_mixed_chain(torch, G, lctx, oracle, nets, wants):
    """A row op between two GEMMs forces an fp32 output and a quantize pass in
    the middle of a fused net (test_static_row_ops_between_gemms' net); the
    hidden-64 net has no fused layer at all.  Both at 70 rows."""
    layers, left, right, _ = nets[(128, 96)]
    bn = [i for i, L in enumerate(layers) if L["kind"] == "batchnorm"][2]
    layers = layers[:bn + 1] + [dict(layers[bn]), {"kind": "relu"}] + layers[bn + 1:]
    ranges = fp32_ranges(oracle, layers, _inputs(300, 4242))
    model = _static_model(G, lctx, layers, left, right, ranges)
    x = _inputs(70, 6)
    assert same(G.nnet_propagate(lctx, model, dev(torch, x)).cpu().numpy(), static_oracle(oracle, layers, x, ranges))
    layers, left, right, ranges = nets[(64, 96)]
    model = _static_model(G, lctx, layers, left, right, ranges)
    assert same(G.nnet_propagate(lctx, model, dev(torch, _inputs(70, 70))).cpu().numpy(), wants((64, 96), 70))


@on_gpu
def test_latency_dispatch(torch, G, ctx, lctx, nets, xs_config):
    from catears_amd import formats
    layers, left, right, ranges = nets[(384, 100)]
    image = formats.nnet_bytes(layers, left, right)
    x70 = dev(torch, _inputs(70, 70))
    n_lin = len(linear_shapes(layers))
    assert 0 < planned(G, layers, 70) <= n_lin
    # latency on, static model, 70 rows: one split-K GEMM per planned Linear
    static = G.Model(lctx, image=image).quantize_static(lctx, ranges)
    c0 = G.debug_i8_latency_launches()
    on = G.nnet_propagate(lctx, static, x70).cpu().numpy()
    c1 = G.debug_i8_latency_launches()
    assert c1 - c0 == planned(G, layers, 70)
    # latency off: none
    off = G.nnet_propagate(ctx, static, x70).cpu().numpy()
    assert G.debug_i8_latency_launches() == c1 and same(on, off)
    # dynamic int8 ignores the mode
    dyn = G.Model(lctx, image=image).quantize(lctx)
    assert np.isfinite(G.nnet_propagate(lctx, dyn, x70).cpu().numpy()).all()
    assert G.debug_i8_latency_launches() == c1
    # just above the crossover: the throughput kernel, the same bits on the
    # rows both blocks hold (a row depends on its own input rows only)
    top = crossover(G)
    x = _inputs(top + 1, 9)
    above = G.nnet_propagate(lctx, static, dev(torch, x)).cpu().numpy()
    assert G.debug_i8_latency_launches() == c1
    below = G.nnet_propagate(lctx, static, dev(torch, x[:top])).cpu().numpy()
    assert G.debug_i8_latency_launches() - c1 == planned(G, layers, top) > 0
    # every output row of the shorter block reads input rows both blocks hold
    assert len(below) == len(above) - 1 > 0 and same(above[:len(below)], below)


@on_gpu
def test_latency_sessions(torch, G, lctx, xs_pair, global_stats):
    """Static TDNN-XS on a latency context: 3 slots, pushes of 1600 / 777 /
    160 samples until EOS; rows bit-identical to the one-shot score, no push
    after the first allocates or frees, and the pushes take the split-K pair."""
    from catears_amd import synth
    model, _ = xs_pair
    gs = dev(torch, global_stats)
    waves = [synth.pcm(940 + k, n) for k, n in enumerate([8000, 6000 + 77, 4000])]
    steps = [1600, 777, 160]
    sess = G.Sessions(lctx, model, 3, 1600, gs)
    rows = [[] for _ in waves]
    pos = [0, 0, 0]
    try:
        c0 = G.debug_i8_latency_launches()
        counters = None
        while any(p < len(w) for p, w in zip(pos, waves)):
            slots, counts, eos, pieces = [], [], [], []
            for k, w in enumerate(waves):
                if pos[k] >= len(w):
                    continue
                c = min(steps[k], len(w) - pos[k])
                slots.append(k), counts.append(c), eos.append(pos[k] + c == len(w))
                pieces.append(w[pos[k]:pos[k] + c])
                pos[k] += c
            out, n = sess.push(slots, dev(torch, np.concatenate(pieces)), counts, eos=eos)
            out = out.cpu().numpy()
            at = 0
            for k, r in zip(slots, n):
                rows[k].append(out[at:at + r])
                at += r
            if counters is None:
                counters = G.debug_counters()  # after the first push
        assert G.debug_counters() == counters
        assert G.debug_i8_latency_launches() > c0
    finally:
        sess.close()
    for k, w in enumerate(waves):
        ref = G.score(lctx, model, G.Plan(lctx, [len(w)], model), dev(torch, w), gs).cpu().numpy()
        assert same(np.concatenate(rows[k]), ref), k
