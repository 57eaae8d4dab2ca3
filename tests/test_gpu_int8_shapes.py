"""The int8 nnet path off the TDNN shapes (tests/i8ref.py has the nets, the
reference and the restated dispatch; tests/test_i8ref.py proves the CPU side).

Everything ahead of a LogSoftmax is exact arithmetic, so every comparison is
bit for bit -- dynamic int8 against i8ref.chunk_reference, static int8
against test_int8_static.static_oracle -- on nets that reach what the TDNN
nets never do: all six PostModes in each epilogue, 8 asymmetric splice
segments gathered by the GEMM loader (also on a first layer behind a row
map), widths off a multiple of 4, column counts ragged over many tiles, and
blocks whose edge rows are large, so the parameters depend on which rows a
Linear's fold holds (in nnet_propagate, in a packed am_forward chunk and in
calibration).  Only where a LogSoftmax follows is the bar the project's 1e-4.
"""
import numpy as np
import pytest

import i8ref
import netgen
from test_gpu_gemm_shapes import first_diff
from test_gpu_parity import LOGLIK_TOL, bits, dev
from test_int8_static import central_half, fp32_ranges, static_oracle

pytestmark = pytest.mark.gpu

GEOMS = sorted(i8ref.I8_GEOMETRIES)
BLOCKS = [70, 33, 151]


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
def ctxs(torch, G):
    c = {"plain": G.Context(0), "latency": G.Context(0)}
    c["latency"].set_latency(True)
    return c


@pytest.fixture(scope="module")
def ranges_of(oracle):
    """geom -> (num_linear, 2) fp32 ranges of i8ref.calibration_input."""
    cache = {}

    def get(geom):
        if geom not in cache:
            cache[geom] = fp32_ranges(oracle, i8ref.net(geom), i8ref.calibration_input(geom))
        return cache[geom]
    return get


def dynamic(G, ctx, layers, prior=None):
    model = G.Model(ctx, image=netgen.image(layers), prior=prior)
    assert (model.left, model.right) == netgen.context(layers)
    return model.quantize(ctx)


def static(G, ctx, layers, ranges):
    return G.Model(ctx, image=netgen.image(layers)).quantize_static(ctx, ranges)


# ------------------------------------------------------- a. dynamic, blocks --

@pytest.mark.parametrize("geom", GEOMS)
def test_dynamic_block_bit_exact(torch, G, ctxs, oracle, geom):
    layers = i8ref.net(geom)
    model = dynamic(G, ctxs["plain"], layers)
    failures = []
    for rows in i8ref.ROWS:
        x, want = i8ref.reference(oracle, geom, rows)
        got = G.nnet_propagate(ctxs["plain"], model, dev(torch, x)).cpu().numpy()
        d = first_diff(got, want)
        if d:
            failures.append(f"{geom} rows={rows} {i8ref.paths(layers, rows, 'dynamic')}: {d}")
    assert not failures, "\n".join(failures)


# ----------------------------------------------------- b. dynamic, finalize --

@pytest.mark.parametrize("geom", i8ref.FINALIZE)
def test_dynamic_finalize(torch, G, ctxs, oracle, geom):
    """A final LogSoftmax and the prior subtraction behind the int8 body (n >
    4096: launch_finalize's strided loop, rows 16-byte aligned or not):
    within 1e-4 of float64 x - logsumexp(x) - log prior of the bit-exact
    body."""
    body = i8ref.net(geom)
    n = i8ref.I8_GEOMETRIES[geom][1][-1]
    prior = netgen.prior(n, 77)
    model = dynamic(G, ctxs["plain"], body + [{"kind": "log_softmax"}], prior=prior)
    errs = {}
    for rows in i8ref.ROWS:
        x, y = i8ref.reference(oracle, geom, rows)
        y = y.astype(np.float64)
        mx = y.max(axis=1, keepdims=True)
        want = y - (mx + np.log(np.exp(y - mx).sum(axis=1, keepdims=True))) - np.log(prior.astype(np.float64))
        got = G.nnet_propagate(ctxs["plain"], model, dev(torch, x), subtract_prior=True).cpu().numpy()
        assert got.shape == want.shape
        errs[rows] = float(np.abs(got - want).max())
    print(geom, errs)
    assert max(errs.values()) <= LOGLIK_TOL, errs


# ------------------------------------------------------------ c. held rows --

@pytest.mark.parametrize("geom", i8ref.HELD)
def test_held_rows_blocks(torch, G, ctxs, oracle, geom):
    """Blocks whose first or last few rows are 32 times the rest
    (i8ref.held_inputs: test_i8ref shows that folding every row, or
    exchanging the contexts, changes the parameters): one by one, and packed
    through nnet_propagate_blocks, where each block is quantized alone."""
    layers = i8ref.net(geom)
    ctx = ctxs["plain"]
    model = dynamic(G, ctx, layers)
    inputs = i8ref.held_inputs(geom)
    wants, failures = [], []
    for name, x in inputs:
        (want,), _, _ = i8ref.chunk_reference(oracle, layers, [x])
        wants.append(want)
        d = first_diff(G.nnet_propagate(ctx, model, dev(torch, x)).cpu().numpy(), want)
        if d:
            failures.append(f"{geom} {name}: {d}")
    packed = np.concatenate([x for _, x in inputs])
    got = G.nnet_propagate_blocks(ctx, model, dev(torch, packed), [len(x) for _, x in inputs]).cpu().numpy()
    d = first_diff(got, np.concatenate(wants))
    if d:
        failures.append(f"{geom} packed blocks: {d}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("geom", i8ref.CHUNK)
def test_held_rows_packed_chunk(torch, G, ctxs, oracle, geom):
    """One am_forward chunk of five utterances (1 and 3 frames among them,
    shorter than the context), first or last frames scaled: the row map
    replicates them into the context, row_edge marks the utterance ends, one
    set of parameters per Linear covers the chunk.  Against chunk_reference
    over all the padded blocks; the chunk-wide parameters show in that some
    utterance differs from itself scored alone."""
    layers = i8ref.net(geom)
    ctx = ctxs["plain"]
    n = i8ref.I8_GEOMETRIES[geom][1][-1]
    model = dynamic(G, ctx, layers, prior=np.ones(n, np.float32))   # log prior exactly 0
    plan = G.Plan(ctx, [i8ref.frames_to_samples(t) for t in i8ref.CHUNK_LENGTHS], model)
    assert plan.n_chunks == 1 and plan.total_frames == sum(i8ref.CHUNK_LENGTHS)
    failures = []
    for name, utts in i8ref.chunk_inputs(geom):
        blocks = [i8ref.padded(layers, u) for u in utts]
        wants, _, _ = i8ref.chunk_reference(oracle, layers, blocks)
        got = G.am_forward(ctx, model, plan, dev(torch, np.concatenate(utts))).cpu().numpy()
        d = first_diff(got, np.concatenate(wants))
        if d:
            failures.append(f"{geom} {name} {i8ref.paths(layers, 1, 'dynamic', row_map=True)}: {d}")
        off = plan.frame_offsets
        alone = [i8ref.chunk_reference(oracle, layers, [b])[0][0] for b in blocks]
        assert any(first_diff(got[off[u]:off[u + 1]], a) for u, a in enumerate(alone)), (geom, name)
    assert not failures, "\n".join(failures)


# --------------------------------------------------------------- d. static --

@pytest.mark.parametrize("geom", GEOMS)
def test_static_block_bit_exact(torch, G, ctxs, oracle, ranges_of, geom):
    """Plain and latency contexts against static_oracle, the latency rows of
    the plain ones' bits -- also at the last row count of the split-K pair
    and the first beyond it."""
    layers = i8ref.net(geom)
    ranges = ranges_of(geom)
    models = {k: static(G, c, layers, ranges) for k, c in ctxs.items()}
    failures = []
    for rows in i8ref.ROWS + i8ref.latency_rows(geom):
        x = i8ref.block_input(geom, rows)
        want = static_oracle(oracle, layers, x, ranges)
        got = {k: G.nnet_propagate(ctxs[k], m, dev(torch, x)).cpu().numpy() for k, m in models.items()}
        for k, d in (("plain", first_diff(got["plain"], want)), ("latency", first_diff(got["latency"], want)),
                     ("latency vs plain", first_diff(got["latency"], got["plain"]))):
            if d:
                form = "static" if k == "plain" else "static-latency"
                failures.append(f"{geom} {k} rows={rows} {i8ref.paths(layers, rows, form)}: {d}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("geom", GEOMS)
def test_static_clamps_both_ends(torch, G, ctxs, oracle, ranges_of, geom):
    """Ranges shrunk to their central half: every Linear's bytes hold 0, 255
    and interior values (on the reference's bytes), in the quantize pass and
    in the requantize epilogue / reduce alike."""
    layers = i8ref.net(geom)
    half = central_half(ranges_of(geom))
    x = i8ref.clamp_input(geom)
    taps = []
    want = static_oracle(oracle, layers, x, half, taps)
    assert len(taps) == len(half)
    for i, q in enumerate(taps):
        assert (q == 0).any() and (q == 255).any() and ((q > 0) & (q < 255)).any(), (geom, i)
    for k, c in ctxs.items():
        got = G.nnet_propagate(c, static(G, c, layers, half), dev(torch, x)).cpu().numpy()
        assert first_diff(got, want) is None, f"{geom} {k}: {first_diff(got, want)}"


@pytest.mark.parametrize("geom", GEOMS)
def test_static_blocks_equal_one_block(torch, G, ctxs, oracle, ranges_of, geom):
    """Rows do not depend on the block: windows of 70, 33 and 151 output rows
    through nnet_propagate_blocks carry the bits of the one block holding
    them all."""
    layers = i8ref.net(geom)
    c = sum(netgen.context(layers))
    x = i8ref.block_input(geom, sum(BLOCKS))
    starts = np.concatenate([[0], np.cumsum(BLOCKS)])
    packed = np.concatenate([x[s:s + n + c] for s, n in zip(starts, BLOCKS)])
    want = static_oracle(oracle, layers, x, ranges_of(geom))
    for k, cx in ctxs.items():
        model = static(G, cx, layers, ranges_of(geom))
        one = G.nnet_propagate(cx, model, dev(torch, x)).cpu().numpy()
        assert first_diff(one, want) is None, f"{geom} {k}: {first_diff(one, want)}"
        blocks = G.nnet_propagate_blocks(cx, model, dev(torch, packed), [n + c for n in BLOCKS]).cpu().numpy()
        assert first_diff(blocks, one) is None, f"{geom} {k} blocks: {first_diff(blocks, one)}"


def test_static_launches_follow_paths(torch, G, oracle, ranges_of):
    """i8ref.paths against the library's own counters: a quantize pass runs
    exactly where no requantize epilogue wrote the bytes, and the split-K pair
    exactly where the slice rule gives it the layer."""
    ctx = G.Context(0)
    ctx.set_latency(True)
    ctx.profile(True)
    for geom in ("A", "I1", "I4", "I5"):
        layers = i8ref.net(geom)
        model = static(G, ctx, layers, ranges_of(geom))
        for rows in (70,) + i8ref.latency_rows(geom):
            ps = i8ref.paths(layers, rows, "static-latency")
            ctx.profile_read(ctx.PROF_QUANT), ctx.profile_read(ctx.PROF_GEMM)
            before = G.debug_i8_latency_launches()
            G.nnet_propagate(ctx, model, dev(torch, i8ref.block_input(geom, rows)))
            torch.cuda.synchronize()
            assert ctx.profile_read(ctx.PROF_QUANT)[1] == sum(p["quantize"] != "none" for p in ps), (geom, rows)
            assert ctx.profile_read(ctx.PROF_GEMM)[1] == len(ps), (geom, rows)
            assert G.debug_i8_latency_launches() - before == sum(p["slices"][0] > 0 for p in ps), (geom, rows)
    ctx.profile(False)


# ---------------------------------------------------------- e. calibration --

@pytest.mark.parametrize("mode", ["fp32", "bf16x6"])
def test_calibrate_folds_the_held_rows(torch, G, ctxs, oracle, mode):
    """ce_gpu_model_calibrate on an exact-integer net (the fp32-class GEMMs
    are exact on it) over five edge-scaled utterances in one chunk, a 1-frame
    one among them: the exact per-Linear ranges over the rows the reference
    chain holds -- test_i8ref shows that any other row rule gives other
    ranges here."""
    layers, cases = i8ref.calib_case()
    ctx = ctxs["plain"]
    model = G.Model(ctx, image=netgen.image(layers)).set_gemm(mode)
    for name, utts in cases.items():
        blocks = [i8ref.padded(layers, u) for u in utts]
        for b in blocks:
            netgen.check_exact_budget(layers, b)
        want = i8ref.fp32_held_ranges(oracle, layers, blocks)
        plan = G.Plan(ctx, [i8ref.frames_to_samples(len(u)) for u in utts], model)
        assert plan.n_chunks == 1 and plan.total_frames == sum(len(u) for u in utts)
        got = model.calibrate(ctx, plan, dev(torch, np.concatenate(utts)))
        assert np.array_equal(bits(got), bits(want)), (mode, name, got, want)
