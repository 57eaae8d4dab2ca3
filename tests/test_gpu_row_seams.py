"""The nnet kernels at the row counts on their tile and dispatch seams
(tests/rowseams.py derives the counts; tests/test_rowseams.py proves on the
CPU that they sit on every edge and that the earlier counts did not).

Every comparison is bit for bit.  Each input is uploaded once at its largest
count and every smaller count scores a prefix of that device tensor; the
results are compared on the device and read back only to describe a failure.

1. exact-integer nets against netgen.exact at every count of seam_rows, in
   every mode (plain bf16 against bf16ref.walk, f16x3 on its own recipes);
2. static int8 against the static oracle's prefix, dynamic int8 against the
   oracle per count;
3. the row kernels on an admitted net and on a renorm net in static int8,
   with 1, 2, 3 and 4 rows in their last block next to the row-tile seams;
4. finalize: the bits at a count are the prefix of the largest block's;
5. packed blocks whose boundaries fall on row-tile boundaries;
6. plans whose max_rows sit on the seams;
7. call order: a larger call leaves nothing behind for a smaller one."""
import functools

import numpy as np
import pytest

import bf16ref
import i8ref
import netgen
import rownet
import rowseams
from test_gpu_gemm_shapes import MODES, first_diff, load
from test_int8_static import fp32_ranges, static_oracle

pytestmark = pytest.mark.gpu

ALL_MODES = dict(MODES, bf16=("plain", "bf16"), f16x3=("plain", "f16x3"))


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
    c = {"plain": G.Context(0), "wide": G.Context(0), "latency": G.Context(0)}
    c["wide"].set_wide_tiles(True)
    c["latency"].set_latency(True)
    return c


def load_any(G, ctxs, layers, mode, prior=None):
    """load() of test_gpu_gemm_shapes, and the two modes it does not know."""
    if mode in MODES:
        return load(G, ctxs, layers, mode, prior)
    ctx = ctxs["plain"]
    model = G.Model(ctx, image=netgen.image(layers), prior=prior)
    assert netgen.x6_ok(layers) and model.gemm == "bf16x6"
    model.set_gemm(mode)
    assert model.gemm == mode
    return ctx, model


def dev(torch, x):
    """One upload (a copy: the cached inputs and references are read-only)."""
    return torch.from_numpy(np.array(x, np.float32)).cuda()


def same(torch, got, want):
    """Bit equality of two device tensors."""
    return got.shape == want.shape and bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))


def diff(got, want):
    """first_diff of two device tensors."""
    return first_diff(got.cpu().numpy(), want.cpu().numpy())


def sweep(torch, G, ctx, model, xd, wantd, c, counts, what, **kw):
    """nnet_propagate at every m of counts on the prefix xd[:m]; the result
    must carry the bits of wantd[:m - c].  Returns the failures."""
    failures = []
    for m in counts:
        got = G.nnet_propagate(ctx, model, xd[:m], **kw)
        if not same(torch, got, wantd[:m - c]):
            failures.append(f"{what(m)}: {diff(got, wantd[:m - c])}")
    return failures


# ---------------------------------------------------- 1. exact-integer nets --

@functools.lru_cache(maxsize=None)
def exact_want(geom, recipe, bf16):
    layers, x = rowseams.exact_case(geom, recipe)
    form = "f16x3" if (geom, recipe) in rowseams.F16_CASES else "bf16x6"
    netgen.check_exact_budget(layers, x, form)
    want = bf16ref.walk(layers, x, np.float64).astype(np.float32) if bf16 else netgen.exact(layers, x)
    want.setflags(write=False)
    return want


EXACT_RUNS = [(g, r, mode) for g, r in rowseams.exact_ids() for mode in rowseams.case_modes(g, r)]


@pytest.mark.parametrize("geom,recipe,mode", EXACT_RUNS)
def test_exact_nets_at_every_seam_count(torch, G, ctxs, geom, recipe, mode):
    """A: gathered first layer; D: splice-pad first layer, the 512 x 128
    kernel from 2945 rows; H: whole-K-tile first layer.  Every count of
    seam_rows(layers, mode), no sample."""
    layers, x = rowseams.exact_case(geom, recipe)
    ctx, model = load_any(G, ctxs, layers, mode)
    c = model.left + model.right
    counts = rowseams.seam_rows(layers, mode)
    assert counts and counts[-1] <= len(x)
    if mode == "f16x3":
        assert not ctx.overflow()
    failures = sweep(torch, G, ctx, model, dev(torch, x), dev(torch, exact_want(geom, recipe, mode == "bf16")), c,
                     counts, lambda m: f"{geom} {recipe} {mode} m={m} {rowseams.dispatch(layers, m, mode)}")
    assert not failures, "\n".join(failures[:20])
    if mode == "f16x3":
        assert not ctx.overflow()


def test_fp32_pipe2_on_misaligned_rows(torch, G, ctxs):
    """H's first layer has whole K-tiles: on caller rows whose base is 4 bytes
    off a float4 the fp32 program leaves the LDS-DMA kernel (128-row tiles)
    for pipe2 on 64-row tiles.  The 128-row counts hold every residue of the
    64-row tile too."""
    from test_gpu_caller_buffers import placed
    layers, x = rowseams.exact_case("H", "wide")
    ctx, model = load(G, ctxs, layers, "fp32")
    c = model.left + model.right
    counts = rowseams.seam_rows(layers, "fp32")
    assert set(m for m in rowseams.tile_counts("f32_pipe2") if m > c) <= set(counts)
    assert netgen.kernels(layers, counts[0] - c, "fp32", caller_aligned=False)[0] == "f32_pipe2"
    xin = placed(torch, x, x.shape[1], 1, "nan")
    failures = sweep(torch, G, ctx, model, xin, dev(torch, exact_want("H", "wide", False)), c, counts,
                     lambda m: f"H wide fp32 lead=1 m={m} {netgen.kernels(layers, m - c, 'fp32', False)}")
    assert not failures, "\n".join(failures[:20])


# ------------------------------------------------------------------ 2. int8 --

@functools.lru_cache(maxsize=None)
def i8_block(geom):
    """The int8 nets' block at the largest count of both static sweeps."""
    layers = i8ref.net(geom)
    m = max(rowseams.seam_rows(layers, "int8") + rowseams.seam_rows(layers, "int8-latency"))
    x = netgen.real_input(layers, m - sum(netgen.context(layers)), 7700 + i8ref.seed_of(geom))
    x.setflags(write=False)
    return layers, x


@pytest.fixture(scope="module")
def i8_static_case(oracle):
    cache = {}

    def get(geom):
        if geom not in cache:
            layers, x = i8_block(geom)
            ranges = fp32_ranges(oracle, layers, i8ref.calibration_input(geom))
            want = static_oracle(oracle, layers, x, ranges)
            want.setflags(write=False)
            cache[geom] = (layers, x, ranges, want)
        return cache[geom]
    return get


@pytest.mark.parametrize("flavour", ["plain", "latency"])
@pytest.mark.parametrize("geom", rowseams.I8_GEOMS)
def test_static_int8_at_every_seam_count(torch, G, ctxs, i8_static_case, geom, flavour):
    """Static rows do not depend on the batch: one reference at the largest
    count, prefixes of it at every other.  Latency: the split-K kernel's
    96-row tile below 281 rows, the throughput kernel's 256-row tile above."""
    layers, x, ranges, want = i8_static_case(geom)
    ctx = ctxs[flavour]
    model = G.Model(ctx, image=netgen.image(layers)).quantize_static(ctx, ranges)
    mode = "int8" if flavour == "plain" else "int8-latency"
    failures = sweep(torch, G, ctx, model, dev(torch, x), dev(torch, want), model.left + model.right,
                     rowseams.seam_rows(layers, mode),
                     lambda m: f"{geom} {mode} m={m} {rowseams.dispatch(layers, m, mode)}")
    assert not failures, "\n".join(failures[:20])


@pytest.mark.parametrize("geom", rowseams.I8_GEOMS)
def test_dynamic_int8_at_its_tile_seams(torch, G, ctxs, oracle, geom):
    """Dynamic int8 quantizes per call: the oracle at each count."""
    layers, x = i8_block(geom)
    ctx = ctxs["plain"]
    model = G.Model(ctx, image=netgen.image(layers)).quantize(ctx)
    xd = dev(torch, x)
    failures = []
    for m in rowseams.seam_rows(layers, "int8-dynamic"):
        (want,), _, _ = i8ref.chunk_reference(oracle, layers, [x[:m]])
        d = first_diff(G.nnet_propagate(ctx, model, xd[:m]).cpu().numpy(), want)
        if d:
            failures.append(f"{geom} dynamic m={m}: {d}")
    assert not failures, "\n".join(failures)


# ----------------------------------------------------------- 3. row kernels --

ROW_CASE = "second-bn"    # a BatchNorm and a ReLU as row steps behind the first Linear


@functools.lru_cache(maxsize=None)
def row_case(bf16):
    layers, _ = rownet.exact_cases()[ROW_CASE]
    x = netgen.int_input(layers, rowseams.row_kernel_rows()[-1] - sum(netgen.context(layers)), 7800)
    want = rownet.walk(layers, x, rnd=bf16ref.rne_bf16) if bf16 else rownet.check_exact(layers, x)
    return layers, x, np.ascontiguousarray(want, np.float32)


@pytest.mark.parametrize("mode", ["bf16x6", "latency", "bf16"])
def test_row_steps_with_one_to_four_rows_in_the_last_block(torch, G, ctxs, mode):
    """rowop_kernel takes 4 rows per block: 126 .. 129 and 254 .. 257 rows
    leave 2, 3, 4 and 1 in the last one, next to the GEMMs' row-tile seams."""
    layers, x, want = row_case(mode == "bf16")
    flavour, gemm = ALL_MODES[mode]
    ctx = ctxs[flavour]
    model = G.Model(ctx, image=netgen.image(layers))
    assert model.gemm == "fp32" and model.admit_row_ops(ctx) is model and model.gemm == "bf16x6"
    model.set_gemm(gemm)
    counts = rowseams.row_kernel_rows()
    assert sorted({m % rowseams.ROW_KERNEL_ROWS for m in counts}) == [0, 1, 2, 3]
    failures = sweep(torch, G, ctx, model, dev(torch, x), dev(torch, want), model.left + model.right, counts,
                     lambda m: f"{ROW_CASE} {mode} m={m}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("flavour", ["plain", "latency"])
def test_byte_writing_row_chain_at_the_int8_row_tiles(torch, G, ctxs, oracle, flavour):
    """The renorm net in static int8 (hidden width 128: every boundary takes
    rowop_chain_kernel<int8_t>, which writes the next layer's bytes and row
    sums) at 254 .. 257 and 510 .. 513 rows."""
    import i8rowref
    from test_gpu_i8_row_chain import PDFS, calibrated, renorm
    layers, _ = renorm(128)
    body = i8rowref.without_final_log_softmax(layers)
    c = sum(netgen.context(body))
    counts = rowseams.row_kernel_rows(rowseams.FAMILIES["i8_256x128"][0])
    x = np.random.default_rng(7900).normal(0.0, 1.0, size=(counts[-1], 40)).astype(np.float32)
    ranges = calibrated(torch, G, ctxs["plain"], 128)
    want = i8rowref.static_rows(oracle, body, x, ranges)
    assert want.shape == (counts[-1] - c, PDFS)
    ctx = ctxs[flavour]
    model = G.Model(ctx, image=netgen.image(body)).quantize_static(ctx, ranges)
    failures = sweep(torch, G, ctx, model, dev(torch, x), dev(torch, want), c, counts,
                     lambda m: f"renorm-128 {flavour} m={m}")
    assert not failures, "\n".join(failures)


# -------------------------------------------------------------- 4. finalize --

@functools.lru_cache(maxsize=None)
def finalize_case(geom):
    layers = rowseams.finalize_net(geom)
    m = max(max(rowseams.seam_rows(layers, mode)) for mode in MODES)
    return layers, netgen.real_input(layers, m - sum(netgen.context(layers)), 7500)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("geom", rowseams.FINALIZE_GEOMS)
def test_finalize_rows_are_the_large_block_s(torch, G, ctxs, geom, mode):
    """LogSoftmax and the prior behind real-valued nets (G20: finalize_vec;
    F4100: the loop finalize): an invariance test -- the bits at every seam
    count are the prefix of the largest block's (which is right:
    test_real_nets_vs_fp64).  Latency at 1024 / 1025: the fused lat_finalize
    hands over to lat_reduce and the finalize kernels."""
    layers, x = finalize_case(geom)
    n = netgen.linears(layers)[-1]["n"]
    assert netgen.finalize_path(n) == ("vector" if geom == "G20" else "loop")
    ctx, model = load(G, ctxs, layers, mode, prior=netgen.prior(n, 77))
    xd = dev(torch, x)
    big = G.nnet_propagate(ctx, model, xd, subtract_prior=True)
    assert bool(torch.isfinite(big).all())
    counts = rowseams.seam_rows(layers, mode)
    if mode == "latency":
        assert {1024, 1025} <= set(counts)
    failures = sweep(torch, G, ctx, model, xd, big, model.left + model.right, counts,
                     lambda m: f"{geom} {mode} m={m} {rowseams.dispatch(layers, m, mode)}", subtract_prior=True)
    assert not failures, "\n".join(failures[:20])


# --------------------------------------------------------- 5. packed blocks --

def seam_blocks(c):
    """Input rows per block: the packed boundaries fall on 64, 128 and 256
    (row-tile boundaries), then one row before and one behind such a one."""
    return [64, 64, 128, 1 + c, 127, 129]


@pytest.mark.parametrize("mode", list(MODES) + ["bf16"])
def test_packed_blocks_on_tile_boundaries(torch, G, ctxs, mode):
    """nnet_propagate_blocks clamps every spliced row to its block: here a
    block edge is a tile edge, or one row off it.  Geometry A, exact."""
    layers, x = rowseams.exact_case("A", "wide")
    want = exact_want("A", "wide", mode == "bf16")
    ctx, model = load_any(G, ctxs, layers, mode)
    c = model.left + model.right
    blocks = seam_blocks(c)
    assert np.cumsum(blocks)[:3].tolist() == [64, 128, 256]
    starts = np.concatenate([[0], np.cumsum([b - c for b in blocks])])
    packed = np.concatenate([x[s:s + b] for s, b in zip(starts, blocks)])
    got = G.nnet_propagate_blocks(ctx, model, dev(torch, packed), blocks).cpu().numpy()
    assert got.shape[0] == starts[-1]
    for i, b in enumerate(blocks):
        d = first_diff(got[starts[i]:starts[i + 1]], want[starts[i]:starts[i + 1]])
        assert d is None, f"A {mode} block {i} of {blocks} (rows {b}): {d}"


# ------------------------------------------------------------------ 6. plans --

PLAN_FRAMES = (700, 129, 1300)
PLAN_MAX_ROWS = (128, 129, 256, 1024, 1025)


@pytest.mark.parametrize("mode", ["fp32", "bf16x6", "int8"])
def test_plans_with_max_rows_on_the_seams(torch, G, ctxs, oracle, mode):
    """am_forward on three ragged utterances: chunks of at most 128, 129,
    256, 1024 and 1025 rows give the rows of one 4096-row chunk (static int8:
    its rows do not depend on the batch)."""
    layers = i8ref.net("A")
    ctx = ctxs["plain"]
    n = netgen.linears(layers)[-1]["n"]
    model = G.Model(ctx, image=netgen.image(layers), prior=np.ones(n, np.float32))
    if mode == "int8":
        model = model.quantize_static(ctx, fp32_ranges(oracle, layers, i8ref.calibration_input("A")))
    else:
        model.set_gemm(mode)
    feats = dev(torch, np.random.default_rng(7600).normal(0.0, 3.0, size=(sum(PLAN_FRAMES), 40)).astype(np.float32))
    samples = [i8ref.frames_to_samples(t) for t in PLAN_FRAMES]
    one = G.Plan(ctx, samples, model, max_rows=4096)
    assert one.n_chunks == 1 and one.total_frames == sum(PLAN_FRAMES)
    want = G.am_forward(ctx, model, one, feats)
    for max_rows in PLAN_MAX_ROWS:
        assert max_rows > model.left + model.right       # legal: room for a row beside the context
        plan = G.Plan(ctx, samples, model, max_rows=max_rows)
        assert plan.n_chunks > 1 and plan.total_frames == sum(PLAN_FRAMES)
        got = G.am_forward(ctx, model, plan, feats)
        assert same(torch, got, want), f"{mode} max_rows={max_rows}: {diff(got, want)}"


# ------------------------------------------------------------ 7. call order --

@pytest.mark.parametrize("mode", list(MODES) + ["bf16", "int8", "int8-latency"])
def test_call_order_leaves_nothing_behind(torch, G, ctxs, i8_static_case, mode):
    """The workspace layout, the int8 row sums and zero words and the latency
    partials are sized from the row count: the counts ascending, descending,
    and (static int8, latency, bf16x6) the largest, the smallest and the
    largest again give the bits of the first pass."""
    if mode.startswith("int8"):
        layers, x, ranges, _ = i8_static_case("I1")
        ctx = ctxs["latency" if mode == "int8-latency" else "plain"]
        model = G.Model(ctx, image=netgen.image(layers)).quantize_static(ctx, ranges)
    else:
        layers, x = rowseams.exact_case("A", "wide")
        ctx, model = load_any(G, ctxs, layers, mode)
    xd = dev(torch, x)
    counts = rowseams.seam_rows(layers, mode)
    first = {m: G.nnet_propagate(ctx, model, xd[:m]).clone() for m in counts}
    order = counts[::-1] + counts
    if mode in ("int8", "int8-latency", "latency", "bf16x6"):
        order += [counts[-1], counts[0], counts[-1], counts[0]]
    for i, m in enumerate(order):
        got = G.nnet_propagate(ctx, model, xd[:m])
        assert same(torch, got, first[m]), \
            f"{mode} m={m} after m={order[i - 1] if i else counts[-1]}: {diff(got, first[m])}"
