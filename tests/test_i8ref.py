"""The CPU side of tests/test_gpu_int8_shapes.py: that tests/i8ref.py's
chunk_reference is the oracle's int8 propagate, that the geometries reach
every class of the int8 dispatch (i8ref.paths), that no float64 GEMM of the
reference can differ from the int32 ring, and that the held-row tests' inputs
can see a wrong held-row rule -- so a mismatch on the GPU is the kernel's, and
a kernel that ignored the rule could not pass."""
import numpy as np
import pytest

import i8ref
import netgen
from test_int8_static import bits, fold_range

GEOMS = sorted(i8ref.I8_GEOMETRIES)
AGREE_ROWS = (1, 70, 129)


def _all_paths(form, row_map=False):
    for g in GEOMS:
        for rows in i8ref.ROWS + (i8ref.latency_rows(g) if form == "static-latency" else ()):
            for p in i8ref.paths(i8ref.net(g), rows, form, row_map=row_map):
                yield g, rows, p


def _asymmetric(off):
    return sorted(off) != sorted(-o for o in off)


# ------------------------------------------------------ reference agreement --

@pytest.mark.parametrize("geom", GEOMS)
def test_chunk_reference_is_the_oracle(oracle, geom):
    """One block: bit for bit oracle.nnet_propagate_int8 (its scalar u8 GEMM,
    Splice and Narrow in place), although chunk_reference defers the Narrows
    and takes the float64 GEMM wherever the guard lets it."""
    layers = i8ref.net(geom)
    n = i8ref.I8_GEOMETRIES[geom][1][-1]
    for rows in AGREE_ROWS:
        x = netgen.real_input(layers, rows, i8ref.seed_of(geom) + rows)
        log = []
        (got,), ranges, params = i8ref.chunk_reference(oracle, layers, [x], log=log)
        want = oracle.nnet_propagate_int8(layers, x)
        assert got.shape == want.shape == (rows, n) and np.isfinite(want).all()
        assert np.array_equal(bits(got), bits(want)), (geom, rows)
        assert len(ranges) == len(params) == len(log) == len(netgen.linears(layers))
        # no silent wrap: the float64 GEMM only inside static_oracle's guard
        for e in log:
            if e["f64"]:
                assert e["k"] * (255 + abs(e["z"])) * (255 + abs(e["zw"])) < 2 ** 31
                assert 0 <= e["z"] <= 255 and 0 <= e["zw"] <= 255
        assert any(e["f64"] for e in log)


def test_zero_point_outside_a_byte_takes_the_scalar_gemm(oracle):
    """A BatchNorm-only layer that lifts every activation above zero gives the
    next Linear a negative zero point: float64 would disagree with the int32
    ring there, and chunk_reference must not use it."""
    layers = [dict(L) for L in netgen.real_net(40, [32, 36], [[0], [-1, 0, 1]], [("batchnorm",), ()], 11, log_softmax=False)]
    bn = next(L for L in layers if L["kind"] == "batchnorm")
    bn["offset"] = (bn["offset"] + np.float32(1000.0)).astype(np.float32)
    x = netgen.real_input(layers, 17, 12)
    log = []
    (got,), _, params = i8ref.chunk_reference(oracle, layers, [x], log=log)
    assert params[1][1] < 0 and [e["f64"] for e in log] == [True, False]
    assert np.array_equal(bits(got), bits(oracle.nnet_propagate_int8(layers, x)))
    assert not i8ref.f64_gemm_ok(64, -1, 0) and not i8ref.f64_gemm_ok(64, 0, 256)
    assert not i8ref.f64_gemm_ok(2 ** 31 // (255 * 255) + 1, 0, 0) and i8ref.f64_gemm_ok(4096, 255, 255)


def test_blocks_share_parameters(oracle):
    """Several blocks: the ranges are the fold over all of them, and a block's
    rows differ from the same block scored alone."""
    layers = i8ref.net("I1")
    _, utts = i8ref.chunk_inputs("I1")[0]
    blocks = [i8ref.padded(layers, u) for u in utts]
    outs, ranges, _ = i8ref.chunk_reference(oracle, layers, blocks)
    assert [len(o) for o in outs] == list(i8ref.CHUNK_LENGTHS)
    alone = [i8ref.chunk_reference(oracle, layers, [b]) for b in blocks]
    lo = np.min([r[:, 0] for _, r, _ in alone], axis=0)
    hi = np.max([r[:, 1] for _, r, _ in alone], axis=0)
    assert np.array_equal(ranges[:, 0], lo) and np.array_equal(ranges[:, 1], hi)
    assert any(not np.array_equal(bits(o), bits(a[0][0])) for o, a in zip(outs, alone))


# ---------------------------------------------------------------- coverage --

def test_steps_restate_the_loader():
    """The fused / stand-alone split of the post ops, per geometry."""
    for g in GEOMS:
        st = i8ref.steps(i8ref.net(g))
        post = i8ref.I8_GEOMETRIES[g][3]
        assert [tuple(s["post"]) for s in st] == [tuple(p) for p in post], g
        want_ops = {i: [] for i in range(len(st))}
        if g in i8ref.ROW_OPS:
            want_ops[i8ref.ROW_OPS[g][0]] = list(i8ref.ROW_OPS[g][1])
        assert {i: s["row_ops"] for i, s in enumerate(st)} == want_ops, g
    assert i8ref.contexts(i8ref.net("I4")) == [(0, 0), (4, 1), (4, 1), (5, 3)]
    assert i8ref.contexts(i8ref.net("I1")) == [(0, 0), (2, 2), (9, 22)]


def test_dynamic_paths_cover_the_dispatch():
    P = list(_all_paths("dynamic"))
    kt = {p["ktiles"] for _, _, p in P}
    assert {1, 2, 3} <= kt and any(k >= 5 and k % 2 for k in kt) and any(k >= 4 and k % 2 == 0 for k in kt), kt
    # gathered operands: 1, 3 asymmetric, 8 asymmetric segments at din 128 and din >= 256
    gathered = {(p["nseg"], p["nseg"] > 1 and _asymmetric(p["off"]), min(p["din"], 256))
                for _, _, p in P if p["operand"] == "gathered"}
    for nseg, asym in ((1, False), (3, True), (8, True)):
        for din in (128, 256):
            assert (nseg, asym, din) in gathered, (nseg, asym, din, gathered)
    first = [p for _, _, p in P if p["linear"] == 0 and p["operand"] == "gathered"]
    assert first and all(p["din"] == 128 and _asymmetric(p["off"]) and p["quantize"] == "fast" for p in first)
    # ... whose rows go through the row map in am_forward: the general kernel
    via_map = [p for g, _, p in _all_paths("dynamic", row_map=True) if p["linear"] == 0 and p["operand"] == "gathered"]
    assert via_map and all(p["quantize"] == "general-vector" for p in via_map)
    # spliced operands, and the branches of quantize_row / minmax_kernel
    spliced = [p for _, _, p in P if p["operand"] == "spliced"]
    assert any(p["width"] % 4 == 0 for p in spliced) and any(p["width"] % 4 for p in spliced)
    assert {p["quantize"] for _, _, p in P} == {"fast", "general-vector", "general-scalar"}
    assert {p["minmax"] for _, _, p in P} == {"fused", "vector", "scalar"}
    # output widths
    ns = {(p["n"], p["tiles_n"]) for _, _, p in P}
    assert any(n < 128 for n, _ in ns)
    assert any(n % 128 == 0 and t >= 3 for n, t in ns)
    assert any(n % 128 and n % 4 == 0 and t >= 3 for n, t in ns)
    assert any(n % 4 for n, _ in ns)
    assert any(n > 4096 and n % 4 == 0 for n, _ in ns) and any(n > 4096 and n % 4 for n, _ in ns)
    # tile order (tile_of, group 8): more than 8 column tiles on 2 row tiles,
    # and a last group that is short (33 column tiles)
    assert any(p["tiles_n"] > 8 and p["tiles_m"] >= 2 for _, _, p in P)
    assert any(p["tiles_n"] == 33 and p["tiles_m"] == 2 for _, _, p in P)
    # every PostMode on a hidden layer whose min / max is fused, and on a last layer
    modes = {"none", "relu", "bn", "relu+bn", "bn+relu", "generic"}
    assert {p["post"] for _, _, p in P if p["fused_minmax"]} == modes
    assert {p["post"] for g, _, p in P if p["linear"] + 1 == len(i8ref.I8_GEOMETRIES[g][1])} == modes
    # the fused min / max in the scalar epilogue (n % 4 != 0 on a hidden layer) and the vector one
    assert {p["epilogue"] for _, _, p in P if p["fused_minmax"]} == {"scalar", "vector"}
    # a GEMM whose min / max is not fused: a row op follows
    assert any(not p["fused_minmax"] and p["row_ops"] for _, _, p in P)
    assert all(p["epilogue"] != "requantize" for _, _, p in P)


def test_static_paths_cover_the_dispatch():
    P = list(_all_paths("static"))
    modes = {"none", "relu", "bn", "relu+bn", "bn+relu", "generic"}
    assert {p["post"] for _, _, p in P if p["epilogue"] == "requantize"} == modes
    reasons = {r for _, _, p in P for r in p["unfused_because"]}
    assert reasons == {"n % 128", "next spliced", "row op"}
    assert {p["epilogue"] for _, _, p in P} == {"requantize", "vector", "scalar"}
    # behind a requantize epilogue no quantize pass runs
    for g in GEOMS:
        ps = i8ref.paths(i8ref.net(g), 70, "static")
        for a, b in zip(ps, ps[1:]):
            assert (b["quantize"] == "none") == (a["epilogue"] == "requantize"), g
    L = list(_all_paths("static-latency"))
    pair = [p for _, _, p in L if p["slices"][0] > 0]
    assert {p["epilogue"] == "requantize" for p in pair} == {True, False}
    assert {p["post"] for p in pair} == modes
    assert {p["post"] for p in pair if p["epilogue"] == "requantize"} == modes
    # the crossover: the pair up to kI8LatMaxRows GEMM rows, the throughput kernel beyond
    for g, rows, p in L:
        m = rows + sum(netgen.context(i8ref.net(g)))
        assert (p["slices"][0] > 0) == (m <= i8ref.LAT_MAX_ROWS), (g, rows, p)
    assert any(p["slices"][0] > 1 for p in pair) and any(p["slices"][0] == 1 for p in pair)


def test_latency_rows_straddle_the_crossover():
    for g in GEOMS:
        ctx = sum(netgen.context(i8ref.net(g)))
        a, b = i8ref.latency_rows(g)
        assert a >= 1 and (a + ctx, b + ctx) == (i8ref.LAT_MAX_ROWS, i8ref.LAT_MAX_ROWS + 1)
        assert all(p["slices"][0] > 0 for p in i8ref.paths(i8ref.net(g), a, "static-latency")), g
        assert all(p["slices"][0] == 0 for p in i8ref.paths(i8ref.net(g), b, "static-latency")), g


@pytest.mark.parametrize("geom", GEOMS)
def test_central_half_ranges_clamp_both_ends(oracle, geom):
    """The clamp test's inputs, on the reference's bytes alone: with the
    ranges shrunk to their central half every Linear's quantized input holds
    byte 0, byte 255 and interior bytes."""
    from test_int8_static import central_half, fp32_ranges, static_oracle
    layers = i8ref.net(geom)
    half = central_half(fp32_ranges(oracle, layers, i8ref.calibration_input(geom)))
    taps = []
    static_oracle(oracle, layers, i8ref.clamp_input(geom), half, taps)
    assert len(taps) == len(half)
    for i, q in enumerate(taps):
        assert (q == 0).any() and (q == 255).any() and ((q > 0) & (q < 255)).any(), (geom, i)


def test_the_fallback_gemm_is_unreachable():
    """launch_i8_gemm returns CE_GPU_EINVAL when kpad, the loader's segment
    width or the operand's row stride is off a multiple of 128 / 128 / 16 (the
    branch once launched gemm_i8_nnet_kernel, now the experiments library's
    variant 0): quantize_weights pads K to 128 and splices every layer whose
    segments are not whole K-tiles, so no layer of any geometry gets there."""
    for form in ("dynamic", "static", "static-latency"):
        assert not any(p["fallback_gemm"] for _, _, p in _all_paths(form))


def test_variant_cases_cover_the_gemm_paths():
    """What tests/test_gpu_i8_variants.py runs on every kept int8 GEMM variant
    (i8ref.VARIANT_GEOMS x VARIANT_ROWS, dynamic and static) reaches both
    operand forms, the segment changing on every K-tile, the three epilogues,
    the fused min / max in the vector and in the scalar epilogue, one partial
    row tile and two row tiles with a ragged second one, and more than one
    column tile."""
    I8_VARIANT_GEOMS, I8_VARIANT_ROWS = i8ref.VARIANT_GEOMS, i8ref.VARIANT_ROWS
    assert (I8_VARIANT_GEOMS, I8_VARIANT_ROWS) == (("I1", "I3"), (70, 300))
    P = {form: [(g, rows, p) for g in I8_VARIANT_GEOMS for rows in I8_VARIANT_ROWS
                for p in i8ref.paths(i8ref.net(g), rows, form)] for form in ("dynamic", "static")}
    for form, ps in P.items():
        assert {p["operand"] for _, _, p in ps} == {"gathered", "spliced"}, form
        # 8 asymmetric segments of one K-tile each: the loader's offsets change on every K-tile
        assert any(p["operand"] == "gathered" and p["nseg"] == 8 and p["din"] == i8ref.K_ALIGN and
                   p["ktiles"] == 8 and _asymmetric(p["off"]) for _, _, p in ps), form
        for rows, tiles_m in ((70, 1), (300, 2)):
            m = {rows + sum(netgen.context(i8ref.net(g))) for g in I8_VARIANT_GEOMS}
            assert all(i8ref.TILE_M * (tiles_m - 1) < v < i8ref.TILE_M * tiles_m for v in m), (rows, m)
            assert {p["tiles_m"] for _, r, p in ps if r == rows} == {tiles_m}, (form, rows)
        assert any(p["tiles_n"] > 1 for _, _, p in ps), form
        assert not any(p["fallback_gemm"] for _, _, p in ps), form
    dyn, sta = P["dynamic"], P["static"]
    assert {p["epilogue"] for _, _, p in dyn} == {"vector", "scalar"}
    assert {p["epilogue"] for _, _, p in dyn if p["fused_minmax"]} == {"vector", "scalar"}
    assert any(p["n"] == 100 and p["epilogue"] == "vector" and p["minmax"] == "fused" for g, _, p in dyn if g == "I1")
    assert any(p["n"] == 130 and p["epilogue"] == "scalar" and p["operand"] == "spliced" for g, _, p in dyn if g == "I3")
    assert {p["epilogue"] for _, _, p in sta} == {"requantize", "vector", "scalar"}


# --------------------------------------------------------------- sharpness --

def _differs(oracle, layers, blocks, rule):
    _, _, ref = i8ref.chunk_reference(oracle, layers, blocks)
    _, _, alt = i8ref.chunk_reference(oracle, layers, blocks, rule=rule)
    return np.array([a != b for a, b in zip(ref, alt)])


@pytest.mark.parametrize("geom", i8ref.HELD)
def test_held_row_inputs_see_a_wrong_rule(oracle, geom):
    """On the reference alone: folding every row changes the parameters of
    every Linear after the first, and exchanging left and right those of every
    Linear whose contexts differ, for at least one of the blocks the GPU test
    scores.  (The same blocks unscaled, printed below, show an exchanged rule
    on no Linear and a fold of every row on 3 of 14: DESIGN.md §5.)"""
    layers = i8ref.net(geom)
    ctxs = i8ref.contexts(layers)
    inputs = i8ref.held_inputs(geom)
    assert inputs
    every = np.array([_differs(oracle, layers, [x], "all") for _, x in inputs]).any(0)
    swapped = np.array([_differs(oracle, layers, [x], "swapped") for _, x in inputs]).any(0)
    assert not every[0] and every[1:].all(), (geom, every)
    for i, (left, right) in enumerate(ctxs):
        assert swapped[i] == (left != right), (geom, i, ctxs, swapped)
    plain = netgen.real_input(layers, 70, 5000 + i8ref.seed_of(geom))
    print(geom, "N(0, 3) alone: all", _differs(oracle, layers, [plain], "all").astype(int),
          "swapped", _differs(oracle, layers, [plain], "swapped").astype(int))


def test_asymmetric_contexts_are_among_the_held_geometries():
    asym = [g for g in i8ref.HELD if any(l != r for l, r in i8ref.contexts(i8ref.net(g)))]
    assert len(asym) >= 4, asym


@pytest.mark.parametrize("geom", i8ref.CHUNK_SHARP)
def test_packed_chunk_inputs_see_a_wrong_rule(oracle, geom):
    """The packed chunk of am_forward (replicated first / last frames): the
    last Linear's parameters change when every row is folded, and when left
    and right are exchanged where its contexts differ."""
    layers = i8ref.net(geom)
    blocks = [[i8ref.padded(layers, u) for u in utts] for _, utts in i8ref.chunk_inputs(geom)]
    every = np.array([_differs(oracle, layers, b, "all") for b in blocks]).any(0)
    swapped = np.array([_differs(oracle, layers, b, "swapped") for b in blocks]).any(0)
    left, right = i8ref.contexts(layers)[-1]
    assert every[-1] and swapped[-1] == (left != right), (geom, every, swapped)


def test_calibration_inputs_are_exact_and_see_a_wrong_rule(oracle):
    """The calibration case: inside the exact-integer budget, its held-row
    ranges equal those of netgen._walk (Splice + Narrow in place), and the
    wrong rules give other ranges on the Linears where they can."""
    layers, cases = i8ref.calib_case()
    assert netgen.x6_ok(layers)
    every, swapped = np.zeros(3, bool), np.zeros(3, bool)
    for name, utts in cases.items():
        blocks = [i8ref.padded(layers, u) for u in utts]
        want = [[np.float32(np.finfo(np.float32).max), np.float32(np.finfo(np.float32).tiny)] for _ in range(3)]
        for b in blocks:
            netgen.check_exact_budget(layers, b)
            seen = []
            netgen._walk(layers, b, lambda L, a: seen.append(a) if L is not None and L["kind"] == "linear" else None)
            for i, a in enumerate(seen):
                mn, mx = fold_range(a.astype(np.float32))
                want[i] = [min(want[i][0], mn), max(want[i][1], mx)]
        ref = i8ref.fp32_held_ranges(oracle, layers, blocks)
        assert np.array_equal(bits(ref), bits(np.array(want, np.float32))), name
        every |= (i8ref.fp32_held_ranges(oracle, layers, blocks, "all") != ref).any(1)
        swapped |= (i8ref.fp32_held_ranges(oracle, layers, blocks, "swapped") != ref).any(1)
    assert list(every) == [False, True, True] and list(swapped) == [False, False, True]
