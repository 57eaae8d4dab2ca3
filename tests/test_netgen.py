"""The exact-integer nets of tests/netgen.py are exact: for every geometry and
recipe tests/test_gpu_gemm_shapes.py runs, check_exact_budget passes on the
whole input and the oracle gives the same bits in three summation orders
(its naive fp32 loop, an fp64 GEMM, the fp32 loop with K reversed), all equal
to netgen.exact; the f16x3 cases also in an emulation of that kernel's own
arithmetic.  A GPU mismatch on these nets is then the kernel's.

The plane tools (split3_planes, split2_planes) against torch's conversions;
the coverage matrix -- every plane product a form keeps x every position x
every kernel family has an exact case that makes it nonzero there -- and, per
cell, the proof that dropping the product changes output bits."""
import numpy as np
import pytest

import netgen

EMU_ROWS = 12    # output rows of the f16x3 emulation (a Python loop over K)
ORDER_ROWS = 40  # output rows of the three-order check (the budget covers every row)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _f64(a, w):
    return (a.astype(np.float64) @ w.astype(np.float64)).astype(np.float32)


def _f16x3_gemm(order):
    """The f16x3 kernel's own arithmetic on one Linear, as the `product` of
    netgen._walk: both operands as two fp16 planes, a0b0 summed in one fp32
    accumulator and a0b1, a1b0 in a second (K ascending with a0b1 first, or
    K descending with a1b0 first), the epilogue's (acc0 + 2^-11 acc1) *
    unscale in fp32.  The hidden outputs are split again by the next call."""
    def product(n, a, W):
        sw = netgen.f16_weight_shift(W)
        x0, x1 = netgen.split2_raw(a, netgen.F16_ACT_SHIFT)
        w0, w1 = netgen.split2_raw(W, sw)
        acc0 = np.zeros((a.shape[0], W.shape[1]), np.float32)
        acc1 = np.zeros_like(acc0)
        ks = np.flatnonzero((W != 0.0).any(axis=1))   # a zero weight row adds +0.0
        for k in (ks if order == "ascending" else ks[::-1]):
            acc0 += np.outer(x0[:, k], w0[k])
            cross = [np.outer(x0[:, k], w1[k]), np.outer(x1[:, k], w0[k])]
            for t in (cross if order == "ascending" else cross[::-1]):
                acc1 += t
        assert acc0.dtype == acc1.dtype == np.float32
        unscale = np.float32(np.ldexp(1.0, -(sw + netgen.F16_ACT_SHIFT)))
        return ((acc0 + acc1 * np.float32(1.0 / 2048.0)) * unscale).astype(np.float64)
    return product


@pytest.mark.parametrize("geom", sorted(netgen.GEOMETRIES))
def test_exact_cases_are_order_independent(oracle, geom):
    for form, (name, layers, x) in [(f, c) for f in netgen.FORMS for c in netgen.exact_cases(geom, f)]:
        left, right = netgen.context(layers)
        assert x.shape[0] == netgen.max_rows(geom, name) + left + right
        if "*2^" not in name:  # the shifted forms: the same products, scaled exactly (binade_shift)
            bounds = netgen.check_exact_budget(layers, x, form)
            assert len(bounds) == len(netgen.GEOMETRIES[geom][1])
        want = netgen.exact(layers, x)
        assert want.shape == (netgen.max_rows(geom, name), netgen.GEOMETRIES[geom][1][-1])
        xs = x[:ORDER_ROWS + left + right]
        naive = oracle.nnet_propagate(layers, xs)
        assert naive.shape == (ORDER_ROWS, want.shape[1])
        assert np.array_equal(bits(naive), bits(want[:ORDER_ROWS])), f"{geom} {name}: naive fp32"
        f64 = oracle.nnet_propagate(layers, xs, gemm=_f64)
        assert np.array_equal(bits(f64), bits(naive)), f"{geom} {name}: fp64 GEMM"
        rev = oracle.nnet_propagate(layers, xs, gemm=lambda a, w: oracle.sgemm(a[:, ::-1], w[::-1]))
        assert np.array_equal(bits(rev), bits(naive)), f"{geom} {name}: K reversed"
        if form == "f16x3":
            for order in ("ascending", "descending"):
                emu = netgen._walk(layers, xs[:EMU_ROWS + left + right], product=_f16x3_gemm(order)).astype(np.float32)
                assert np.array_equal(bits(emu), bits(naive[:EMU_ROWS])), f"{geom} {name}: f16x3 arithmetic, K {order}"


@pytest.mark.parametrize("geom", sorted(netgen.GEOMETRIES))
def test_every_k_tile_reaches_the_output(geom):
    """The nets can see what the kernels can get wrong: leaving out any one
    32-wide K-tile of any Linear (a dropped loop tail, a clamped prefetch used
    for real, a slice cut short) changes the output of every row."""
    _, layers, x = netgen.exact_cases(geom)[0]
    left, right = netgen.context(layers)
    xs = x[:ORDER_ROWS + left + right]
    want = netgen.exact(layers, xs)
    for li, L in enumerate(layers):
        if L["kind"] != "linear":
            continue
        for k0 in range(0, L["W"].shape[0], 32):
            W = L["W"].copy()
            W[k0:k0 + 32] = 0.0
            got = netgen.exact(layers[:li] + [dict(L, W=W)] + layers[li + 1:], xs)
            assert np.all((got != want).any(axis=1)), f"{geom}: layer {li}, K-tile at {k0} does not matter"


def test_binade_shift_keeps_the_bits():
    for geom in netgen.BINADE:
        cases = dict((n, (l, x)) for n, l, x in netgen.exact_cases(geom))
        for recipe in ("wide",) + (netgen.PLANE_BINADE if geom == "A" else ()):
            base_layers, base_x = cases[recipe]
            want = netgen.exact(base_layers, base_x)
            head = slice(0, 17 + sum(netgen.context(base_layers)))
            for e in (60, -60):
                layers, x = cases[f"{recipe}*2^{e}"]
                assert np.abs(x).max() == np.ldexp(np.abs(base_x).max(), e)
                assert np.array_equal(bits(netgen.exact(layers, x)), bits(want))
                # the same plane products, |e| binades away: a third plane survives the distant exponent
                assert netgen.census(layers, x[head], "bf16x6") == netgen.census(base_layers, base_x[head], "bf16x6")
    cases = dict((n, (l, x[:40])) for n, l, x in netgen.exact_cases("A"))
    assert (0, 2) in netgen.census(*cases["W3@0*2^60"], "bf16x6")[0]
    assert (2, 0) in netgen.census(*cases["A3*2^-60"], "bf16x6")[0]


def test_budget_rejects_an_inexact_recipe():
    """|w| <= 32767 with 8 nonzeros per column leaves the budget: the
    generator's check must say so rather than assume exactness."""
    in_d, widths, splices, post = netgen.GEOMETRIES["B"]
    layers = netgen.int_net(in_d, widths, splices, post, [(32767, 8)] * 3, seed=5)
    with pytest.raises(AssertionError):
        netgen.check_exact_budget(layers, netgen.int_input(layers, 17, seed=6, amax=2047))
    layers = netgen.int_net(in_d, widths, splices, post, netgen.WIDE, seed=5)
    x = netgen.int_input(layers, 17, seed=6)
    netgen.check_exact_budget(layers, x)
    with pytest.raises(AssertionError):
        netgen.check_exact_budget(layers, x + np.float32(0.5))
    # f16x3: the WIDE recipe's third layer reads values beyond 2047 (two fp16
    # planes) but its weights fit one, so the dropped a1b1 is zero there ...
    netgen.check_exact_budget(layers, x, "f16x3")
    assert (1, 1) not in netgen.census(layers, x, "f16x3")[2] and (1, 0) in netgen.census(layers, x, "f16x3")[2]
    # ... and is not when both operands of a Linear need two planes
    two = netgen.int_net(in_d, widths, splices, post, [(2500, 1, 2049), (1, 1), (1, 1)], seed=5, bn_scales=(1.0, -1.0))
    x2 = netgen.int_input(two, 17, seed=6, amax=2500, amin=2049)
    netgen.check_exact_budget(two, x2)
    with pytest.raises(AssertionError, match="a1b1"):
        netgen.check_exact_budget(two, x2, "f16x3")
    # a hidden output of 24 significant bits does not come back from two fp16 planes
    big = netgen.int_net(in_d, widths, splices, post, [((1 << 21) - 1, 1, 1 << 20), (1, 1), (1, 1)], seed=5,
                         bn_scales=(1.0,), bias=4)
    netgen.check_exact_budget(big, x)
    with pytest.raises(AssertionError, match="two planes do not hold the activations"):
        netgen.check_exact_budget(big, x, "f16x3")


def test_every_post_mode_is_covered():
    """Each post chain the loader maps to a PostMode sits on a hidden layer
    and on a last layer of a geometry the bf16x6 program takes with n <= 4096
    (where latency mode applies it in lat_finalize)."""
    modes = {(), ("relu",), ("batchnorm",), netgen.RB, netgen.BR, netgen.RBR}
    hidden, last = set(), set()
    for geom, (_, widths, _, post) in netgen.GEOMETRIES.items():
        if geom in ("E", "F4099") or widths[-1] > 4096:
            continue
        hidden.update(post[:-1])
        last.add(post[-1])
    assert hidden == modes and last == modes


def test_real_net_matches_its_layers(oracle):
    in_d, widths, splices, post = netgen.GEOMETRIES["C"]
    layers = netgen.real_net(in_d, widths, splices, post, seed=3)
    assert layers[-1]["kind"] == "log_softmax"
    x = netgen.real_input(layers, 9, seed=4)
    ref = oracle.nnet_propagate(layers, x)
    got = netgen.eval_f64(layers, x)
    assert got.shape == ref.shape == (9, 100)
    assert np.abs(got - ref).max() <= 1e-4


def _net(geom):
    in_d, widths, splices, post = netgen.GEOMETRIES[geom]
    return netgen.int_net(in_d, widths, splices, post, netgen.WIDE, seed=1)


def test_geometries_reach_their_paths():
    """Each geometry's reason for being there, from the dispatch rules
    (netgen.kernels restates them)."""
    K = netgen.kernels
    # A: the 512 x 128 kernel with an odd K tail (9 and 25 tiles) and a ragged
    # last unit tile (772) at 3000 rows, 256 x 128 at 70, 128 x 128 when wide
    a = _net("A")
    assert K(a, 3000, "bf16x6") == ["x6d_128x128_gather[kt=8]", "x6w_512x128[kt=9]", "x6w_512x128[kt=25]"]
    assert K(a, 70, "bf16x6")[1:] == ["x6d_256x128[kt=9]", "x6d_256x128[kt=25]"]
    assert K(a, 70, "wide")[1:] == ["x6d_128x128[kt=9]", "x6d_128x128[kt=25]"]
    assert 772 % 128 != 0 and (772 + 255) // 256 * 256 >= 2 * 512
    # B: one K-tile; an unspliced first layer gathered by the loader; n = 36
    assert K(_net("B"), 70, "bf16x6") == ["x6d_128x128_gather[kt=2]", "x6d_256x128[kt=1]", "x6d_256x128[kt=2]"]
    assert netgen.linears(_net("B"))[0]["nseg"] == 1
    assert K(_net("B"), 70, "latency")[1] == "lat_gemm<KT=2>[1]+lat_reduce"
    # C: 24-wide segments (seams inside the loader's 8-float chunks at every
    # third chunk), 8 asymmetric segments, offsets beyond a 16-row block
    c = netgen.linears(_net("C"))
    assert c[0]["din"] == 24 and c[0]["k"] == 168 and K(_net("C"), 70, "bf16x6")[0] == "x6d_128x128_gather[kt=6]"
    assert c[1]["nseg"] == 8 and max(c[1]["off"]) > 16 and -min(c[1]["off"]) != max(c[1]["off"])
    # D: in_dim % 8 != 0 -> splice_pad; after it the first layer is an
    # ordinary one and a large block takes the 512 x 128 kernel; n = 1028 has
    # the tiles for it (3 x 24 >= 48) but the fragment image does not cover
    # the last 512-unit tile
    d = _net("D")
    assert K(d, 3000, "bf16x6") == ["splice_pad+x6w_512x128[kt=4]", "x6d_256x128[kt=75]", "x6d_256x128[kt=8]"]
    assert (1028 + 255) // 256 * 256 < 3 * 512
    assert K(d, 70, "latency")[0].startswith("splice_pad+lat_gemm")
    # E: not the bf16x6 program, padded segments on every layer, odd n
    assert not netgen.x6_ok(_net("E")) and netgen.finalize_path(37) == "scalar"
    assert K(_net("E"), 70, "bf16x6") == ["splice_pad+f32_glds"] * 3
    # F: n > 4096 leaves the fused reduce + finalize and the in-register finalize
    assert netgen.x6_ok(_net("F4100")) and not netgen.x6_ok(_net("F4099"))
    assert K(_net("F4100"), 70, "latency")[2] == "lat_gemm<KT=8>[7,7,6]+lat_reduce"
    assert netgen.finalize_path(4100) == netgen.finalize_path(4099) == "loop"
    # G: latency slices of 3, of 7 with a shorter tail, of 5
    assert K(_net("G9"), 70, "latency")[1] == "lat_gemm<KT=4>[3,3,3]+lat_finalize"
    assert K(_net("G25"), 70, "latency")[1] == "lat_gemm<KT=8>[7,7,7,4]+lat_finalize"
    assert K(_net("G20"), 70, "latency")[1] == "lat_gemm<KT=6>[5,5,5,5]+lat_finalize"
    assert K(_net("G25"), 3000, "bf16x6")[1] == "x6w_512x128[kt=25]"
    # H: first-layer segments of two whole K-tiles: no splice_pad in any
    # program, the caller's rows reach the fp32 LDS-DMA kernel and the generic
    # (not `first`) direct-weight kernel through the splice offsets
    h = _net("H")
    assert netgen.x6_ok(h) and netgen.linears(h)[0]["din"] == 64 and netgen.linears(h)[0]["nseg"] == 3
    assert K(h, 70, "fp32") == ["f32_glds"] * 3
    assert K(h, 70, "bf16x6") == ["x6d_256x128[kt=6]", "x6d_256x128[kt=9]", "x6d_256x128[kt=2]"]
    assert K(h, 70, "latency") == ["lat_gemm<KT=2>[1,1,1,1,1,1]+lat_reduce",
                                   "lat_gemm<KT=2>[1,1,1,1,1,1,1,1,1]+lat_reduce", "lat_gemm<KT=2>[1,1]+lat_finalize"]
    # the shapes the existing models already cover give the rule's known answers
    assert netgen.lat_slices(32, 1024) == [2] * 16 and netgen.lat_slices(96, 1024) == [6] * 16


def test_unaligned_caller_rows_leave_the_fast_paths():
    """A caller's block that is not made of float4 rows (base off 16 bytes, or
    ld_in % 4 != 0; netgen.kernels' caller_aligned=False): the bf16x6 and
    latency first layers that gather the caller's rows go through splice_pad
    instead, a whole-K-tile fp32 first layer leaves the LDS-DMA kernel; the
    programs that pad anyway, and every later layer, stay as they are."""
    def K(geom, mode):
        return netgen.kernels(_net(geom), 70, mode, caller_aligned=False)

    assert K("A", "bf16x6") == ["splice_pad+x6d_256x128[kt=8]", "x6d_256x128[kt=9]", "x6d_256x128[kt=25]"]
    assert K("C", "bf16x6") == ["splice_pad+x6d_256x128[kt=6]", "x6d_256x128[kt=24]", "x6d_256x128[kt=2]"]
    assert K("H", "bf16x6") == ["splice_pad+x6d_256x128[kt=6]", "x6d_256x128[kt=9]", "x6d_256x128[kt=2]"]
    assert K("A", "wide")[0] == "splice_pad+x6d_128x128[kt=8]"
    assert K("A", "latency")[0] == "splice_pad+lat_gemm<KT=2>[1,1,1,1,1,1,1,1]+lat_reduce"
    assert K("C", "latency")[0] == "splice_pad+lat_gemm<KT=2>[1,1,1,1,1,1]+lat_reduce"
    assert K("H", "latency")[0] == "splice_pad+lat_gemm<KT=2>[1,1,1,1,1,1]+lat_reduce"
    assert K("H", "fp32") == ["f32_pipe2", "f32_glds", "f32_glds"]
    assert K("A", "fp32") == ["splice_pad+f32_glds", "f32_glds", "f32_glds"]
    for geom in ("A", "C", "H"):
        for mode in ("bf16x6", "wide", "latency"):
            assert K(geom, mode)[1:] == netgen.kernels(_net(geom), 70, mode)[1:]
    for geom in ("D", "E"):
        for mode in ("fp32", "bf16x6", "bf16x6p", "wide", "latency"):
            assert K(geom, mode) == netgen.kernels(_net(geom), 70, mode), (geom, mode)
    for geom in ("A", "C", "D", "H"):
        assert K(geom, "bf16x6p") == netgen.kernels(_net(geom), 70, "bf16x6p"), geom


# ------------------------------------------------------------- the planes --

def _edge_values():
    rng = np.random.default_rng(11)
    v = [rng.integers(-(1 << 24) + 1, 1 << 24, size=20000).astype(np.float32),           # integers, 24 bits
         rng.standard_normal(20000).astype(np.float32),
         np.ldexp(rng.standard_normal(2000), rng.integers(-100, 100, size=2000)).astype(np.float32)]
    # rounding ties of each plane: 8 significant bits followed by exactly one half, even and odd
    base = np.arange(128, 256, dtype=np.float64)
    for tail in (0.5, 0.5 + 2.0 ** -9, 0.5 - 2.0 ** -9, 0.5 + 2.0 ** -8 * 0.5, 0.5 + 2.0 ** -15):
        v.append((base + tail).astype(np.float32))
        v.append(-np.ldexp(base + tail, 40).astype(np.float32))
    v.append(np.array([0.0, -0.0, 1.0, 255.0, 256.0, 257.0, 65535.0, 65536.0, 65537.0, 131071.0, 131073.0,
                       (1 << 24) - 1, 1 << 24, 2.0 ** -126, 2.0 ** 100, 3.0e38 / 4], np.float32))
    return np.concatenate(v)


def test_split3_planes_against_torch():
    """split3_planes is three float32 -> bfloat16 conversions of exact
    residuals: each plane equals torch's conversion of what is left, the
    planes sum to the value, and a plane is at most half an ulp of the one
    before it."""
    import torch
    v = _edge_values()
    h, m, l = netgen.split3_planes(v)

    def bf16(a):
        a32 = a.astype(np.float32)
        assert np.array_equal(a32.astype(np.float64), a)   # the residual is a float32
        return torch.from_numpy(a32).to(torch.bfloat16).to(torch.float64).numpy()

    v64 = v.astype(np.float64)
    assert np.array_equal(h, bf16(v64))
    assert np.array_equal(m, bf16(v64 - h))
    assert np.array_equal(l, bf16(v64 - h - m))
    assert np.array_equal(h + m + l, v64)
    assert np.all(np.abs(m) <= np.abs(h) * 2.0 ** -8) and np.all(np.abs(l) <= np.abs(m) * 2.0 ** -8)
    # 17 significant bits fit two planes (a negative m reaches one bit further), 18 need the third
    assert netgen.split3_planes(np.float32(131071.0))[2] == 0.0
    assert netgen.split3_planes(np.float32(131073.0))[2] == 0.0          # 2^17 + 1: h and m hold it
    assert netgen.split3_planes(np.float32(131585.0)) == (132096.0, -512.0, 1.0)
    assert netgen.split3_planes(np.float32((1 << 18) - 1))[2] == 0.0
    assert netgen.split3_planes(np.float32((1 << 18) + 257))[2] == 1.0


def test_split2_planes_against_torch():
    import torch
    rng = np.random.default_rng(12)
    v = np.concatenate([rng.integers(-(1 << 22), 1 << 22, size=20000), np.arange(2040, 2060), [4097, 4095, 0, 1, -1]])
    v = v.astype(np.float32)
    for s in (netgen.F16_ACT_SHIFT, -3, 0, 5):
        if np.abs(np.ldexp(v, s)).max() >= 65504:
            continue
        x0, x1 = netgen.split2_raw(v, s)
        u = torch.from_numpy(np.ldexp(v, s).astype(np.float32))
        t0 = u.to(torch.float16)
        t1 = ((u - t0.to(torch.float32)) * 2048.0).to(torch.float16)
        assert np.array_equal(x0, t0.to(torch.float32).numpy()) and np.array_equal(x1, t1.to(torch.float32).numpy())
        p0, p1 = netgen.split2_planes(v, s)
        assert np.array_equal(p0 + p1, v.astype(np.float64))        # 22 bits: two planes of 11
    # the weight scale: max |w| 2^s in [2^14, 2^15)
    for mx, s in ((1.0, 14), (3.0, 13), (2047.0, 4), (2048.0, 3), (16383.0, 1), (16384.0, 0), (0.75, 15), (0.0, 15)):
        assert netgen.f16_weight_shift(np.array([[mx, -mx / 2]], np.float32)) == s, mx
    # 2049 = 2048 + 1: the second plane holds the 1
    assert [p[0] for p in netgen.split2_planes(np.array([2049.0], np.float32), netgen.F16_ACT_SHIFT)] == [2048.0, 1.0]


# ---------------------------------------------------- the coverage matrix --

def _show(cells):
    return "\n".join(f"{f} / {pos} / a{i}b{j}" for (f, pos, (i, j)) in cells)


def _recipes(form):
    """Every plane recipe by its full name (W3@0, W3@1, ...)."""
    return sorted({name for geom in netgen.GEOMETRIES for name in netgen.recipe_names(geom, form)})


@pytest.mark.parametrize("form", netgen.FORMS)
def test_every_kept_product_reaches_every_kernel(form):
    """For every plane product the form computes, every position (first,
    hidden, last of a two-Linear net, last of a three-Linear net) and every
    kernel family, some exact case has the product nonzero at a Linear that
    runs that kernel, at a row count and in a mode the GPU test scores it at.
    The cells left out are left out by rule: a family has cells at the
    positions it can run at (netgen.FAMILIES), and runs nowhere else.
    Every single recipe (W3@0, W3@1, W3@2, A3, P11@1, P11@2; FX, FW@0, FW@1,
    FW@2) holds cells that no other case fills: deleting or breaking one
    empties them.  F1 alone adds no product (a0b0 is everywhere); what it is
    there for is asserted in test_f1_runs_wherever_f16x3_does."""
    cells = netgen.coverage(form)
    assert {(f, pos) for f, pos, _ in cells} == {(f, pos) for f, (positions, _) in netgen.FAMILIES[form].items()
                                                 for pos in positions}
    assert {pair for _, _, pair in cells} == set(netgen.KEPT[form])
    empty = [c for c, w in cells.items() if not w]
    assert not empty, "no exact case reaches\n" + _show(empty)
    recipes = _recipes(form)
    assert recipes == {"bf16x6": ["A3", "P11@1", "P11@2", "W3@0", "W3@1", "W3@2"],
                       "f16x3": ["F1", "FW@0", "FW@1", "FW@2", "FX"]}[form]
    for recipe in recipes:
        if recipe != "F1":
            assert [c for c, w in netgen.coverage(form, skip=(recipe,)).items() if not w], f"nothing rests on {recipe}"
    # a family runs nowhere outside the positions it lists
    for geom, name, li, pos, mode, r, k, _ in netgen.launches(form):
        hit = [f for f, (positions, match) in netgen.FAMILIES[form].items() if match(k)]
        assert hit, f"{geom} {name}: {k} is in no family"
        for f in hit:
            assert pos in netgen.FAMILIES[form][f][0], f"{geom} {name}: {k} runs at {pos}"


def test_f1_runs_wherever_f16x3_does():
    """F1 is the f16x3 case of the geometries FX and FW leave out: every
    geometry the bf16x6 / f16x3 programs take has an f16x3 case, with a0b0
    nonzero at every Linear and, under F1, nothing else."""
    for geom, (in_d, widths, splices, post) in netgen.GEOMETRIES.items():
        ok = netgen.x6_ok(netgen.int_net(in_d, widths, splices, post, netgen.WIDE, seed=1))
        cases = netgen._case_census(geom, "f16x3")
        assert bool(cases) == ok, geom
        for name, _, nonzero in cases:
            assert all((0, 0) in s for s in nonzero), (geom, name)
            if name in ("F1", "wide"):   # wide: B2's, every operand one fp16 plane
                assert all(s == {(0, 0)} for s in nonzero), geom
        assert not ok or "F1" in [name for name, _, _ in cases], geom


def test_census_before_the_plane_recipes():
    """What the WIDE and TWO_PLANES cases alone reach (the table in DESIGN.md):
    a0b2 nowhere, a1b1 and a0b1 in first Linears only, a2b0 in no first one."""
    first, later = {}, {}
    for geom in netgen.GEOMETRIES:
        for name, layers, nonzero in netgen._case_census(geom, "bf16x6"):
            if name in ("wide", "two-planes"):
                first.setdefault(name, set()).update(nonzero[0])
                later.setdefault(name, set()).update(*nonzero[1:])
    assert first == {"wide": {(0, 0)}, "two-planes": {(0, 0), (0, 1), (1, 0), (1, 1)}}
    assert later == {"wide": {(0, 0), (1, 0)}, "two-planes": {(0, 0), (1, 0), (2, 0)}}


@pytest.mark.parametrize("form", netgen.FORMS)
def test_a_dropped_product_changes_the_output(form):
    """The mutation the GPU test must be able to see.  Each cell of the matrix
    has a witness (geometry, case, Linear); on the largest block at which the
    GPU test scores that witness on a kernel of the cell's family (129 rows,
    3000 where the cell needs them), the net evaluated with that one plane
    product left out of that one Linear (what a kernel that skipped it, or
    read a wrong plane image there, computes) differs from netgen.exact in at
    least one row of every 128-row tile of the block, and within the first 17
    rows.  Among a cell's witnesses the one with the smallest such block is
    taken."""
    mutations = {}
    for (f, pos, pair), witnesses in netgen.coverage(form).items():
        largest = {}
        for geom, name, li, mode, r in witnesses:
            largest[geom, name, li] = max(largest.get((geom, name, li), 0), r)
        (geom, name, li), r = min(largest.items(), key=lambda kv: (kv[1], kv[0]))
        assert r >= netgen.ROWS[-1]
        key = (geom, name, li, pair)
        mutations[key] = max(mutations.get(key, 0), r)
    assert len(mutations) >= len(netgen.KEPT[form]) * 4
    cases = {}
    for (geom, name, li, pair), r in sorted(mutations.items()):
        if geom not in cases:
            cases.clear()      # one geometry's inputs at a time
            cases[geom] = {n: (l, x, netgen.exact(l, x)) for n, l, x in netgen.exact_cases(geom, form)}
        layers, x, want = cases[geom][name]
        assert r <= want.shape[0]
        got = netgen.drop_product(layers, x[:r + sum(netgen.context(layers))], li, pair, form)
        differs = (bits(got) != bits(want[:r])).any(axis=1)
        label = f"{form} {geom} {name} Linear {li} a{pair[0]}b{pair[1]}"
        assert differs[:17].any(), f"{label}: the first 17 rows do not see it"
        for r0 in range(0, r, 128):
            assert differs[r0:r0 + 128].any(), f"{label}: rows {r0}.. of {r} do not see it"
