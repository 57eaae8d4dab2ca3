"""The exact-integer nets of tests/netgen.py are exact: for every geometry and
recipe tests/test_gpu_gemm_shapes.py runs, check_exact_budget passes on the
whole input and the oracle gives the same bits in three summation orders
(its naive fp32 loop, an fp64 GEMM, the fp32 loop with K reversed), all equal
to netgen.exact.  A GPU mismatch on these nets is then the kernel's."""
import numpy as np
import pytest

import netgen

ORDER_ROWS = 40  # output rows of the three-order check (the budget covers every row)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _f64(a, w):
    return (a.astype(np.float64) @ w.astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize("geom", sorted(netgen.GEOMETRIES))
def test_exact_cases_are_order_independent(oracle, geom):
    for name, layers, x in netgen.exact_cases(geom):
        left, right = netgen.context(layers)
        assert x.shape[0] == netgen.max_rows(geom) + left + right
        if "*2^" not in name:  # the shifted forms: the same products, scaled exactly (binade_shift)
            bounds = netgen.check_exact_budget(layers, x, plane_max=2047 if geom == "B2" else None)
            assert len(bounds) == len(netgen.GEOMETRIES[geom][1])
        want = netgen.exact(layers, x)
        assert want.shape == (netgen.max_rows(geom), netgen.GEOMETRIES[geom][1][-1])
        xs = x[:ORDER_ROWS + left + right]
        naive = oracle.nnet_propagate(layers, xs)
        assert naive.shape == (ORDER_ROWS, want.shape[1])
        assert np.array_equal(bits(naive), bits(want[:ORDER_ROWS])), f"{geom} {name}: naive fp32"
        f64 = oracle.nnet_propagate(layers, xs, gemm=_f64)
        assert np.array_equal(bits(f64), bits(naive)), f"{geom} {name}: fp64 GEMM"
        rev = oracle.nnet_propagate(layers, xs, gemm=lambda a, w: oracle.sgemm(a[:, ::-1], w[::-1]))
        assert np.array_equal(bits(rev), bits(naive)), f"{geom} {name}: K reversed"


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
        want = netgen.exact(*cases["wide"])
        for e in (60, -60):
            layers, x = cases[f"wide*2^{e}"]
            assert np.abs(x).max() == np.ldexp(np.abs(cases["wide"][1]).max(), e)
            assert np.array_equal(bits(netgen.exact(layers, x)), bits(want))


def test_budget_rejects_an_inexact_recipe():
    """|w| <= 32767 with 8 nonzeros per column leaves the budget: the
    generator's check must say so rather than assume exactness."""
    in_d, widths, splices, post = netgen.GEOMETRIES["B"]
    layers = netgen.int_net(in_d, widths, splices, post, [(32767, 8)] * 3, seed=5)
    with pytest.raises(AssertionError):
        netgen.check_exact_budget(layers, netgen.int_input(layers, 17, seed=6, amax=2047))
    # one fp16 plane: the WIDE recipe's third layer reads values beyond 2047
    layers = netgen.int_net(in_d, widths, splices, post, netgen.WIDE, seed=5)
    x = netgen.int_input(layers, 17, seed=6)
    netgen.check_exact_budget(layers, x)
    with pytest.raises(AssertionError):
        netgen.check_exact_budget(layers, x, plane_max=2047)
    with pytest.raises(AssertionError):
        netgen.check_exact_budget(layers, x + np.float32(0.5))


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
