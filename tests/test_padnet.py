"""tests/padnet.py's re-layout is what ce_gpu_model_pad_widths claims to be
(no GPU): the padded net is an x6 program, computes the original net's bits
in its first n columns, keeps every pad column at +0, stays inside the exact
budget, and reaches the kernels each geometry is there for."""
import functools

import numpy as np
import pytest

import netgen
import padnet

ROWS = 40  # output rows of the value checks (the budget covers every row)
CASES = [(g, r) for g in sorted(padnet.GEOMETRIES) for r in sorted(padnet.RECIPES)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(geom, recipe):
    (layers, x), = [(l, x) for name, l, x in padnet.exact_cases(geom) if name == recipe]
    return layers, x, padnet.pad_layers(layers)


@pytest.mark.parametrize("geom,recipe", CASES)
def test_padded_net_is_an_x6_program(geom, recipe):
    layers, _, padded = case(geom, recipe)
    assert not netgen.x6_ok(layers) and netgen.x6_ok(padded)
    assert padnet.widths(layers) == padnet.GEOMETRIES[geom][1]
    assert padnet.widths(padded) == padnet.PADDED_WIDTHS[geom]
    assert netgen.context(padded) == netgen.context(layers) and netgen.in_dim(padded) == netgen.in_dim(layers)
    for g, p in zip(netgen.linears(layers), netgen.linears(padded)):
        assert (p["nseg"], p["off"]) == (g["nseg"], g["off"])
    # padding a padded net changes nothing (the entry's "already inside the envelope")
    again = padnet.pad_layers(padded)
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(again, padded) if a["kind"] == "linear" for k in ("W", "b"))


@pytest.mark.parametrize("geom,recipe", CASES)
def test_padded_net_computes_the_original_bits(geom, recipe):
    layers, x, padded = case(geom, recipe)
    left, right = netgen.context(layers)
    xs = x[:ROWS + left + right]
    want = netgen.exact(layers, xs)
    got = netgen.exact(padded, xs)
    n = want.shape[1]
    assert got.shape == (ROWS, padnet.PADDED_WIDTHS[geom][-1])
    assert np.array_equal(bits(got[:, :n]), bits(want))
    assert np.array_equal(bits(got[:, n:]), np.zeros((ROWS, got.shape[1] - n), np.uint32))  # +0


@pytest.mark.parametrize("geom,recipe", CASES)
def test_every_pad_column_is_plus_zero(geom, recipe):
    """Every Linear of the padded net reads +0 in its pad columns (the bits,
    so not -0 either) and its true columns are the original net's input."""
    layers, x, padded = case(geom, recipe)
    left, right = netgen.context(layers)
    xs = x[:ROWS + left + right]
    seen = {"orig": [], "pad": []}

    def visit_into(key):
        def visit(L, a):
            if L is not None and L["kind"] == "linear":
                seen[key].append(np.array(a))
        return visit

    netgen._walk(layers, xs, visit_into("orig"))
    netgen._walk(padded, xs, visit_into("pad"))
    masks = padnet.pad_columns(layers)
    assert len(seen["orig"]) == len(seen["pad"]) == len(masks) == 3
    hidden = padnet.GEOMETRIES[geom][1][:-1]  # P4's hidden widths are whole K-tiles: only its output is padded
    assert not masks[0].any() and [bool(m.any()) for m in masks[1:]] == [n % 32 != 0 for n in hidden]
    for a, p, m in zip(seen["orig"], seen["pad"], masks):
        assert np.array_equal(p[:, ~m], a)
        assert not np.any(p[:, m].view(np.uint64)), "a pad column is not +0"


@pytest.mark.parametrize("geom,recipe", CASES)
def test_padded_net_stays_inside_the_exact_budget(geom, recipe):
    layers, x, padded = case(geom, recipe)
    assert netgen.check_exact_budget(padded, x) == netgen.check_exact_budget(layers, x)


def _padded_kernels(geom, rows, mode):
    return padnet.kernels(case(geom, "wide")[0], rows, mode)


def test_geometries_reach_their_paths():
    """Each geometry's reason for being there, from the dispatch rules
    (netgen.kernels on the padded net; padnet.kernels adds the one choice
    that reads the true width)."""
    K = _padded_kernels
    # P1: as loaded the fp32 program pads every layer's segments; padded, the
    # 40-wide first layer is gathered by the loader, the hidden layers are
    # whole K-tiles (5 x 128 and 3 x 128), and the 37 true outputs still end
    # in the scalar finalize -- with the reduce unfused in latency mode
    p1 = case("P1", "wide")[0]
    assert netgen.kernels(p1, 70, "bf16x6") == ["splice_pad+f32_glds"] * 3
    assert K("P1", 70, "bf16x6") == ["x6d_128x128_gather[kt=8]", "x6d_256x128[kt=12]", "x6d_256x128[kt=4]"]
    assert netgen.finalize_path(37) == "scalar"
    assert K("P1", 70, "latency")[2] == "lat_gemm<KT=2>[1,1,1,1]+lat_reduce"
    # P2: 24-wide first-layer segments and 8 asymmetric segments of 96 (72 true)
    p2 = netgen.linears(case("P2", "wide")[2])
    assert p2[0]["din"] == 24 and (p2[1]["nseg"], p2[1]["din"], p2[1]["k"]) == (8, 96, 768)
    assert K("P2", 70, "bf16x6") == ["x6d_128x128_gather[kt=6]", "x6d_256x128[kt=24]", "x6d_256x128[kt=2]"]
    assert netgen.finalize_path(101) == "scalar"
    # P3: 13-wide input -> splice_pad; 780 -> 800 takes the 512 x 128 kernel
    # on its first hidden layer at 3000 rows; an odd 75 K-tiles behind it
    assert K("P3", 3000, "bf16x6") == ["splice_pad+x6w_512x128[kt=4]", "x6d_256x128[kt=75]", "x6d_256x128[kt=4]"]
    assert K("P3", 70, "bf16x6")[0] == "splice_pad+x6d_256x128[kt=4]"
    assert K("P3", 70, "latency")[2].endswith("+lat_reduce") and netgen.finalize_path(1029) == "scalar"
    # P4: 4099 -> 4100 > 4096: the unfused lat_reduce and the loop finalize at width 4099
    assert K("P4", 70, "latency")[2] == "lat_gemm<KT=8>[7,7,6]+lat_reduce"
    assert netgen.finalize_path(4099) == "loop"
    assert K("P4", 70, "bf16x6") == netgen.kernels(
        netgen.int_net(*netgen.GEOMETRIES["F4100"], netgen.WIDE, seed=1), 70, "bf16x6")


def test_pad_layers_refuses_a_softmax_over_pads():
    in_d, widths, splices, post = padnet.GEOMETRIES["P1"]
    with pytest.raises(AssertionError):
        padnet.pad_layers(netgen.real_net(in_d, widths, splices, post, seed=1))
    ok = netgen.real_net(in_d, widths[:-1] + [40], splices, post, seed=1)
    assert padnet.pad_layers(ok)[-1]["kind"] == "log_softmax"
