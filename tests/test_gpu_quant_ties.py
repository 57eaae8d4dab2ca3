"""Every quantizer on the rounding ties of its range (tests/quantties.py has
the inputs and the CPU proofs that they tell a 1-ulp quotient error apart).

Bit for bit against the oracle's pieces -- oracle.quantize,
oracle._quantize_with, static_oracle, i8ref.chunk_reference -- one test per
place a quantizer lives:

  ce_gpu_quantize               kernels/quant.hip, the division
  the first-layer quantize pass quantize_row, vector (width 40) and scalar (13)
  quantize_fast_kernel          a hidden Linear 192 wide
  i8_epilogue_q                 a hidden Linear 256 wide (the requantize epilogue)
  the latency pair's reduce     the same net on a latency context
  dynamic int8                  the same carriers, the block's own min / max

The hidden quantizers are reached through the bias: Linear A reads rows of
0.0 with a frozen range around 0, so its bytes are its zero point, its
accumulator is 0 and y == bias exactly -- the bias holds the tie inputs of
Linear B's range.  B has real-valued weights and no bias, so every byte of
its input moves its output.

The ranges [0, 7.6e-37] .. [0, 2.4e-35] have scales whose reciprocal is finite
while the reciprocal product's remainder underflows: the product without
qbyte_rscale's threshold misses bytes there (test_quantties.py).
"""
import functools

import numpy as np
import pytest

import i8ref
import netgen
import quantties as qt
from test_gpu_parity import bits, dev
from test_int8_static import FLT_MIN, static_oracle

pytestmark = pytest.mark.gpu

N_RANGES = 18
ROWS = 9            # three blocks of four rows per block, the last ragged
A_RANGE = (-1.0, 1.0)   # Linear A's frozen range: scale 2 / 255, zero point 128


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
    return G.Context(0)


@pytest.fixture(scope="module")
def lctx(torch, G):
    c = G.Context(0)
    c.set_latency(True)
    return c


def the_range(oracle, i):
    ranges = qt.all_ranges(oracle)
    assert len(ranges) == N_RANGES
    return ranges[i][1]


def diff(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    a, b = (got, want) if got.dtype == np.uint8 else (bits(got), bits(want))
    bad = np.argwhere(a != b)
    if not len(bad):
        return None
    at = tuple(bad[0])
    return f"{len(bad)} of {got.size} differ, first at {at}: got {got[at]!r}, want {want[at]!r}"


def real_linear(k, n, seed, bias=None):
    """netgen.real_net's weights; no bias unless given."""
    from catears_amd import synth
    W = (synth.uniform(seed, k * n, -1.0, 1.0) * np.sqrt(3.0 / k)).astype(np.float32).reshape(k, n)
    return {"kind": "linear", "W": W, "b": np.zeros(n, np.float32) if bias is None else np.asarray(bias, np.float32)}


def assert_every_byte_reaches_the_output(oracle, linear, xq, s, z):
    """One column of the Linear's quantized weights differs from the weight
    zero point in every row, so a change of any input byte changes that
    column's accumulator; with no bias the output is float(acc) * (s * sw),
    which distinct accumulators below 2^22 do not share (neighbouring
    integers there are more than a float32 spacing apart, before and after
    the product)."""
    wq, sw, zw = oracle.quantize(linear["W"])
    w = wq.astype(np.int64) - zw
    clean = np.flatnonzero((w != 0).all(axis=0))
    assert len(clean) and not linear["b"].any()
    acc = (xq.astype(np.int64) - z) @ w[:, clean]
    assert np.abs(acc).max() < 2 ** 22 and np.float32(s) * np.float32(sw) > 0


def static(G, ctx, layers, ranges):
    return G.Model(ctx, image=netgen.image(layers)).quantize_static(ctx, np.asarray(ranges, np.float32))


# ------------------------------------------------------------ ce_gpu_quantize --

@pytest.mark.parametrize("i", range(N_RANGES))
def test_ce_gpu_quantize_on_ties(torch, G, ctx, oracle, i):
    """The tensor [mn, mx, tie inputs inside the range]: its own extremes
    reproduce the range's parameters; bytes and parameters are the oracle's."""
    mn, mx = the_range(oracle, i)
    ties, sens, scale, zp = qt.tie_inputs(oracle, mn, mx)
    inside = (ties >= np.float32(mn)) & (ties <= max(np.float32(mx), FLT_MIN))
    assert (sens & inside).sum() >= 200
    x = np.concatenate([np.float32([mn, mx]), ties[inside]])
    want, s, z = oracle.quantize(x)
    assert np.float32(s) == scale and z == zp
    q, prm = G.quantize(ctx, dev(torch, x))
    gs, gz = G.params_host(prm)
    assert np.float32(gs).view(np.uint32) == scale.view(np.uint32) and gz == zp, (gs, gz, scale, zp)
    assert diff(q.cpu().numpy(), want) is None, diff(q.cpu().numpy(), want)


# -------------------------------------------------- the first-layer pass ----

@functools.lru_cache(maxsize=None)
def first_layer_net(width):
    layers = [{"kind": "splice", "indices": [-1, 0, 1]}, {"kind": "narrow", "left": 1, "right": 1},
              real_linear(3 * width, 64, 8100 + width)]
    return layers


@pytest.mark.parametrize("width", [40, 13])
@pytest.mark.parametrize("i", range(N_RANGES))
def test_first_layer_quantize_pass_on_ties(torch, G, ctx, oracle, i, width):
    """quantize_row's vector (width 40) and scalar (width 13) forms: the input
    rows carry all the tie inputs, clamp values included, spliced over three
    rows; Linear 0's frozen range is the range."""
    mn, mx = the_range(oracle, i)
    ties, sens, scale, zp = qt.tie_inputs(oracle, mn, mx)
    layers = first_layer_net(width)
    rows = -(-len(ties) // width)
    assert rows <= 300
    x = np.resize(ties, rows * width).reshape(rows, width)
    want_path = "general-vector" if width == 40 else "general-scalar"
    assert i8ref.paths(layers, rows - 2, "static")[0]["quantize"] == want_path
    taps = []
    want = static_oracle(oracle, layers, x, [(mn, mx)], taps)
    spliced = oracle.layer_forward(layers[1], oracle.layer_forward(layers[0], x))
    assert spliced.shape == (rows - 2, 3 * width)
    assert set(bits(spliced).reshape(-1).tolist()) == set(bits(ties).tolist())
    assert np.array_equal(taps[0], oracle._quantize_with(spliced, scale, zp))
    assert_every_byte_reaches_the_output(oracle, layers[2], taps[0], scale, zp)
    model = static(G, ctx, layers, [(mn, mx)])
    got = G.nnet_propagate(ctx, model, dev(torch, x)).cpu().numpy()
    assert diff(got, want) is None, diff(got, want)


# ------------------------------------------ hidden layers, through the bias --

def carrier_values(oracle, mn, mx, inside_only=False):
    """The range's sensitive tie inputs and its clamp values; inside_only:
    those a block may hold without moving its own min / max off the range."""
    ties, sens, _, _ = qt.tie_inputs(oracle, mn, mx)
    keep = sens.copy()
    keep[-8:] = True
    if inside_only:
        keep &= (ties >= np.float32(mn)) & (ties <= max(np.float32(mx), FLT_MIN))
    assert (keep & sens).sum() >= 200
    return ties[keep]


def carriers(values, width, seed, head=()):
    """[layers]: Linear A (40 -> width, no post-ops, bias = `head` + a slice
    of `values`, the last slice wrapping around) then Linear B (width -> 64,
    real weights, no bias), as many nets as hold all the values."""
    room = width - len(head)
    out = []
    for at in range(0, len(values), room):
        bias = np.concatenate([np.float32(list(head)), np.resize(values[at:], room) if at + room > len(values)
                               else values[at:at + room]]).astype(np.float32)
        assert len(bias) == width
        out.append([real_linear(40, width, seed), real_linear(width, 64, seed + 1, bias=None)])
        out[-1][0]["b"] = bias
    return out


def check_static_carrier(torch, G, c, oracle, layers, rng, latency=False):
    """One carrier net on context c against static_oracle; returns B's bytes."""
    x = np.zeros((ROWS, 40), np.float32)
    ranges = [A_RANGE, rng]
    scale, zp = qt.params(oracle, *rng)
    _, sa, za = oracle.quantize(np.float32(A_RANGE))
    assert 0 <= za <= 255
    # the oracle side: A's bytes are its zero point, so y == bias exactly
    taps = []
    want = static_oracle(oracle, layers, x, ranges, taps)
    assert (taps[0] == za).all()
    y = static_oracle(oracle, layers[:1], x, ranges[:1])
    assert np.array_equal(bits(y), bits(np.broadcast_to(layers[0]["b"], y.shape)))
    assert np.array_equal(taps[1], np.broadcast_to(oracle._quantize_with(layers[0]["b"], scale, zp), taps[1].shape))
    assert_every_byte_reaches_the_output(oracle, layers[1], taps[1], scale, zp)
    model = static(G, c, layers, ranges)
    before = G.debug_i8_latency_launches()
    got = G.nnet_propagate(c, model, dev(torch, x)).cpu().numpy()
    launched = G.debug_i8_latency_launches() - before
    if latency:
        plan = [G.i8_latency_plan((L["W"].shape[0] + 127) // 128 * 128, L["W"].shape[1], ROWS)[0] for L in layers]
        assert ROWS <= i8ref.LAT_MAX_ROWS and plan[0] > 0 and launched == sum(s > 0 for s in plan), (plan, launched)
    else:
        assert launched == 0
    assert diff(got, want) is None, diff(got, want)
    return taps[1]


@pytest.mark.parametrize("i", range(N_RANGES))
def test_quantize_fast_kernel_on_ties(torch, G, ctx, oracle, i):
    """Width 192 is no multiple of 128: A's epilogue writes fp32 and B takes
    the quantize pass, one segment of float4 rows: quantize_fast_kernel."""
    mn, mx = the_range(oracle, i)
    seen = set()
    for layers in carriers(carrier_values(oracle, mn, mx), 192, 8200):
        p = i8ref.paths(layers, ROWS, "static")
        assert p[0]["epilogue"] != "requantize" and p[1]["quantize"] == "fast"
        seen |= set(check_static_carrier(torch, G, ctx, oracle, layers, (mn, mx)).reshape(-1).tolist())
    assert len(seen) >= 128


@pytest.mark.parametrize("i", range(N_RANGES))
def test_requantize_epilogue_on_ties(torch, G, ctx, lctx, oracle, i):
    """Width 256: A's epilogue quantizes with B's frozen parameters
    (i8_epilogue_q) and no quantize pass runs for B; on the latency context
    the split-K pair's reduce does the same."""
    mn, mx = the_range(oracle, i)
    for layers in carriers(carrier_values(oracle, mn, mx), 256, 8300):
        for form in ("static", "static-latency"):
            p = i8ref.paths(layers, ROWS, form)
            assert p[0]["epilogue"] == "requantize" and p[1]["quantize"] == "none"
        assert p[0]["slices"][0] > 0
        check_static_carrier(torch, G, ctx, oracle, layers, (mn, mx))
        check_static_carrier(torch, G, lctx, oracle, layers, (mn, mx), latency=True)


@pytest.mark.parametrize("width", [192, 256])
@pytest.mark.parametrize("i", range(N_RANGES))
def test_dynamic_int8_on_ties(torch, G, ctx, oracle, i, width):
    """ce_gpu_model_quantize on the carriers: two bias columns hold mn and mx,
    so B's own min / max reproduces the range; A's input is all 0.0, its range
    [0, FLT_MIN], its bytes and zero point 0."""
    mn, mx = the_range(oracle, i)
    scale, zp = qt.params(oracle, mn, mx)
    x = np.zeros((ROWS, 40), np.float32)
    for layers in carriers(carrier_values(oracle, mn, mx, inside_only=True), width, 8400 + width, head=(mn, mx)):
        assert [p["quantize"] for p in i8ref.paths(layers, ROWS, "dynamic")] == ["fast", "fast"]
        (ya,), _, (pa,) = i8ref.chunk_reference(oracle, layers[:1], [x])
        assert pa[1] == 0 and np.array_equal(bits(ya), bits(np.broadcast_to(layers[0]["b"], ya.shape)))
        (want,), _, params = i8ref.chunk_reference(oracle, layers, [x])
        assert np.float32(params[1][0]) == scale and params[1][1] == zp
        assert_every_byte_reaches_the_output(oracle, layers[1], oracle._quantize_with(ya, scale, zp), scale, zp)
        model = G.Model(ctx, image=netgen.image(layers)).quantize(ctx)
        got = G.nnet_propagate(ctx, model, dev(torch, x)).cpu().numpy()
        assert diff(got, want) is None, diff(got, want)
