"""The nnet GEMMs off the two TDNN shapes (tests/netgen.py has the nets and
the reasoning; tests/test_netgen.py proves the oracle side on the CPU).

Exact-integer leg: nets whose every fp32 summation order gives the same
integers, so each kernel family -- gemm_f32, the bf16x6 direct-weight kernels
on 128 x 128, 256 x 128 and 512 x 128 tiles, the plane kernels, the split-K
latency kernels with their reduce / fused finalize -- must reproduce
netgen.exact bit for bit: odd K-tile counts, one K-tile, ragged unit tiles,
first-layer widths 24 / 13, 8 asymmetric splice segments, uneven latency
slices, n > 4096, every PostMode, the fp32 fallback program.  No tolerance.

Real-valued leg: the same geometries with variance-preserving float weights
against an fp64 evaluation at the project's bars, the bf16x6 schedules
bit-identical to each other, and every mode invariant to the row block a row
is scored in."""
import functools

import numpy as np
import pytest

import netgen
from test_gpu_parity import LOGLIK_TOL, bits, dev

pytestmark = pytest.mark.gpu

# mode -> (context flavour, ce_gpu_model_set_gemm mode)
MODES = {"fp32": ("plain", "fp32"), "bf16x6": ("plain", "bf16x6"), "bf16x6p": ("plain", "bf16x6p"),
         "wide": ("wide", "bf16x6"), "latency": ("latency", "bf16x6")}
SPLIT_MODES = ("bf16x6", "bf16x6p", "wide", "latency")
EXACT_GEOMS = [g for g in sorted(netgen.GEOMETRIES) if g != "B2"]
REAL_GEOMS = ["A", "C", "F4100", "F4099", "G9", "G25", "G20"]


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


def load(G, ctxs, layers, mode, prior=None):
    """(ctx, model) of `layers` in `mode`.  A net outside the bf16x6 program's
    envelope runs the fp32 program and says so: it loads as "fp32" and
    refuses every split mode."""
    flavour, gemm = MODES[mode]
    ctx = ctxs[flavour]
    model = G.Model(ctx, image=netgen.image(layers), prior=prior)
    assert (model.left, model.right) == netgen.context(layers)
    if netgen.x6_ok(layers):
        assert model.gemm == "bf16x6"
        model.set_gemm(gemm)
        assert model.gemm == gemm
    else:
        assert model.gemm == "fp32"
        if gemm != "fp32":
            with pytest.raises(G.CatearsError, match="ENOTSUP"):
                model.set_gemm(gemm)
        assert model.gemm == "fp32"
    return ctx, model


def first_diff(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    bad = np.argwhere(bits(got) != bits(want))
    if not len(bad):
        return None
    r, c = bad[0]
    return (f"{len(bad)} of {got.size} differ, first at (row {r}, col {c}): got {got[r, c]!r}, want {want[r, c]!r}; "
            f"rows {np.unique(bad[:, 0])[:8].tolist()}.., cols {np.unique(bad[:, 1])[:8].tolist()}..")


@functools.lru_cache(maxsize=None)
def exact_cases(geom, form="bf16x6"):
    """[(name, layers, x, want)], checked against the budget once."""
    out = []
    for name, layers, x in netgen.exact_cases(geom, form):
        if "*2^" not in name:
            netgen.check_exact_budget(layers, x, form)
            if geom == "B2":
                netgen.check_exact_budget(layers, x, "f16x3")
        want = netgen.exact(layers, x)
        want.setflags(write=False)
        out.append((name, layers, x, want))
    return out


# ------------------------------------------------------ exact-integer leg --

@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("geom", EXACT_GEOMS)
def test_exact_integer_nets(torch, G, ctxs, geom, mode):
    """Every case of netgen.exact_cases: WIDE, TWO_PLANES, the plane recipes
    (W3@p, A3, P11@p: every plane product the bf16x6 kernels keep, nonzero at
    every position of every kernel family -- the matrix and the mutation
    proofs are in tests/test_netgen.py) and the binade-shifted forms."""
    failures = []
    for name, layers, x, want in exact_cases(geom):
        ctx, model = load(G, ctxs, layers, mode)
        ctx_rows = model.left + model.right
        for r in netgen.case_rows(geom, name):
            got = G.nnet_propagate(ctx, model, dev(torch, x[:r + ctx_rows])).cpu().numpy()
            d = first_diff(got, want[:r])
            if d:
                failures.append(f"{geom} {name} {mode} rows={r} {netgen.kernels(layers, r, mode)}: {d}")
    assert not failures, "\n".join(failures)


F16_CASES = [(g, name) for g in sorted(netgen.GEOMETRIES)
             for name in (["wide"] if g == "B2" else []) + netgen.recipe_names(g, "f16x3")]


@pytest.fixture(scope="module")
def f16_ctx(torch, G):
    return G.Context(0)


@pytest.mark.parametrize("geom,name", F16_CASES)
def test_exact_integer_f16x3(torch, G, f16_ctx, geom, name):
    """f16x3 drops the a1b1 product: exact while, per Linear, one operand
    fits one fp16 plane (|v| <= 2047) and two planes hold every operand and
    hidden output (check_exact_budget's f16x3 form).  B2's WIDE net and F1
    keep every operand in one plane (a0b0 alone); FX puts two-plane
    activations on one-plane weights at the first and the later Linears
    (a1b0: the second accumulator, the epilogue's 2^-11 recombination, the
    split of the hidden outputs), FW@p two-plane weights on one-plane
    activations (a0b1).  Spliced first and hidden layers, K-tiles of 32 and
    of 64.  Its range is limited, so no binade-shifted form."""
    ctx = f16_ctx
    assert not ctx.overflow()
    (layers, x, want), = [c[1:] for c in exact_cases(geom, "f16x3") if c[0] == name]
    model = G.Model(ctx, image=netgen.image(layers)).set_gemm("f16x3")
    assert model.gemm == "f16x3"
    assert netgen.case_rows(geom, name) == netgen.ROWS
    for r in netgen.ROWS:
        got = G.nnet_propagate(ctx, model, dev(torch, x[:r + model.left + model.right])).cpu().numpy()
        assert first_diff(got, want[:r]) is None, f"rows={r} {netgen.f16x3_kernels(layers)}: {first_diff(got, want[:r])}"
    assert not ctx.overflow()


def test_launch_classes_follow_the_first_layer_path(torch, G):
    """The profile classes confirm the first-layer paths the geometries are
    there for: A's 40-wide segments are gathered in the GEMM's loader (no
    launch before it), D's 13-wide ones go through splice_pad, the plane
    program always writes the spliced planes first, and E (the fp32 program,
    segments of 100) pads every layer."""
    ctx = G.Context(0)
    ctx.profile(True)

    def launches(geom, gemm):
        _, layers, x, _ = exact_cases(geom)[0]
        model = G.Model(ctx, image=netgen.image(layers))
        if netgen.x6_ok(layers):
            model.set_gemm(gemm)
        G.nnet_propagate(ctx, model, dev(torch, x[:70 + model.left + model.right]))
        return ctx.profile_read(ctx.PROF_GEMM_GATHER)[1], ctx.profile_read(ctx.PROF_GEMM)[1]

    assert launches("A", "bf16x6") == (0, 3)
    assert launches("A", "bf16x6p") == (1, 3)
    assert launches("C", "bf16x6") == (0, 3)
    assert launches("D", "bf16x6") == (1, 3)
    assert launches("E", "bf16x6") == (3, 0)
    assert launches("F4099", "bf16x6") == (1, 2)
    ctx.profile(False)


# -------------------------------------------------------- real-valued leg --

@functools.lru_cache(maxsize=None)
def real_case(geom, rows):
    in_d, widths, splices, post = netgen.GEOMETRIES[geom]
    seed = 2000 + sorted(netgen.GEOMETRIES).index(geom)
    layers = netgen.real_net(in_d, widths, splices, post, seed)
    x = netgen.real_input(layers, rows, seed + 500)
    return layers, x


@functools.lru_cache(maxsize=None)
def real_reference(geom, rows, with_prior):
    layers, x = real_case(geom, rows)
    want = netgen.eval_f64(layers, x)
    if with_prior:
        want = want - np.log(netgen.prior(want.shape[1], 77).astype(np.float64))
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("geom", REAL_GEOMS)
def test_real_nets_vs_fp64(torch, G, ctxs, geom):
    """Ending in LogSoftmax every mode is within LOGLIK_TOL of the fp64
    evaluation and the split modes' error is of the fp32 mode's size (the
    bars of test_split_gemms_are_fp32_accurate); the bf16x6 schedules --
    fp32 operands, planes, 128 x 128 tiles -- give one set of bits."""
    rows = netgen.max_rows(geom)
    layers, x = real_case(geom, rows)
    want = real_reference(geom, rows, False)
    errs, outs = {}, {}
    for mode in MODES:
        ctx, model = load(G, ctxs, layers, mode)
        outs[mode] = G.nnet_propagate(ctx, model, dev(torch, x)).cpu().numpy()
        assert outs[mode].shape == want.shape
        errs[mode] = float(np.abs(outs[mode] - want).max())
    print(geom, errs)
    for mode in MODES:
        assert errs[mode] <= LOGLIK_TOL, errs
    for mode in SPLIT_MODES:
        assert errs[mode] <= max(2.0 * errs["fp32"], 2e-5), errs
    assert first_diff(outs["bf16x6p"], outs["bf16x6"]) is None, first_diff(outs["bf16x6p"], outs["bf16x6"])
    assert first_diff(outs["wide"], outs["bf16x6"]) is None, first_diff(outs["wide"], outs["bf16x6"])


BLOCKS = [70, 33, 151]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("geom", REAL_GEOMS)
def test_row_block_invariance(torch, G, ctxs, geom, mode):
    """A row's bits do not depend on the block it is scored in: rows [0, 70)
    of a 3000-row block scored alone, and blocks of 70, 33 and 151 rows
    through nnet_propagate_blocks, carry the big block's bits -- across the
    kernel switch at 48 tiles, and in latency mode across its 1024-row
    windows, its row tiles and the fused / unfused last reduce."""
    layers, x = real_case(geom, netgen.BIG_ROWS)
    ctx, model = load(G, ctxs, layers, mode)
    c = model.left + model.right
    big = G.nnet_propagate(ctx, model, dev(torch, x)).cpu().numpy()
    assert big.shape == (netgen.BIG_ROWS, netgen.GEOMETRIES[geom][1][-1]) and np.all(np.isfinite(big))
    alone = G.nnet_propagate(ctx, model, dev(torch, x[:70 + c])).cpu().numpy()
    assert first_diff(alone, big[:70]) is None, first_diff(alone, big[:70])
    # one row more: the other parity of the row count (workspace offsets)
    again = G.nnet_propagate(ctx, model, dev(torch, x[:71 + c])).cpu().numpy()
    assert first_diff(again[:70], alone) is None, first_diff(again[:70], alone)
    starts = np.concatenate([[0], np.cumsum(BLOCKS)])
    packed = np.concatenate([x[s:s + n + c] for s, n in zip(starts, BLOCKS)])
    blocks = G.nnet_propagate_blocks(ctx, model, dev(torch, packed), [n + c for n in BLOCKS]).cpu().numpy()
    assert first_diff(blocks, big[:sum(BLOCKS)]) is None, first_diff(blocks, big[:sum(BLOCKS)])


# ------------------------------------------------------------ finalize (F) --

@pytest.mark.parametrize("geom", ["F4100", "F4099"])
def test_finalize_beyond_4096(torch, G, ctxs, geom):
    """LogSoftmax and the prior subtraction at n > 4096 (launch_finalize's
    strided loop; in latency mode after the unfused lat_reduce): within 1e-4
    of the fp64 x - logsumexp(x) - log prior, at every row count, in every
    mode (4099 is the fp32 program)."""
    rows = netgen.ROWS[-1]
    layers, x = real_case(geom, rows)
    want = real_reference(geom, rows, True)
    prior = netgen.prior(want.shape[1], 77)
    assert netgen.finalize_path(want.shape[1]) == "loop"
    errs = {}
    for mode in MODES:
        ctx, model = load(G, ctxs, layers, mode, prior=prior)
        c = model.left + model.right
        for r in netgen.ROWS:
            got = G.nnet_propagate(ctx, model, dev(torch, x[:r + c]), subtract_prior=True).cpu().numpy()
            assert got.shape == (r, want.shape[1])
            errs[mode, r] = float(np.abs(got - want[:r]).max())
    print(geom, errs)
    assert max(errs.values()) <= 1e-4, errs
