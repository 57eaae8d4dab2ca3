"""The C-ABI's entry points on caller-shaped buffers: strided rows, bases that
are only 4-byte aligned, outputs laid into the middle of a larger allocation.

include/catears_gpu.h asks for no alignment of any device pointer and for no
more of a leading dimension than ld >= width.  Behind the entries almost every
kernel has a fast form for 16-byte aligned rows and a second branch for the
rest, chosen at launch time from the pointer's low bits and ld % 4; every
other GPU test passes dense, freshly allocated tensors and so only ever takes
the first.  Here each entry runs on the layouts of LAYOUTS, given as (ld -
width, lead) in elements.

placed() lays an input into a poisoned allocation: NaN (a stray read times a
zero weight is still NaN) or alternating +-3.0e38 (a min / max scan ignores a
NaN, only a finite outlier moves a range).  At least TAIL poison elements
follow the last row, so a kernel that reads past it meets poison inside the
allocation -- a failed assertion, never a fault.  Outputs lie in a buffer of
one sentinel word, and every sentinel outside the output's own elements --
before its base, in its gap columns, behind it -- must keep its bits.

Everything is bit for bit against the CPU references the dense tests use; only
the LogSoftmax / row-op cases are held to the project's LOGLIK_TOL against
float64."""
import functools

import numpy as np
import pytest

import i8ref
import netgen
from test_gpu_gemm_shapes import MODES, exact_cases, first_diff, load, real_case, real_reference
from test_gpu_parity import LOGLIK_TOL, bits, dev
from test_int8_static import fp32_ranges, static_oracle

pytestmark = pytest.mark.gpu

TAIL = 4096               # poison / sentinel elements behind the last row
SENTINEL = 0x7fc0dead     # every output buffer's fill, one 32-bit word
SENTINEL_BYTE = 0xa5
# (ld - width, lead): dense and aligned (the control); base 4 bytes off; odd
# stride (every row another alignment); aligned with a gap (a fast path must
# not read it); base 8-byte aligned only; misaligned base and odd stride
LAYOUTS = [(0, 0), (0, 1), (1, 0), (4, 0), (4, 2), (3, 2)]
ALIGNED = [(0, 0), (4, 0)]
POISONS = ("nan", "huge")
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
    c = {"plain": G.Context(0), "wide": G.Context(0), "latency": G.Context(0)}
    c["wide"].set_wide_tiles(True)
    c["latency"].set_latency(True)
    return c


# ------------------------------------------------------------ the buffers --

def poison_values(poison, n):
    if poison == "nan":
        return np.full(n, np.nan, np.float32)
    assert poison == "huge", poison
    v = np.full(n, 3.0e38, np.float32)
    v[1::2] = -3.0e38
    return v


def upload(torch, host):
    """A fresh device allocation holding `host` (256-byte aligned base)."""
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 256 == 0
    return t


def placed(torch, x, ld, lead, poison):
    """x (rows, width) at element `lead` of a poisoned flat buffer of lead +
    rows * ld + TAIL elements, rows ld apart: the strided view of it."""
    x = np.ascontiguousarray(x, np.float32)
    rows, width = x.shape
    assert ld >= width and lead >= 0
    host = poison_values(poison, lead + rows * ld + TAIL)
    np.lib.stride_tricks.as_strided(host[lead:], (rows, width), (4 * ld, 4))[:] = x
    return upload(torch, host).as_strided((rows, width), (ld, 1), lead)


def placed_flat(torch, v, lead, poison="nan"):
    """A vector at element `lead` of a poisoned buffer."""
    v = np.ascontiguousarray(v, np.float32).ravel()
    host = poison_values(poison, lead + v.size + TAIL)
    host[lead:lead + v.size] = v
    return upload(torch, host)[lead:lead + v.size]


class Out:
    """A (rows, width) float32 (or int32) output at element `lead` of a buffer
    of SENTINEL words, rows ld apart.  `init`: values the rows hold before the
    call (an in-place operand)."""

    def __init__(self, torch, rows, width, ld, lead, dtype=None, init=None):
        assert ld >= width
        self.rows, self.width, self.ld, self.lead = rows, width, ld, lead
        host = np.full(lead + rows * ld + TAIL, SENTINEL, np.uint32)
        self.own = np.zeros(host.size, bool)
        np.lib.stride_tricks.as_strided(self.own[lead:], (rows, width), (ld, 1))[:] = True
        if init is not None:
            host[self.own] = np.ascontiguousarray(init, np.float32).view(np.uint32).ravel()
        self.base = upload(torch, host.view(np.int32))
        self.view = self.base.view(dtype or torch.float32).as_strided((rows, width), (ld, 1), lead)

    def read(self):
        """(the output rows as uint32 words, None or what is wrong with the
        sentinels)."""
        host = self.base.cpu().numpy().view(np.uint32)
        bad = np.flatnonzero((host != SENTINEL) & ~self.own)
        msg = None
        if len(bad):
            msg = (f"{len(bad)} sentinel words overwritten, first at element {bad[0]} (output: lead {self.lead}, "
                   f"{self.rows} rows of {self.width} at stride {self.ld})")
        return host[self.own].reshape(self.rows, self.width), msg

    def diff(self, want):
        """None, or how the output differs from `want` (bit for bit) or which
        sentinels are gone."""
        got, msg = self.read()
        want = np.ascontiguousarray(want)
        if want.dtype != np.float32:
            want = want.view(np.float32)      # 32-bit words of another type
        return msg or first_diff(got.view(np.float32), want)


def test_placed_and_out_lay_out_what_they_say(torch):
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    for poison in POISONS:
        v = placed(torch, x, 7, 2, poison)
        assert (v.stride(0), v.stride(1), v.storage_offset(), v.data_ptr() % 16) == (7, 1, 2, 8)
        assert np.array_equal(v.cpu().numpy(), x)
        flat = torch.as_strided(v, (2 + 3 * 7 + TAIL,), (1,), 0).cpu().numpy()
        own = np.zeros(flat.size, bool)
        for r in range(3):
            own[2 + 7 * r:2 + 7 * r + 4] = True
        assert np.array_equal(bits(flat[~own]), bits(poison_values(poison, flat.size)[~own]))
        assert np.isnan(flat[~own]).all() if poison == "nan" else (np.abs(flat[~own]) == np.float32(3.0e38)).all()
    o = Out(torch, 3, 4, 5, 1)
    assert o.view.data_ptr() % 16 == 4 and o.diff(np.full((3, 4), SENTINEL, np.uint32)) is None
    o.view.copy_(dev(torch, x))
    assert o.diff(x) is None
    o.base[0] = 0
    assert "sentinel" in o.diff(x)
    o = Out(torch, 3, 4, 5, 1)
    o.base[1 + 4] = 0      # the first gap column
    assert "sentinel" in o.diff(np.full((3, 4), SENTINEL, np.uint32))


# ------------------------------------------------- 4. nnet_propagate, exact --

def sweep(torch, G, ctx, model, cases, label, layouts=LAYOUTS, poisons=POISONS, **kw):
    """nnet_propagate on every layout x poison of every (x, want) in `cases`,
    the dense output at lead 0 and 1: the list of failures."""
    failures = []
    for x, want in cases:
        for gap, lead in layouts:
            for poison in poisons:
                xin = placed(torch, x, x.shape[1] + gap, lead, poison)
                for out_lead in (0, 1):
                    out = Out(torch, want.shape[0], want.shape[1], want.shape[1], out_lead)
                    G.nnet_propagate(ctx, model, xin, out=out.view, **kw)
                    d = out.diff(want)
                    if d:
                        failures.append(f"{label} rows={want.shape[0]} ld-width={gap} lead={lead} {poison} "
                                        f"out lead={out_lead}: {d}")
    return failures


def row_cases(x, want, ctx_rows, rows=netgen.ROWS):
    return [(x[:r + ctx_rows], want[:r]) for r in rows]


NNET_GEOMS = ["A", "B", "C", "D", "E", "H", "F4099"]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("geom", NNET_GEOMS)
def test_exact_nets(torch, G, ctxs, geom, mode):
    """fp32 (splice_pad, the LDS-DMA kernel or pipe2 on the caller's rows),
    bf16x6 and latency (the loaders' gather or splice_pad), the plane program
    (splice_pad_split), the fp32 fallback program (E, F4099).  The WIDE case
    of each geometry: what a buffer's layout can break is the loaders'
    addressing, which does not depend on the operands' planes; the plane
    recipes (W3, A3, P11) and the binade-shifted forms of netgen.exact_cases
    are left to tests/test_gpu_gemm_shapes.py."""
    name, layers, x, want = exact_cases(geom)[0]
    assert name == "wide"
    ctx, model = load(G, ctxs, layers, mode)
    failures = sweep(torch, G, ctx, model, row_cases(x, want, model.left + model.right), f"{geom} {name} {mode}")
    assert not failures, "\n".join(failures[:20])


def test_exact_f16x3(torch, G):
    """B2's WIDE case; the f16x3 plane recipes (F1, FX, FW) are left to
    tests/test_gpu_gemm_shapes.py."""
    ctx = G.Context(0)
    (name, layers, x, want), = exact_cases("B2")
    model = G.Model(ctx, image=netgen.image(layers)).set_gemm("f16x3")
    failures = sweep(torch, G, ctx, model, row_cases(x, want, model.left + model.right), "B2 f16x3")
    assert not failures, "\n".join(failures[:20])
    assert not ctx.overflow()


@pytest.mark.parametrize("geom", ["A", "C", "D", "H"])
def test_exact_bf16(torch, G, ctxs, geom):
    """Plain bf16 (splice_pad_bf16 reads the caller's rows) against its fp64
    walk, which equals its every evaluation order on these cases."""
    import test_gpu_gemm_bf16 as tb
    failures = []
    for name, layers, x, want in tb.exact_cases(geom):
        model = tb.bf16_model(G, ctxs["plain"], layers)
        failures += sweep(torch, G, ctxs["plain"], model, row_cases(x, want, model.left + model.right),
                          f"{geom} {name} bf16")
    assert not failures, "\n".join(failures[:20])


# ---------------------------------------------------------------- 4. int8 --

# I5: a row op between two Linears, so the Linear behind it takes the
# stand-alone min / max and quantize passes (no fused partials)
I8_GEOMS = ["A", "C", "E", "H", "I5"]


@functools.lru_cache(maxsize=None)
def i8_ranges(geom):
    from oracle import pyoracle
    return fp32_ranges(pyoracle, i8ref.net(geom), i8ref.calibration_input(geom))


@functools.lru_cache(maxsize=None)
def static_reference(geom, rows):
    from oracle import pyoracle
    x = i8ref.block_input(geom, rows)
    want = static_oracle(pyoracle, i8ref.net(geom), x, i8_ranges(geom))
    want.setflags(write=False)
    return x, want


@pytest.mark.parametrize("geom", I8_GEOMS)
def test_dynamic_int8(torch, G, ctxs, oracle, geom):
    """The first Linear's range is a reduction over the caller's rows
    (minmax_kernel): one gap element of the `huge` poison folded into it would
    change every byte.  Then the quantize pass reads the same rows."""
    layers = i8ref.net(geom)
    ctx = ctxs["plain"]
    model = G.Model(ctx, image=netgen.image(layers)).quantize(ctx)
    assert any(p["minmax"] != "fused" for p in i8ref.paths(layers, 70, "dynamic")[1:]) == (geom == "I5")
    failures = sweep(torch, G, ctx, model, [i8ref.reference(oracle, geom, r) for r in netgen.ROWS], f"{geom} dynamic")
    assert not failures, "\n".join(failures[:20])


@pytest.mark.parametrize("flavour", ["plain", "latency"])
@pytest.mark.parametrize("geom", I8_GEOMS)
def test_static_int8(torch, G, ctxs, oracle, geom, flavour):
    ctx = ctxs[flavour]
    model = G.Model(ctx, image=netgen.image(i8ref.net(geom))).quantize_static(ctx, i8_ranges(geom))
    failures = sweep(torch, G, ctx, model, [static_reference(geom, r) for r in netgen.ROWS],
                     f"{geom} static {flavour}")
    assert not failures, "\n".join(failures[:20])


# -------------------------------------------------------------- 4. blocks --

@pytest.mark.parametrize("mode", ["bf16x6", "latency", "static"])
@pytest.mark.parametrize("geom", ["A", "H"])
def test_propagate_blocks(torch, G, ctxs, oracle, geom, mode):
    """Blocks of 70 / 33 / 151 output rows back to back at stride ld: every
    block's rows equal that block scored by the reference alone."""
    if mode == "static":
        layers, ctx = i8ref.net(geom), ctxs["plain"]
        model = G.Model(ctx, image=netgen.image(layers)).quantize_static(ctx, i8_ranges(geom))
        c = sum(netgen.context(layers))
        x = i8ref.block_input(geom, sum(BLOCKS))
        ref = lambda b: static_oracle(oracle, layers, b, i8_ranges(geom))
    else:
        _, layers, x, _ = exact_cases(geom)[0]
        ctx, model = load(G, ctxs, layers, mode)
        c = sum(netgen.context(layers))
        ref = lambda b: netgen.exact(layers, b)
    starts = np.concatenate([[0], np.cumsum(BLOCKS)])
    blocks = [x[s:s + n + c] for s, n in zip(starts, BLOCKS)]
    want = np.concatenate([ref(b) for b in blocks])
    packed = np.concatenate(blocks)
    failures = []
    for gap, lead in LAYOUTS:
        for poison in POISONS:
            xin = placed(torch, packed, packed.shape[1] + gap, lead, poison)
            for out_lead in (0, 1):
                out = Out(torch, want.shape[0], want.shape[1], want.shape[1], out_lead)
                G.nnet_propagate_blocks(ctx, model, xin, [len(b) for b in blocks], out=out.view)
                d = out.diff(want)
                if d:
                    failures.append(f"{geom} {mode} ld-width={gap} lead={lead} {poison} out lead={out_lead}: {d}")
    assert not failures, "\n".join(failures[:20])


# ------------------------------------------------------ 4. the window seam --

@functools.lru_cache(maxsize=None)
def seam_case():
    _, layers, _, _ = exact_cases("B")[0]
    x = netgen.int_input(layers, (1 << 16) + 4000, seed=4242)
    netgen.check_exact_budget(layers, x)
    want = netgen.exact(layers, x)
    want.setflags(write=False)
    return layers, x, want


@pytest.mark.parametrize("mode", ["fp32", "bf16x6"])
def test_window_seam(torch, G, ctxs, mode):
    """65 536 + 4 000 rows run as two windows, the second from d_in + o *
    ld_in: with ld_in = 41 that base has another alignment than the first,
    with lead = 1 both are off."""
    layers, x, want = seam_case()
    ctx, model = load(G, ctxs, layers, mode)
    assert model.left + model.right == 0 and len(x) > (1 << 16)
    for gap, lead in ((1, 0), (0, 1)):
        xin = placed(torch, x, x.shape[1] + gap, lead, "nan")
        out = Out(torch, want.shape[0], want.shape[1], want.shape[1], 0)
        G.nnet_propagate(ctx, model, xin, out=out.view)
        d = out.diff(want)
        assert d is None, f"B {mode} ld-width={gap} lead={lead}: {d}"


# ------------------------------------------- 4. calibrate and am_forward --

def int_net_of(geom):
    in_d, widths, splices, post = netgen.GEOMETRIES[geom]
    return netgen.int_net(in_d, widths, splices, post, netgen.WIDE, 1000 + sorted(netgen.GEOMETRIES).index(geom))


def int_utterances(layers, lengths, seed, edge=1):
    """Integer utterances in [-7, 7]; the longer ones' first and last frames
    times `edge`."""
    rng = np.random.default_rng(seed)
    us = [rng.integers(-7, 8, size=(t, netgen.in_dim(layers))).astype(np.float32) for t in lengths]
    for u in us:
        if len(u) > 3:
            u[0] *= edge
            u[-1] *= edge
    return us


def flat_feats(torch, utts, lead, poison):
    feats = np.concatenate(utts)
    return placed_flat(torch, feats, lead, poison).view(feats.shape)


@pytest.mark.parametrize("mode", ["fp32", "bf16x6"])
@pytest.mark.parametrize("geom", ["A", "H"])
def test_calibrate_through_a_misaligned_base(torch, G, ctxs, oracle, geom, mode):
    """ce_gpu_model_calibrate reads the features through the plan's row map;
    from a base one float off 16 bytes the first layer's range scan and the
    first GEMM's input both leave their float4 forms.  The ranges are the
    exact ones over the rows the reference chain holds."""
    layers = int_net_of(geom)
    ctx = ctxs["plain"]
    model = G.Model(ctx, image=netgen.image(layers)).set_gemm(mode)
    utts = int_utterances(layers, (1, 3, 37, 64, 20), 1501, edge=4)
    blocks = [i8ref.padded(layers, u) for u in utts]
    for b in blocks:
        netgen.check_exact_budget(layers, b)
    want = i8ref.fp32_held_ranges(oracle, layers, blocks)
    plan = G.Plan(ctx, [i8ref.frames_to_samples(len(u)) for u in utts], model)
    assert plan.n_chunks == 1 and plan.total_frames == sum(len(u) for u in utts)
    for lead in (0, 1, 2, 3):
        for poison in POISONS:
            got = model.calibrate(ctx, plan, flat_feats(torch, utts, lead, poison))
            assert np.array_equal(bits(got), bits(want)), (geom, mode, lead, poison, got, want)


AM_LENGTHS = (1, 33, 70)


@pytest.mark.parametrize("mode", ["fp32", "bf16x6", "latency", "static"])
@pytest.mark.parametrize("geom", ["A", "H"])
def test_am_forward_offset_bases(torch, G, ctxs, oracle, geom, mode):
    """d_feats and d_loglik one float off their allocations: three utterances
    (1, 33, 70 frames) in one chunk, each against its own padded block.  The
    prior is all ones: its log is exactly zero."""
    n = netgen.GEOMETRIES[geom][1][-1]
    prior = np.ones(n, np.float32)
    if mode == "static":
        layers, ctx = i8ref.net(geom), ctxs["plain"]
        model = G.Model(ctx, image=netgen.image(layers), prior=prior).quantize_static(ctx, i8_ranges(geom))
        utts = i8ref.utterances(layers, AM_LENGTHS, 8100 + i8ref.seed_of(geom))
        ref = lambda b: static_oracle(oracle, layers, b, i8_ranges(geom))
    else:
        layers = int_net_of(geom)
        ctx, model = load(G, ctxs, layers, mode, prior=prior)
        utts = int_utterances(layers, AM_LENGTHS, 1601)
        for u in utts:
            netgen.check_exact_budget(layers, i8ref.padded(layers, u))
        ref = lambda b: netgen.exact(layers, b)
    want = np.concatenate([ref(i8ref.padded(layers, u)) for u in utts])
    plan = G.Plan(ctx, [i8ref.frames_to_samples(t) for t in AM_LENGTHS], model)
    assert plan.n_chunks == 1 and plan.total_frames == sum(AM_LENGTHS) == len(want)
    for lead, out_lead in ((0, 0), (1, 0), (0, 1), (1, 1), (3, 2)):
        for poison in POISONS:
            out = Out(torch, len(want), n, n, out_lead)
            G.am_forward(ctx, model, plan, flat_feats(torch, utts, lead, poison), out=out.view)
            d = out.diff(want)
            assert d is None, f"{geom} {mode} feats lead={lead} {poison} loglik lead={out_lead}: {d}"


# ------------------------------------------------------ 4. which branch ran --

def test_layouts_reach_their_branches(torch, G):
    """The profile classes' launch counts: a caller's block of float4 rows --
    dense or with a gap -- is spliced by the first GEMM's own loader (no
    launch ahead of it); off 16 bytes or at an odd stride it goes through
    splice_pad; the plane program always writes the spliced planes first.
    Without this every other test here could be green on the fast path."""
    ctxs = {"bf16x6": G.Context(0), "latency": G.Context(0)}
    ctxs["latency"].set_latency(True)
    for ctx in ctxs.values():
        ctx.profile(True)

    def launches(geom, mode, gap, lead):
        _, layers, x, _ = exact_cases(geom)[0]
        ctx = ctxs["latency" if mode == "latency" else "bf16x6"]
        model = G.Model(ctx, image=netgen.image(layers)).set_gemm(MODES[mode][1])
        x = x[:70 + model.left + model.right]
        ctx.profile_read(ctx.PROF_GEMM_GATHER), ctx.profile_read(ctx.PROF_GEMM)
        G.nnet_propagate(ctx, model, placed(torch, x, x.shape[1] + gap, lead, "nan"))
        torch.cuda.synchronize()
        return ctx.profile_read(ctx.PROF_GEMM_GATHER)[1], ctx.profile_read(ctx.PROF_GEMM)[1]

    for geom in ("A", "H"):
        for mode in ("bf16x6", "latency"):
            for gap, lead in LAYOUTS:
                direct = (gap, lead) in ALIGNED
                assert launches(geom, mode, gap, lead) == ((0, 3) if direct else (1, 3)), (geom, mode, gap, lead)
                layers = exact_cases(geom)[0][1]
                assert netgen.kernels(layers, 70, mode, caller_aligned=direct)[0].startswith("splice_pad+") != direct
        for gap, lead in LAYOUTS:
            assert launches(geom, "bf16x6p", gap, lead) == (1, 3), (geom, gap, lead)
    for ctx in ctxs.values():
        ctx.profile(False)


# ------------------------------- 5. finalize and the fused latency tail --

@pytest.mark.parametrize("geom", ["A", "G9", "F4100"])
def test_finalize_on_an_offset_output(torch, G, ctxs, geom):
    """LogSoftmax and the prior subtraction into an output one or two floats
    off 16 bytes: launch_finalize moves the row's chunks with 4-byte accesses
    (n = 772, 3456) or takes the loop (4100), and latency mode cannot fuse the
    last reduce into the finalize (lat_tail_ok), so lat_reduce and this
    finalize run.  Where the output lies changes no bit, in any mode: the exp
    sum keeps one order (this test found the 4-byte form summing in another:
    3403 of 241920 values of G9 differed in the last place)."""
    rows = 70
    layers, x = real_case(geom, rows)
    want = real_reference(geom, rows, True)
    n = want.shape[1]
    assert n == {"A": 772, "G9": 3456, "F4100": 4100}[geom]
    assert netgen.finalize_path(n) == ("loop" if n > 4096 else "vector")
    prior = netgen.prior(n, 77)
    errs, got = {}, {}
    for mode in ("fp32", "bf16x6", "latency"):
        ctx, model = load(G, ctxs, layers, mode, prior=prior)
        for out_lead in (0, 1, 2):
            out = Out(torch, rows, n, n, out_lead)
            G.nnet_propagate(ctx, model, dev(torch, x), subtract_prior=True, out=out.view)
            words, msg = out.read()
            assert msg is None, f"{geom} {mode} out lead={out_lead}: {msg}"
            got[mode, out_lead] = words.view(np.float32)
            errs[mode, out_lead] = float(np.abs(got[mode, out_lead].astype(np.float64) - want).max())
    print(geom, errs)
    assert max(errs.values()) <= LOGLIK_TOL, errs
    for mode in ("fp32", "bf16x6", "latency"):
        for out_lead in (1, 2):
            d = first_diff(got[mode, out_lead], got[mode, 0])
            assert d is None, f"{geom} {mode}, out lead={out_lead} against the aligned output: {d}"


@pytest.mark.parametrize("mode", ["fp32", "bf16x6", "latency"])
@pytest.mark.parametrize("geom", ["A", "H"])
def test_real_nets_do_not_depend_on_the_layout(torch, G, ctxs, geom, mode):
    """Real-valued weights, where a summation order shows: every kernel a
    layout can send the first layer to (the loaders' gather or splice_pad, the
    fp32 LDS-DMA kernel or pipe2) adds the K products into one accumulator in
    ascending K, so the rows carry the dense, aligned input's bits."""
    layers, x = real_case(geom, 70)
    ctx, model = load(G, ctxs, layers, mode)
    want = G.nnet_propagate(ctx, model, dev(torch, x)).cpu().numpy()
    assert float(np.abs(want - real_reference(geom, 70, False)).max()) <= LOGLIK_TOL
    failures = sweep(torch, G, ctx, model, [(x, want)], f"{geom} real {mode}")
    assert not failures, "\n".join(failures[:20])


# ----------------------------------------------------------- 6. primitives --

GEMM_SHAPES = [(5, 3, 2), (37, 50, 3), (129, 100, 64), (70, 36, 200)]


def operand_layouts(operands):
    """One operand at a time through every layout (the others dense and
    aligned), then all of them at (3, 2)."""
    dense = {o: (0, 0) for o in operands}
    out = [dense]
    for o in operands:
        out += [dict(dense, **{o: lay}) for lay in LAYOUTS[1:]]
    out.append({o: (3, 2) for o in operands})
    return out


def int_operands(m, n, k, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(-7, 8, size=(m, k)).astype(np.float32)
    b = rng.integers(-7, 8, size=(k, n)).astype(np.float32)
    bias = rng.integers(-64, 65, size=n).astype(np.float32)
    assert k <= 200    # |sum| <= 200 * 49 + 64: every order is exact
    return a, b, bias, a.astype(np.int64) @ b.astype(np.int64)


@pytest.mark.parametrize("shape", GEMM_SHAPES)
def test_sgemm(torch, G, ctxs, shape):
    m, n, k = shape
    a, b, _, prod = int_operands(m, n, k, m + n + k)
    want = prod.astype(np.float32)
    failures = []
    for lay in operand_layouts("abc"):
        da = placed(torch, a, k + lay["a"][0], lay["a"][1], "nan")
        db = placed(torch, b, n + lay["b"][0], lay["b"][1], "nan")
        out = Out(torch, m, n, n + lay["c"][0], lay["c"][1])
        G.sgemm(ctxs["plain"], da, db, out.view)
        d = out.diff(want)
        if d:
            failures.append(f"{shape} {lay}: {d}")
    assert not failures, "\n".join(failures[:20])


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("shape", GEMM_SHAPES)
def test_linear(torch, G, ctxs, shape, with_bias):
    m, n, k = shape
    a, w, bias, prod = int_operands(m, n, k, 2 * (m + n + k) + 1)
    want = (prod + (bias.astype(np.int64) if with_bias else 0)).astype(np.float32)
    failures = []
    for lay in operand_layouts(("x", "w", "out", "bias") if with_bias else ("x", "w", "out")):
        dx = placed(torch, a, k + lay["x"][0], lay["x"][1], "nan")
        dw = placed(torch, w, n + lay["w"][0], lay["w"][1], "nan")
        db = placed_flat(torch, bias, lay["bias"][1]) if with_bias else None
        out = Out(torch, m, n, n + lay["out"][0], lay["out"][1])
        G.linear(ctxs["plain"], dx, dw, db, out.view)
        d = out.diff(want)
        if d:
            failures.append(f"{shape} {lay}: {d}")
    assert not failures, "\n".join(failures[:20])


@pytest.mark.parametrize("dim", [24, 33])
def test_splice(torch, G, ctxs, oracle, dim):
    idx = [-3, 0, 2]
    x = np.random.default_rng(dim).normal(0, 1.5, size=(9, dim)).astype(np.float32)
    want = oracle.layer_forward({"kind": "splice", "indices": idx}, x)
    for gap, lead in LAYOUTS:
        for out_lead in (0, 1):
            out = Out(torch, 9, 3 * dim, 3 * dim, out_lead)
            G.splice(ctxs["plain"], placed(torch, x, dim + gap, lead, "nan"), idx, out.view)
            d = out.diff(want)
            assert d is None, f"dim={dim} ld-width={gap} lead={lead} out lead={out_lead}: {d}"


ROW_EXACT = ("relu", "batchnorm")


@pytest.mark.parametrize("op", ["relu", "batchnorm", "softmax", "log_softmax", "normalize"])
def test_rowwise(torch, G, ctxs, oracle, op):
    """In place on rows ld apart: ReLU and BatchNorm bit for bit, the three
    reductions within LOGLIK_TOL of the oracle; the gap columns keep their
    bits (Out's sentinels)."""
    failures = []
    for rows in (1, 5):
        for dim in (1, 24, 64, 65, 257):
            rng = np.random.default_rng(rows * 1000 + dim)
            x = rng.normal(0, 1.5, size=(rows, dim)).astype(np.float32)
            layer = {"kind": op}
            if op == "batchnorm":
                layer.update(scale=rng.uniform(0.5, 1.5, dim).astype(np.float32),
                             offset=rng.normal(0, 1, dim).astype(np.float32))
            want = oracle.layer_forward(layer, x)
            for gap, lead in LAYOUTS:
                io = Out(torch, rows, dim, dim + gap, lead, init=x)
                scale = placed_flat(torch, layer["scale"], lead) if op == "batchnorm" else None
                offset = placed_flat(torch, layer["offset"], (lead + 1) % 4) if op == "batchnorm" else None
                G.rowwise(ctxs["plain"], op, io.view, scale, offset)
                words, msg = io.read()
                got = words.view(np.float32)
                if msg is None and op in ROW_EXACT:
                    msg = first_diff(got, want)
                elif msg is None and not np.abs(got.astype(np.float64) - want).max() <= LOGLIK_TOL:
                    msg = f"max |got - oracle| = {np.abs(got.astype(np.float64) - want).max()}"
                if msg:
                    failures.append(f"{op} rows={rows} dim={dim} ld-width={gap} lead={lead}: {msg}")
    assert not failures, "\n".join(failures[:20])


@pytest.fixture(scope="module")
def scored(torch, G, ctxs, xs_config):
    """tests/test_gpu_decoder_gather.py's rows (the XS model on two
    utterances), laid at ld = dim + 5 from a base one float off, the gap NaN."""
    from catears_amd import synth
    ctx = ctxs["plain"]
    model = G.Model(ctx, xs_config)
    waves = [synth.pcm(70 + i, 16000 * 2 + 333 * i) for i in range(2)]
    plan = G.Plan(ctx, [len(w) for w in waves], model)
    ll = G.score(ctx, model, plan, torch.from_numpy(np.concatenate(waves)).cuda())
    torch.cuda.synchronize()
    host = ll.cpu().numpy()
    return model, host, placed(torch, host, host.shape[1] + 5, 1, "nan")


@pytest.mark.parametrize("n,am_scale", [(1, 1.0), (5000, 0.1), (100003, 0.0833)])
def test_loglik_gather(torch, G, ctxs, oracle, scored, n, am_scale):
    model, host, ll = scored
    assert ll.stride(0) == host.shape[1] + 5 and ll.data_ptr() % 16 == 4
    tpm = model.tid2pdf()
    rng = np.random.default_rng(n)
    rows = rng.integers(0, ll.shape[0], n).astype(np.int32)
    trans = rng.integers(1, len(tpm), n).astype(np.int32)
    out = Out(torch, 1, n, n, 1)
    G.loglik_gather(ctxs["plain"], ll, dev(torch, tpm), dev(torch, rows), dev(torch, trans), am_scale,
                    out=out.view.view(-1))
    d = out.diff(oracle.decoder_loglikelihood(host, tpm, rows, trans, am_scale).reshape(1, n))
    assert d is None, d


def test_loglik_gather_edges(torch, G, ctxs, scored):
    model, host, ll = scored
    ctx = ctxs["plain"]
    tpm = dev(torch, model.tid2pdf())
    rows = torch.tensor([0, -1, ll.shape[0], 3, 3], dtype=torch.int32, device="cuda")
    trans = torch.tensor([1, 1, 1, -5, tpm.numel()], dtype=torch.int32, device="cuda")
    got = G.loglik_gather(ctx, ll, tpm, rows, trans).cpu().numpy()
    assert np.isfinite(got[0]) and np.isnan(got[1:]).all()
    # a pdf in the gap columns (dim <= pdf < ld) is outside the row too
    bad = torch.tensor([0, ll.shape[1], -1, 2**30, ll.shape[1] + 4], dtype=torch.int32, device="cuda")
    rows = torch.tensor([0, 0, 0, ll.shape[0] - 1, 0], dtype=torch.int32, device="cuda")
    trans = torch.tensor([0, 1, 2, 3, 4], dtype=torch.int32, device="cuda")
    got = G.loglik_gather(ctx, ll, bad, rows, trans).cpu().numpy()
    assert np.isfinite(got[0]) and np.isnan(got[1:]).all()
    assert got[0] == host[0, 0]


def test_loglik_columns(torch, G, ctxs, scored):
    _, host, ll = scored
    rng = np.random.default_rng(9)
    dim = ll.shape[1]
    cols = np.concatenate([rng.permutation(dim)[:97], [0, dim - 1, dim, -1]]).astype(np.int32)
    out = Out(torch, ll.shape[0], len(cols), len(cols), 1)
    G.loglik_columns(ctxs["plain"], ll, dev(torch, cols), out=out.view)
    words, msg = out.read()
    assert msg is None, msg
    got = words.view(np.float32)
    assert np.array_equal(bits(got[:, :-2]), bits(host[:, cols[:-2]]))
    assert np.isnan(got[:, -2:]).all()


def byte_buffer(torch, payload, lead):
    """uint8 `payload` at byte `lead` of a buffer of SENTINEL_BYTE."""
    payload = np.ascontiguousarray(payload, np.uint8)
    host = np.full(lead + payload.size + TAIL, SENTINEL_BYTE, np.uint8)
    host[lead:lead + payload.size] = payload.ravel()
    base = upload(torch, host)
    return base, base[lead:lead + payload.size].view(payload.shape)


@pytest.mark.parametrize("count", [1, 5, 1023, 4097])
def test_quantize(torch, G, ctxs, oracle, count):
    x = np.random.default_rng(count).uniform(-0.5, 1.5, count).astype(np.float32)
    want, s, z = oracle.quantize(x)
    for poison in POISONS:
        for x_lead in (0, 1, 3):
            for q_lead in (0, 1, 3):
                base, q = byte_buffer(torch, np.full(count, SENTINEL_BYTE, np.uint8), q_lead)
                _, prm = G.quantize(ctxs["plain"], placed_flat(torch, x, x_lead, poison), q=q)
                what = f"count={count} {poison} x lead={x_lead} q lead={q_lead}"
                assert G.params_host(prm) == (s, z), what
                host = base.cpu().numpy()
                assert np.array_equal(host[q_lead:q_lead + count], want.ravel()), what
                host[q_lead:q_lead + count] = SENTINEL_BYTE
                assert (host == SENTINEL_BYTE).all(), what + ": bytes outside d_q overwritten"


@pytest.mark.parametrize("k", [64, 80])
@pytest.mark.parametrize("m,n", [(70, 45), (129, 130)])
def test_gemm_u8(torch, G, ctxs, oracle, m, n, k):
    """k % 16 == 0, so the base alone decides gemm_i8_kernel's 16-byte A
    loads."""
    ctx = ctxs["plain"]
    rng = np.random.default_rng(m + n + k)
    A = rng.uniform(-0.5, 0.5, (m, k)).astype(np.float32)
    B = rng.uniform(1, 2, (k, n)).astype(np.float32)
    oa, sa, za = oracle.quantize(A)
    ob, sb, zb = oracle.quantize(B)
    _, pa = G.quantize(ctx, dev(torch, A))
    _, pb = G.quantize(ctx, dev(torch, B))
    assert G.params_host(pa) == (sa, za) and G.params_host(pb) == (sb, zb)
    want_i = oracle.gemm_u8u8_i32(oa, za, ob, zb)
    want_f = oracle.gemm_u8u8f32(oa, sa, za, ob, sb, zb)
    for a_lead, b_lead in ((0, 0), (1, 0), (3, 0), (8, 0), (0, 1), (1, 1), (3, 1), (8, 1)):
        _, qa = byte_buffer(torch, oa, a_lead)
        _, qb = byte_buffer(torch, ob, b_lead)
        what = f"A lead={a_lead} B lead={b_lead}"
        assert np.array_equal(G.gemm_u8(ctx, qa, pa, qb, pb, out_int32=True).cpu().numpy(), want_i), what
        assert np.array_equal(bits(G.gemm_u8(ctx, qa, pa, qb, pb).cpu().numpy()), bits(want_f)), what
