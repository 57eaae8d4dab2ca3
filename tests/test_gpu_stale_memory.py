"""No call reads library-owned device memory it did not write.

A context carries a workspace, a scratch buffer, latency partials and block
maps; a session set staging regions, rings, a CMVN carry, caches and per-push
scratch.  The same bytes are an activation in one call and a pad column or an
unused tile row in the next, and a fresh device page is usually zero, so a
stray read of them passes every test that runs on finite residue.  Here the
residue is made hostile (tests/devfill.py: a NaN word and a 3.0e38 word
through the library's ce_gpu_debug_fill_* entries) and every call must give
the same bits.  All comparisons are on uint32 views, zero tolerance.

A. fresh allocations: context, model, plan and session set created while
   every allocation arrives filled; every mode, net and entry point once.
B. residue between calls: the largest seam count, fill, the smallest, fill,
   the largest (the ping-pong block moves between them); then a wide model,
   fill, a narrow model in another mode on the same context.
C. the same through the public API alone (no hook: a cross-check of the
   hook's buffer list): an all-NaN block through the wide model, then the
   finite cases.
D. reset slots: 7 s into a slot (raw ring wrapped, windowed CMVN), reset,
   every region of the slot filled, a second utterance in ragged pushes
   gives its one-shot rows; a live neighbour keeps its own.  Teeth: the same
   fill on a live slot does change its rows.
E. per-push scratch filled between every two pushes of a three-slot set.

References: netgen.exact / bf16ref.walk / rownet on exact-integer nets, the
int8 oracle (bit exact) on i8ref's nets, and for TDNN-XS the oracle bars of
tests/test_gpu_parity.py plus the bits of the same call on a context whose
memory nobody filled."""
import collections
import functools

import numpy as np
import pytest

import bf16ref
import devfill
import i8ref
import netgen
import padnet
import rownet
import rowseams
from test_gpu_gemm_shapes import first_diff
from test_gpu_parity import LOGLIK_TOL, am_oracle, bits, dev
from test_int8_static import fp32_ranges, static_oracle

pytestmark = pytest.mark.gpu

WORDS = sorted(devfill.WORDS)

# mode -> (context flavour, ce_gpu_model_set_gemm mode)
GEMM_MODES = {"fp32": ("plain", "fp32"), "bf16x6": ("plain", "bf16x6"), "bf16x6p": ("plain", "bf16x6p"),
              "wide": ("wide", "bf16x6"), "latency": ("latency", "bf16x6"), "f16x3": ("plain", "f16x3"),
              "bf16": ("plain", "bf16"), "bf16-latency": ("latency", "bf16")}
I8_MODES = {"int8": "plain", "int8-latency": "latency", "int8-dynamic": "plain"}
X6_MODES = ("fp32", "bf16x6", "bf16x6p", "wide", "latency", "bf16", "bf16-latency")
ROW_MODES = ("fp32", "bf16x6", "latency", "bf16")
ROW_NETS = ("second-bn", "row-last", "normalize-96")
BLOCKS = (70, 33, 151)   # output rows of the three packed blocks


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


@pytest.fixture(scope="module", autouse=True)
def fill_allocs_stays_inside_this_module(torch, G):
    """Every test switches the allocation fill on and off around its own
    block (devfill.fresh_allocations); whatever a failure leaves behind, no
    other module sees it."""
    G.debug_fill_allocs(False)
    yield
    G.debug_fill_allocs(False)


def new_ctx(G, flavour):
    ctx = G.Context(0)
    if flavour == "wide":
        ctx.set_wide_tiles(True)
    if flavour == "latency":
        ctx.set_latency(True)
    return ctx


@pytest.fixture(scope="module")
def ctxs(torch, G):
    """Contexts nobody fills at allocation (leg B, C and the references)."""
    return {f: new_ctx(G, f) for f in ("plain", "wide", "latency")}


def seam_mode(mode):
    return "bf16" if mode == "bf16-latency" else mode


# -------------------------------------------------------------- the cases --
# id -> Case.  want: the rows of x at its full length, of which a call on the
# first m rows must give the first m - context (a function of m for dynamic
# int8, whose rows depend on the block).  counts: (smallest, largest) input
# row count.  width: the widest layer output (the workspace bound of leg B).

Case = collections.namedtuple("Case", "layers x want flavour prepare counts width fp32_blocks")


def exact_ids():
    out = [f"{g}-{m}" for g in ("A", "C") for m in X6_MODES + ("f16x3",)]
    out += ["E-fp32"] + [f"Epad-{m}" for m in X6_MODES]
    out += [f"{n}-{m}" for n in ROW_NETS for m in ROW_MODES]
    return out


def i8_ids():
    return ["renorm128-int8", "renorm128-int8-latency"] + [f"{g}-{m}" for g in ("I1", "I2") for m in I8_MODES]


CASE_IDS = exact_ids() + i8_ids()


@functools.lru_cache(maxsize=None)
def exact_net(geom, recipe):
    """netgen's exact-integer net of a geometry with an input at the largest
    seam count of any mode (2049 rows: two latency windows and a row; A's own
    at 3073, where its 800-wide layer reaches the 512 x 128 kernel)."""
    if geom == "A":
        return rowseams.exact_case("A", recipe)
    form = "f16x3" if recipe == "FX" else "bf16x6"
    layers, = [c[1] for c in netgen.exact_cases(geom, form) if c[0] == recipe]
    xargs = dict(amax=7) if recipe == "wide" else netgen.plane_recipes(len(netgen.linears(layers)), form)[recipe][1]
    x = netgen.int_input(layers, 2049 - sum(netgen.context(layers)), 7100 + "CE".index(geom), **xargs)
    x.setflags(write=False)
    return layers, x


@functools.lru_cache(maxsize=None)
def exact_rows(geom, recipe, bf16):
    layers, x = exact_net(geom, recipe)
    netgen.check_exact_budget(layers, x, "f16x3" if recipe == "FX" else "bf16x6")
    if bf16:
        assert max(bf16ref.exact_bounds(layers, x[:300])) < 24
        return bf16ref.walk(layers, x, np.float64).astype(np.float32)
    return netgen.exact(layers, x)


@functools.lru_cache(maxsize=None)
def row_rows(name, bf16):
    layers, x = rownet.exact_cases()[name]
    want = rownet.walk(layers, x, rnd=bf16ref.rne_bf16) if bf16 else rownet.check_exact(layers, x)
    return np.ascontiguousarray(want, np.float32)


def seam_pair(shape_layers, mode, rows):
    counts = [m for m in rowseams.seam_rows(shape_layers, seam_mode(mode)) if m <= rows]
    return counts[0], counts[-1]


_CASES = {}


def case(cid, torch, G, ctxs, oracle):
    if cid not in _CASES:
        _CASES[cid] = build_case(cid, torch, G, ctxs, oracle)
    return _CASES[cid]


def build_case(cid, torch, G, ctxs, oracle):
    name, mode = next((cid[:-len(m) - 1], m) for m in sorted(list(GEMM_MODES) + list(I8_MODES), key=len, reverse=True)
                      if cid.endswith("-" + m))
    if mode in GEMM_MODES:
        flavour, gemm = GEMM_MODES[mode]
        bf16 = gemm == "bf16"
        if name in ROW_NETS:
            layers, x = rownet.exact_cases()[name]
            want = row_rows(name, bf16)
            counts = (rowseams.row_kernel_rows()[0], rowseams.row_kernel_rows()[-1])

            def prepare(ctx, prior=None):
                model = G.Model(ctx, image=netgen.image(layers), prior=prior)
                assert model.gemm == "fp32" and model.admit_row_ops(ctx) is model and model.gemm == "bf16x6"
                return model.set_gemm(gemm)
        else:
            geom, pad = name[0], name.endswith("pad")
            layers, x = exact_net(geom, "FX" if mode == "f16x3" else "wide")
            want = exact_rows(geom, "FX" if mode == "f16x3" else "wide", bf16)
            counts = seam_pair(padnet.pad_layers(layers) if pad else layers, mode, len(x))

            def prepare(ctx, prior=None):
                model = G.Model(ctx, image=netgen.image(layers), prior=prior)
                if pad:
                    assert model.gemm == "fp32" and model.pad_widths(ctx) is model
                if geom == "E" and not pad:
                    assert model.gemm == "fp32" and not netgen.x6_ok(layers)   # the fp32 program, masked K
                    return model
                assert model.gemm == "bf16x6"
                return model.set_gemm(gemm)
        fp32_blocks = gemm == "fp32"
    else:
        flavour = I8_MODES[mode]
        if name == "renorm128":
            import i8rowref
            from test_gpu_i8_row_chain import calibrated, renorm
            layers = i8rowref.without_final_log_softmax(renorm(128)[0])
            counts = rowseams.row_kernel_rows(rowseams.FAMILIES["i8_256x128"][0])
            counts = (counts[0], counts[-1])
            x = np.random.default_rng(7900).normal(0.0, 1.0, size=(counts[-1], 40)).astype(np.float32)
            ranges = calibrated(torch, G, ctxs["plain"], 128)
            want = i8rowref.static_rows(oracle, layers, x, ranges)
        else:
            layers = i8ref.net(name)
            counts = seam_pair(layers, mode, rowseams.CAP)
            x = netgen.real_input(layers, counts[-1] - sum(netgen.context(layers)), 7700 + i8ref.seed_of(name))
            if mode == "int8-dynamic":
                ranges = None
                want = functools.lru_cache(maxsize=None)(
                    lambda m: i8ref.chunk_reference(oracle, layers, [x[:m]])[0][0])
            else:
                ranges = fp32_ranges(oracle, layers, i8ref.calibration_input(name))
                want = static_oracle(oracle, layers, x, ranges)

        def prepare(ctx, prior=None):
            model = G.Model(ctx, image=netgen.image(layers), prior=prior)
            return model.quantize(ctx) if ranges is None else model.quantize_static(ctx, ranges)
        fp32_blocks = True
    if not callable(want):
        want = np.ascontiguousarray(want, np.float32)
        want.setflags(write=False)
    width = max(g["n"] for g in netgen.linears(layers))
    assert sum(netgen.context(layers)) < counts[0] <= counts[1] <= len(x)
    return Case(layers, x, want, flavour, prepare, counts, width, fp32_blocks)


_DEVICE = {}


def on_device(torch, cid, c):
    """(x, want) of a case as device tensors, uploaded once."""
    if cid not in _DEVICE:
        _DEVICE[cid] = (dev(torch, np.array(c.x, np.float32)),
                        None if callable(c.want) else dev(torch, np.array(c.want, np.float32)))
    return _DEVICE[cid]


def wanted(torch, cid, c, m):
    xd, wd = on_device(torch, cid, c)
    if wd is None:
        return dev(torch, np.array(c.want(m), np.float32))
    return wd[:m - sum(netgen.context(c.layers))]


def check_rows(torch, G, ctx, model, cid, c, m, what):
    """nnet_propagate on the first m rows; returns the result."""
    xd, _ = on_device(torch, cid, c)
    got = G.nnet_propagate(ctx, model, xd[:m])
    want = wanted(torch, cid, c, m)
    assert devfill.same_bits(torch, got, want), \
        f"{cid} m={m} {what}: {first_diff(got.cpu().numpy(), want.cpu().numpy())}"
    return got


def check_blocks(torch, G, ctx, model, cid, c, what):
    """nnet_propagate_blocks on three blocks cut from x: each gives the rows
    it gives alone (static rows do not depend on the batch)."""
    if callable(c.want):
        return
    xd, wd = on_device(torch, cid, c)
    ctx_rows = sum(netgen.context(c.layers))
    # (the f16x3 case's input ends at its largest seam count, 257 rows)
    blocks = BLOCKS if sum(BLOCKS) + ctx_rows <= len(c.x) else BLOCKS[:2] + (129,)
    starts = np.concatenate([[0], np.cumsum(blocks)])
    assert starts[-1] + ctx_rows <= len(c.x)
    packed = torch.cat([xd[s:s + n + ctx_rows] for s, n in zip(starts, blocks)])
    got = G.nnet_propagate_blocks(ctx, model, packed, [n + ctx_rows for n in blocks])
    want = wd[:starts[-1]]
    assert devfill.same_bits(torch, got, want), \
        f"{cid} blocks {what}: {first_diff(got.cpu().numpy(), want.cpu().numpy())}"


def settle_f16(ctx, mode):
    """f16x3 reports through the sticky overflow word, which no fill touches:
    an exact case leaves it clear."""
    if mode.endswith("f16x3"):
        assert not ctx.overflow()


# --------------------------------------------- A. fresh allocations: nets --

@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("cid", CASE_IDS)
def test_fresh_allocations_are_not_assumed_zero(torch, G, ctxs, oracle, cid, word):
    """Context and model created while every allocation arrives filled; the
    smallest seam count first (everything behind its rows and columns is the
    word), then the largest (the workspaces grow: fresh, filled buffers
    again), then three packed blocks (the block maps)."""
    c = case(cid, torch, G, ctxs, oracle)
    on_device(torch, cid, c)
    with devfill.fresh_allocations(G, devfill.WORDS[word]):
        ctx = new_ctx(G, c.flavour)
        model = c.prepare(ctx)
        for m in c.counts:
            check_rows(torch, G, ctx, model, cid, c, m, f"fresh {word}")
        check_blocks(torch, G, ctx, model, cid, c, f"fresh {word}")
        settle_f16(ctx, cid)
        ctx.synchronize()
    model.close()
    ctx.close()


# ------------------------------------------ B. residue between two calls --

@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("cid", CASE_IDS)
def test_residue_between_calls(torch, G, ctxs, oracle, cid, word):
    """Large, fill, small, fill, large, fill, blocks: the second activation
    block sits at rows * max_width, so the small call's blocks lie inside what
    the large one used.  The fill covers at least what the large call wrote."""
    c = case(cid, torch, G, ctxs, oracle)
    w = devfill.WORDS[word]
    ctx = ctxs[c.flavour]
    model = c.prepare(ctx)
    small, large = c.counts
    first = check_rows(torch, G, ctx, model, cid, c, large, "first").clone()
    filled = devfill.fill_ctx(G, ctx, w)
    # every program keeps the widest layer's output for all rows, as bf16 at
    # the least; the fp32 and int8 programs two fp32 blocks of it
    assert filled >= large * c.width * (8 if c.fp32_blocks else 2), (filled, large, c.width)
    check_rows(torch, G, ctx, model, cid, c, small, f"after {word} fill")
    assert devfill.fill_ctx(G, ctx, w) == filled
    again = check_rows(torch, G, ctx, model, cid, c, large, f"after {word} fill")
    assert devfill.same_bits(torch, again, first)
    devfill.fill_ctx(G, ctx, w)
    check_blocks(torch, G, ctx, model, cid, c, f"after {word} fill")
    settle_f16(ctx, cid)
    model.close()


# a wide model, the fill, then a narrow one in another mode on that context
CROSS = [("A-fp32", "C-bf16"), ("A-latency", "I1-int8-latency"), ("I2-int8", "C-bf16x6"), ("A-bf16x6", "Epad-bf16x6p"),
         ("A-bf16", "normalize-96-fp32"), ("I2-int8", "renorm128-int8"), ("A-bf16-latency", "second-bn-latency"),
         ("A-fp32", "E-fp32"), ("I2-int8-dynamic", "I1-int8")]


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("wide,narrow", CROSS)
def test_residue_between_models(torch, G, ctxs, oracle, wide, narrow, word):
    a, b = case(wide, torch, G, ctxs, oracle), case(narrow, torch, G, ctxs, oracle)
    assert a.flavour == b.flavour and a.width > b.width
    ctx = ctxs[a.flavour]
    ma, mb = a.prepare(ctx), b.prepare(ctx)
    check_rows(torch, G, ctx, ma, wide, a, a.counts[1], "wide model")
    devfill.fill_ctx(G, ctx, devfill.WORDS[word])
    for m in b.counts:
        check_rows(torch, G, ctx, mb, narrow, b, m, f"behind {wide} and the {word} fill")
    devfill.fill_ctx(G, ctx, devfill.WORDS[word])
    check_rows(torch, G, ctx, ma, wide, a, a.counts[0], f"behind {narrow} and the {word} fill")
    ma.close()
    mb.close()


# ------------------------------------------- C. through the public API alone --

SELF = ["A-" + m for m in X6_MODES + ("f16x3",)] + ["I2-int8", "I1-int8-latency", "I2-int8-dynamic", "renorm128-int8"]
API_PAIRS = [(p, p) for p in SELF] + CROSS + [("A-bf16x6", "second-bn-bf16x6"), ("A-bf16", "row-last-bf16"),
                                              ("A-wide", "C-wide"), ("A-latency", "C-latency")]


@pytest.mark.parametrize("poison,victim", API_PAIRS)
def test_nan_block_leaves_nothing_behind(torch, G, oracle, ctxs, poison, victim):
    """No hook: a block whose every input row is NaN through the wide model at
    its largest count leaves NaN in every buffer the program wrote (int8: the
    quantizer's clamped bytes, and NaN in the fp32 blocks behind the last
    GEMM's bias-less products is not guaranteed -- the hook legs cover those).
    The finite cases on the same context then give the reference's bits, as
    on a context that never saw it."""
    a, b = case(poison, torch, G, ctxs, oracle), case(victim, torch, G, ctxs, oracle)
    assert a.flavour == b.flavour
    ctx = new_ctx(G, a.flavour)
    ma = a.prepare(ctx)
    mb = ma if poison == victim else b.prepare(ctx)
    nan = torch.full((a.counts[1], a.x.shape[1]), float("nan"), dtype=torch.float32, device="cuda")
    out = G.nnet_propagate(ctx, ma, nan)
    if poison.split("-", 1)[1] in GEMM_MODES:
        assert bool(torch.isnan(out).all()), poison
    if poison.endswith("f16x3"):
        assert ctx.overflow()     # a NaN leaves the fp16 range: flagged, and cleared by the read
    for m in b.counts + b.counts[:1]:
        check_rows(torch, G, ctx, mb, victim, b, m, f"behind a NaN block of {poison}")
    check_blocks(torch, G, ctx, mb, victim, b, f"behind a NaN block of {poison}")
    settle_f16(ctx, victim)
    ctx.synchronize()
    mb.close()
    if ma is not mb:
        ma.close()
    ctx.close()


# ------------------------------------------------ TDNN-XS: the entry points --

XS_MODES = ("fp32", "bf16x6", "latency", "bf16", "int8", "int8-latency")
XS_ORACLE_BAR = ("fp32", "bf16x6", "latency")   # fp32-accurate forms (tests/test_gpu_parity.py's bar)
UTTS = (400, 3333, 16000)                       # 1, 19 and 98 frames


def xs_flavour(mode):
    return "latency" if mode.endswith("latency") else "plain"


@pytest.fixture(scope="module")
def xs_ranges(torch, G, ctxs, xs_config):
    """TDNN-XS calibrated on three utterances nobody scores (as
    tests/test_int8_static.py's xs_static)."""
    from catears_amd import synth
    ctx = ctxs["plain"]
    m = G.Model(ctx, xs_config)
    waves = [synth.pcm(60 + i, 16000 * 3) for i in range(3)]
    plan = G.Plan(ctx, [len(w) for w in waves], m)
    ranges = m.calibrate(ctx, plan, G.fbank(ctx, plan, dev(torch, np.concatenate(waves))))
    assert ranges.shape == (m.num_linear, 2) and np.all(ranges[:, 0] < ranges[:, 1])
    return ranges


def xs_model(G, ctx, xs_config, mode, xs_ranges):
    m = G.Model(ctx, xs_config)
    if mode.startswith("int8"):
        return m.quantize_static(ctx, xs_ranges)
    return m.set_gemm({"latency": "bf16x6"}.get(mode, mode))


@pytest.fixture(scope="module")
def gs(torch, global_stats):
    return dev(torch, global_stats)


@pytest.fixture(scope="module")
def utts():
    from catears_amd import synth
    return [synth.pcm(7300 + i, n) for i, n in enumerate(UTTS)]


def pipeline(torch, G, ctx, model, utts, gs, calibrate):
    """Every entry point of the scoring pipeline on the three utterances, on
    a plan of more than one chunk: score, fbank + cmvn + am_forward, calibrate,
    and a plain and an incremental session set streaming the last utterance
    in 100 ms pushes.  Returns the results as host arrays; closes the model."""
    pcm = dev(torch, np.concatenate(utts))
    plan = G.Plan(ctx, [len(u) for u in utts], model, max_rows=64)
    assert plan.n_chunks > 1 and plan.total_frames == 1 + 19 + 98
    out = {"score": G.score(ctx, model, plan, pcm, gs).cpu().numpy()}
    feats = G.cmvn(ctx, plan, gs, G.fbank(ctx, plan, pcm))
    out["am_forward"] = G.am_forward(ctx, model, plan, feats).cpu().numpy()
    if calibrate:
        out["calibrate"] = model.calibrate(ctx, plan, feats)
    wave = dev(torch, utts[-1])
    counts = [1600] * (len(utts[-1]) // 1600)
    assert sum(counts) == len(utts[-1])
    for kind in ("plain", "incremental"):
        sess = G.Sessions(ctx, model, 1, 1600, gs, incremental=kind == "incremental")
        try:
            rows, at = [], 0
            for i, n in enumerate(counts):
                got, _ = sess.push([0], wave[at:at + n], [n], eos=[i == len(counts) - 1])
                rows.append(got.cpu().numpy())
                at += n
            out["sessions-" + kind] = np.concatenate(rows)
        finally:
            sess.close()
    model.close()
    return out


_XS_CLEAN = {}


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("mode", XS_MODES)
def test_fresh_allocations_through_the_pipeline(torch, G, ctxs, oracle, xs_config, xs_ranges, gs, utts, global_stats,
                                                mode, word):
    """Context, model, plan and both session sets created under the fill give
    the bits of a context nobody filled; the streamed rows are the one-shot
    rows; the fp32-accurate forms are within the oracle's bar."""
    from catears_amd import formats
    calibrate = mode in ("fp32", "bf16x6")

    def run(ctx):
        return pipeline(torch, G, ctx, xs_model(G, ctx, xs_config, mode, xs_ranges), utts, gs, calibrate)

    if mode not in _XS_CLEAN:
        _XS_CLEAN[mode] = run(ctxs[xs_flavour(mode)])
    clean = _XS_CLEAN[mode]
    with devfill.fresh_allocations(G, devfill.WORDS[word]):
        ctx = new_ctx(G, xs_flavour(mode))
        got = run(ctx)
        ctx.synchronize()
    ctx.close()
    assert sorted(got) == sorted(clean)
    for k in sorted(got):
        assert got[k].shape == clean[k].shape and np.array_equal(bits(got[k]), bits(clean[k])), \
            f"{mode} {word} {k}: {first_diff(got[k], clean[k])}"
    assert np.array_equal(bits(got["am_forward"]), bits(got["score"]))
    last = got["score"][1 + 19:]
    for kind in ("plain", "incremental"):
        assert np.array_equal(bits(got["sessions-" + kind]), bits(last)), kind
    if mode in XS_ORACLE_BAR:
        am = formats.read_am(xs_config)
        fb, at = oracle.Fbank(), 0
        for u in utts:
            ref = am_oracle(oracle, am, oracle.cmvn(global_stats, fb.compute(u)))
            assert np.abs(got["score"][at:at + len(ref)] - ref).max() <= LOGLIK_TOL
            at += len(ref)
        assert at == len(got["score"])


OPS_SHAPE = (121, 233, 17)


@pytest.mark.parametrize("word", WORDS)
def test_fresh_allocations_under_the_stand_alone_ops(torch, G, ctxs, oracle, word):
    """quantize + gemm_u8u8f32 (the scratch buffer holds their partials and
    column sums), sgemm and linear at (121, 233, 17) on a context created under
    the fill, and again behind a fill of its buffers: the oracle's bits for the
    u8 path, the clean context's bits within test_sgemm's bar for fp32."""
    m, n, k = OPS_SHAPE
    rng = np.random.default_rng(3 * m + n)
    A = rng.uniform(-0.5, 0.5, (m, k)).astype(np.float32)
    B = rng.uniform(1, 2, (k, n)).astype(np.float32)
    bias = rng.uniform(-1, 1, n).astype(np.float32)
    Ad, Bd, bd = dev(torch, A), dev(torch, B), dev(torch, bias)
    oa, sa, za = oracle.quantize(A)
    ob, sb, zb = oracle.quantize(B)
    want_u8 = oracle.gemm_u8u8f32(oa, sa, za, ob, sb, zb)
    clean = ctxs["plain"]
    want_c = G.sgemm(clean, Ad, Bd).cpu().numpy()
    want_l = G.linear(clean, Ad, Bd, bd).cpu().numpy()
    exact = A.astype(np.float64) @ B.astype(np.float64)
    assert np.abs(want_c - exact).max() <= 1e-6 * np.abs(A).sum(1).max() * 2 * k ** 0.5 + 1e-5

    def ops(ctx, what):
        qa, pa = G.quantize(ctx, Ad)
        qb, pb = G.quantize(ctx, Bd)
        assert G.params_host(pa) == (sa, za) and G.params_host(pb) == (sb, zb), what
        assert np.array_equal(qa.cpu().numpy(), oa) and np.array_equal(qb.cpu().numpy(), ob), what
        assert np.array_equal(bits(G.gemm_u8(ctx, qa, pa, qb, pb).cpu().numpy()), bits(want_u8)), what
        assert np.array_equal(G.gemm_u8(ctx, qa, pa, qb, pb, out_int32=True).cpu().numpy(),
                              oracle.gemm_u8u8_i32(oa, za, ob, zb)), what
        assert np.array_equal(bits(G.sgemm(ctx, Ad, Bd).cpu().numpy()), bits(want_c)), what
        assert np.array_equal(bits(G.linear(ctx, Ad, Bd, bd).cpu().numpy()), bits(want_l)), what

    with devfill.fresh_allocations(G, devfill.WORDS[word]):
        ctx = G.Context(0)
        ops(ctx, "fresh")
        assert devfill.fill_ctx(G, ctx, devfill.WORDS[word]) >= 1024 * 8
        ops(ctx, "filled")
        ctx.synchronize()
    ctx.close()


# ------------------------------------------------------ D. reset slots --

SESSION_MODES = ("fp32", "bf16x6", "bf16", "int8")
PUSH = 1600                                         # 100 ms
LONG = 7 * 16000                                    # 698 frames: past 600, the 610-row raw ring has wrapped
SECOND = (1, 399, 400, 1600, 0, 1600, 1600, 0)      # ragged, an empty push, the EOS on a push without samples


@pytest.fixture(scope="module")
def session_waves():
    from catears_amd import synth
    return {"first": synth.pcm(7400, LONG), "second": synth.pcm(7401, sum(SECOND)),
            "neighbour": synth.pcm(7402, LONG + PUSH * len(SECOND))}


_ONE_SHOT = {}


def one_shot(torch, G, ctx, xs_config, xs_ranges, gs, mode, name, wave):
    """ce_gpu_score of one utterance in `mode`, on a context nobody filled."""
    if (mode, name) not in _ONE_SHOT:
        model = xs_model(G, ctx, xs_config, mode, xs_ranges)
        plan = G.Plan(ctx, [len(wave)], model)
        _ONE_SHOT[mode, name] = G.score(ctx, model, plan, dev(torch, wave), gs).cpu().numpy()
        model.close()
    return _ONE_SHOT[mode, name]


def push_all(torch, sess, pieces, eos):
    """One push of {slot: samples}; returns {slot: rows}."""
    slots = sorted(pieces)
    counts = [len(pieces[k]) for k in slots]
    cat = np.concatenate([pieces[k] for k in slots])
    pcm = dev(torch, cat) if len(cat) else None
    out, n = sess.push(slots, pcm, counts, eos=[eos.get(k, False) for k in slots])
    out, at, rows = out.cpu().numpy(), 0, {}
    for k, r in zip(slots, n):
        rows[k] = out[at:at + r]
        at += r
    return rows


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("kind", ["plain", "incremental"])
@pytest.mark.parametrize("mode", SESSION_MODES)
def test_reset_slot_reads_nothing_of_its_past(torch, G, ctxs, xs_config, xs_ranges, gs, session_waves, mode, kind, word):
    """sessions_reset touches no device state.  Slot 0 streams 7 s, is reset,
    and every device region it owns is filled; its next utterance, in ragged
    pushes, gives the one-shot rows.  Slot 1 streams through all of it, in the
    same calls, and keeps its own."""
    waves = session_waves
    ref = {k: one_shot(torch, G, ctxs["plain"], xs_config, xs_ranges, gs, mode, k, w) for k, w in waves.items()}
    ctx = G.Context(0)
    model = xs_model(G, ctx, xs_config, mode, xs_ranges)
    sess = G.Sessions(ctx, model, 2, PUSH, gs, incremental=kind == "incremental")
    try:
        got = {"first": [], "second": [], "neighbour": []}
        n_long = LONG // PUSH
        for i in range(n_long):
            rows = push_all(torch, sess, {0: waves["first"][i * PUSH:(i + 1) * PUSH],
                                          1: waves["neighbour"][i * PUSH:(i + 1) * PUSH]}, {0: i == n_long - 1})
            got["first"].append(rows[0])
            got["neighbour"].append(rows[1])
        sess.reset(0)
        devfill.fill_slots(G, sess, devfill.WORDS[word], [0])
        at = 0
        for j, c in enumerate(SECOND):
            last = j == len(SECOND) - 1
            rows = push_all(torch, sess, {0: waves["second"][at:at + c],
                                          1: waves["neighbour"][LONG + j * PUSH:LONG + (j + 1) * PUSH]},
                            {0: last, 1: last})
            at += c
            got["second"].append(rows[0])
            got["neighbour"].append(rows[1])
    finally:
        sess.close()
        model.close()
        ctx.close()
    for k in ("first", "second", "neighbour"):
        rows = np.concatenate(got[k])
        assert first_diff(rows, ref[k]) is None, f"{mode} {kind} {word} {k}: {first_diff(rows, ref[k])}"


@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("kind", ["plain", "incremental"])
def test_filling_a_live_slot_does_change_its_rows(torch, G, ctxs, xs_config, xs_ranges, gs, session_waves, kind, word):
    """Teeth: the same fill on a slot in the middle of its utterance reaches
    state the slot does read -- its sample tail, its rings, its carry, its
    caches -- so its next rows are not the one-shot rows (NaN under the NaN
    word), while its neighbour, not listed, keeps its own."""
    wave, other = session_waves["first"][:3 * 16000], session_waves["neighbour"][:3 * 16000]
    ref = one_shot(torch, G, ctxs["plain"], xs_config, xs_ranges, gs, "bf16x6", "first-3s", wave)
    ref_other = one_shot(torch, G, ctxs["plain"], xs_config, xs_ranges, gs, "bf16x6", "neighbour-3s", other)
    ctx = G.Context(0)
    model = xs_model(G, ctx, xs_config, "bf16x6", xs_ranges)
    sess = G.Sessions(ctx, model, 2, PUSH, gs, incremental=kind == "incremental")
    try:
        got, got_other = [], []
        n = len(wave) // PUSH
        for i in range(n):
            if i == n // 2:
                devfill.fill_slots(G, sess, devfill.WORDS[word], [0])
            rows = push_all(torch, sess, {0: wave[i * PUSH:(i + 1) * PUSH], 1: other[i * PUSH:(i + 1) * PUSH]},
                            {0: i == n - 1, 1: i == n - 1})
            got.append(rows[0])
            got_other.append(rows[1])
    finally:
        sess.close()
        model.close()
        ctx.close()
    before = sum(len(r) for r in got[:n // 2])
    rows = np.concatenate(got)
    assert rows.shape == ref.shape and first_diff(rows[:before], ref[:before]) is None
    after = np.concatenate(got[n // 2:n // 2 + 2])
    assert len(after) and first_diff(after, ref[before:before + len(after)]) is not None
    if word == "nan":
        assert np.isnan(after).all()
    assert first_diff(np.concatenate(got_other), ref_other) is None


# -------------------------------------------------- E. per-push scratch --

@pytest.mark.parametrize("word", WORDS)
@pytest.mark.parametrize("kind", ["plain", "incremental"])
@pytest.mark.parametrize("mode", ["bf16x6", "int8"])
def test_per_push_scratch_carries_nothing(torch, G, ctxs, xs_config, xs_ranges, gs, session_waves, mode, kind, word):
    """The fbank temporary and the descriptor's device copy are filled between
    every two pushes of a three-slot set (no slot listed), and the context's
    buffers with them: every slot's rows are its one-shot rows."""
    names = ("first", "second", "neighbour")
    waves = {i: session_waves[k][:16000 + 777 * i] for i, k in enumerate(names)}
    waves[1] = session_waves["second"]
    ref = {i: one_shot(torch, G, ctxs["plain"], xs_config, xs_ranges, gs, mode, f"E{i}", w) for i, w in waves.items()}
    ctx = G.Context(0)
    model = xs_model(G, ctx, xs_config, mode, xs_ranges)
    sess = G.Sessions(ctx, model, 3, PUSH, gs, incremental=kind == "incremental")
    try:
        got = {i: [] for i in waves}
        at = 0
        while any(at < len(w) for w in waves.values()):
            live = {i: w[at:at + PUSH] for i, w in waves.items() if at < len(w)}
            rows = push_all(torch, sess, live, {i: at + PUSH >= len(waves[i]) for i in live})
            for i, r in rows.items():
                got[i].append(r)
            at += PUSH
            devfill.fill_slots(G, sess, devfill.WORDS[word], [])
            devfill.fill_ctx(G, ctx, devfill.WORDS[word])
    finally:
        sess.close()
        model.close()
        ctx.close()
    for i in waves:
        rows = np.concatenate(got[i])
        assert first_diff(rows, ref[i]) is None, f"{mode} {kind} {word} slot {i}: {first_diff(rows, ref[i])}"
