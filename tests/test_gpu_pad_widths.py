"""ce_gpu_model_pad_widths on the GPU: a net of any layer width re-laid onto
padded widths runs every matrix-core mode (tests/padnet.py restates the
re-layout; tests/test_padnet.py proves on the CPU that the padded net computes
the original net's bits and which kernels each geometry reaches).

The reference of every value check is the ORIGINAL net: netgen.exact with
zero tolerance on the exact-integer nets, netgen.eval_f64 at the project's
bars on the real-valued ones.  The remaining tests pin what separates a row's
true width from its leading dimension: LogSoftmax and the prior over
num_pdfs columns, no pad column in a caller's buffer, calibration over the
true columns, sessions, the configuration key and the refusals."""
import ctypes
import functools
import subprocess

import numpy as np
import pytest

import bf16ref
import netgen
import padnet
from test_dropin import DRIVER, _load, _put, _run
from test_gpu_gemm_shapes import first_diff
from test_gpu_parity import LOGLIK_TOL, bits, dev

pytestmark = pytest.mark.gpu

MODES = {"fp32": ("plain", "fp32"), "bf16x6": ("plain", "bf16x6"), "bf16x6p": ("plain", "bf16x6p"),
         "wide": ("wide", "bf16x6"), "latency": ("latency", "bf16x6")}
SPLIT_MODES = ("bf16x6", "bf16x6p", "wide", "latency")
GEOMS = sorted(padnet.GEOMETRIES)
SENTINEL = np.float32(-12345.678)


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


def padded_model(G, ctx, layers, gemm=None, prior=None):
    """`layers` loaded (fp32: outside the envelope), then padded."""
    model = G.Model(ctx, image=netgen.image(layers), prior=prior)
    assert model.gemm == "fp32" and not netgen.x6_ok(layers)
    assert model.pad_widths(ctx) is model
    assert model.gemm == "bf16x6"
    return model.set_gemm(gemm) if gemm else model


def run(torch, G, ctx, model, x, **kw):
    return G.nnet_propagate(ctx, model, dev(torch, x), **kw).cpu().numpy()


def rows_of(geom):
    return netgen.ROWS + ((netgen.BIG_ROWS,) if geom in padnet.BIG else ())


def p1_net(seed, real=True, log_softmax=True, **kw):
    in_d, widths, splices, post = padnet.GEOMETRIES["P1"]
    if real:
        return netgen.real_net(in_d, widths, splices, post, seed, log_softmax=log_softmax)
    return netgen.int_net(in_d, widths, splices, post, netgen.WIDE, seed, log_softmax=log_softmax, **kw)


# -------------------------------------------------------------------- gate --

def test_gate(torch, G, ctxs):
    """Loaded, P1 is fp32 and refuses the plane modes; padded, it is bf16x6
    and takes every mode name.  model_info does not change."""
    ctx = ctxs["plain"]
    _, layers, x = padnet.exact_cases("P1")[0]
    model = G.Model(ctx, image=netgen.image(layers))
    info = (model.left, model.right, model.input_dim, model.num_pdfs, model.num_linear, model.num_params)
    assert model.gemm == "fp32"
    with pytest.raises(G.CatearsError, match="ENOTSUP"):
        model.set_gemm("bf16x6")
    t, p = model.padded_widths()
    assert t.tolist() == p.tolist() == [100, 100, 37]
    model.pad_widths(ctx)
    assert model.gemm == "bf16x6"
    t, p = model.padded_widths()
    assert (t.tolist(), p.tolist()) == ([100, 100, 37], padnet.PADDED_WIDTHS["P1"]) and p.tolist() == [128, 128, 40]
    v = [ctypes.c_int() for _ in range(5)]
    n = ctypes.c_int64()
    G.check(G.lib().ce_gpu_model_info(model.h, *[ctypes.byref(c) for c in v], ctypes.byref(n)))
    assert tuple(c.value for c in v) + (n.value,) == info == (3, 3, 40, 37, 3, 200 * 100 + 100 + 200 + 300 * 100 + 100 +
                                                               100 * 37 + 37 + 74)
    for name in G.GEMM_MODES:
        assert model.set_gemm(name).gemm == name
    # a second call, and a model inside the envelope: OK, nothing changed
    model.pad_widths(ctx)
    assert model.gemm == "bf16" and model.padded_widths()[1].tolist() == [128, 128, 40]
    _, a_layers, _ = netgen.exact_cases("A")[0]
    a = G.Model(ctx, image=netgen.image(a_layers)).set_gemm("bf16x6p")
    a.pad_widths(ctx)
    assert a.gemm == "bf16x6p" and a.padded_widths()[0].tolist() == a.padded_widths()[1].tolist() == [96, 800, 772]


# ------------------------------------------------------ exact-integer leg --

@functools.lru_cache(maxsize=None)
def exact_cases(geom):
    out = []
    for name, layers, x in padnet.exact_cases(geom):
        netgen.check_exact_budget(layers, x)
        want = netgen.exact(layers, x)
        want.setflags(write=False)
        out.append((name, layers, x, want))
    return out


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("geom", GEOMS)
def test_exact_integer_nets(torch, G, ctxs, geom, mode):
    flavour, gemm = MODES[mode]
    ctx = ctxs[flavour]
    failures = []
    for name, layers, x, want in exact_cases(geom):
        model = padded_model(G, ctx, layers, gemm)
        c = model.left + model.right
        for r in rows_of(geom):
            got = run(torch, G, ctx, model, x[:r + c])
            d = first_diff(got, want[:r])
            if d:
                failures.append(f"{geom} {name} {mode} rows={r} {padnet.kernels(layers, r, mode)}: {d}")
    assert not failures, "\n".join(failures)


def test_exact_integer_f16x3(torch, G):
    """A two-Linear net of odd widths under B2's recipe (every operand one
    fp16 plane, so the dropped a1b1 product is zero)."""
    ctx = G.Context(0)
    layers = netgen.int_net(40, [50, 37], [[0], [0]], [netgen.RB, ("batchnorm",)], netgen.WIDE, seed=4100)
    x = netgen.int_input(layers, netgen.ROWS[-1], 4600)
    netgen.check_exact_budget(layers, x, "f16x3")
    assert all(pairs == {(0, 0)} for pairs in netgen.census(layers, x, "f16x3"))
    want = netgen.exact(layers, x)
    model = padded_model(G, ctx, layers, "f16x3")
    assert model.padded_widths()[1].tolist() == [64, 40]
    for r in netgen.ROWS:
        got = run(torch, G, ctx, model, x[:r])
        assert first_diff(got, want[:r]) is None, f"rows={r}: {first_diff(got, want[:r])}"
    assert not ctx.overflow()


@pytest.mark.parametrize("geom", ["P1", "P2"])
def test_exact_integer_bf16(torch, G, ctxs, geom):
    """Plain bf16 with every operand in one bf16 plane (integers up to 255:
    nothing is rounded), so the mode's definition on the original net
    (bf16ref.walk) and netgen.exact are the same bits, and the padded model
    must give them."""
    in_d, widths, splices, post = padnet.GEOMETRIES[geom]
    layers = netgen.int_net(in_d, widths, splices, post, [(1, 2)] * 3, seed=4200 + GEOMS.index(geom),
                            bn_scales=(1.0, -1.0))
    x = netgen.int_input(layers, netgen.ROWS[-1], 4700)

    def one_plane(L, a, w):
        assert np.abs(a).max() <= 255 and np.abs(w).max() <= 255

    want = bf16ref.walk(layers, x, np.float64, visit=one_plane)
    assert np.array_equal(bits(want), bits(netgen.exact(layers, x)))
    ctx = ctxs["plain"]
    model = padded_model(G, ctx, layers, "bf16")
    c = model.left + model.right
    for r in netgen.ROWS:
        got = run(torch, G, ctx, model, x[:r + c])
        assert first_diff(got, want[:r]) is None, f"rows={r}: {first_diff(got, want[:r])}"


# -------------------------------------------------------- real-valued leg --

@pytest.mark.parametrize("geom", GEOMS)
def test_real_nets_vs_fp64(torch, G, ctxs, geom):
    """After LogSoftmax every fp32-class mode of the padded model is within
    1e-4 of the fp64 evaluation of the ORIGINAL net, and the split modes'
    error is of the padded fp32 mode's size (test_gpu_gemm_shapes' bars)."""
    in_d, widths, splices, post = padnet.GEOMETRIES[geom]
    seed = 5000 + GEOMS.index(geom)
    layers = netgen.real_net(in_d, widths, splices, post, seed)
    x = netgen.real_input(layers, padnet.max_rows(geom), seed + 500)
    want = netgen.eval_f64(layers, x)
    errs, outs = {}, {}
    for mode, (flavour, gemm) in MODES.items():
        model = padded_model(G, ctxs[flavour], layers, gemm)
        outs[mode] = run(torch, G, ctxs[flavour], model, x)
        assert outs[mode].shape == want.shape == (padnet.max_rows(geom), widths[-1])
        errs[mode] = float(np.abs(outs[mode] - want).max())
    print(geom, errs)
    for mode in MODES:
        assert errs[mode] <= LOGLIK_TOL, errs
    for mode in SPLIT_MODES:
        assert errs[mode] <= max(2.0 * errs["fp32"], 2e-5), errs
    assert first_diff(outs["bf16x6p"], outs["bf16x6"]) is None, first_diff(outs["bf16x6p"], outs["bf16x6"])
    assert first_diff(outs["wide"], outs["bf16x6"]) is None, first_diff(outs["wide"], outs["bf16x6"])


# ------------------------------------------------------- LogSoftmax width --

def test_log_softmax_and_prior_run_over_the_true_width(torch, G, ctxs):
    """P1 with a final LogSoftmax and a prior: the 3 pad columns of the last
    layer (+0 each, e^0 = 1) must stay out of the sum."""
    layers = p1_net(5100)
    x = netgen.real_input(layers, netgen.ROWS[-1], 5600)
    prior = netgen.prior(37, 77)
    want = netgen.eval_f64(layers, x) - np.log(prior.astype(np.float64))
    errs = {}
    for mode, (flavour, gemm) in MODES.items():
        model = padded_model(G, ctxs[flavour], layers, gemm, prior=prior)
        for r in netgen.ROWS:
            got = run(torch, G, ctxs[flavour], model, x[:r + 6], subtract_prior=True)
            assert got.shape == (r, 37)
            errs[mode, r] = float(np.abs(got - want[:r]).max())
    print(errs)
    assert max(errs.values()) <= 1e-4, errs


def test_latency_tail_of_a_padded_last_layer(torch, G, ctxs):
    """Within one 1024-row window latency mode fuses the last layer's reduce
    into the finalize; for a padded last layer it runs lat_reduce and the
    plain finalize instead.  On an exact-integer net the rows are latency
    off's, LogSoftmax and prior included.  (The last Linear is scaled by
    2^-6 -- exact, every sum stays a multiple of 2^-6 below 2^18 -- so that
    the LogSoftmax's exponentials stay finite.)"""
    layers = netgen.int_net(*padnet.GEOMETRIES["P1"], [(1, 2)] * 3, seed=5200, bn_scales=(1.0, -1.0))
    x = netgen.int_input(layers, 1018, 5700)
    netgen.check_exact_budget(layers, x)
    last = [L for L in layers if L["kind"] == "linear"][-1]
    last["W"], last["b"] = np.ldexp(last["W"], -6), np.ldexp(last["b"], -6)
    layers = layers + [{"kind": "log_softmax"}]
    prior = netgen.prior(37, 78)
    want = netgen.eval_f64(layers, x) - np.log(prior.astype(np.float64))
    assert np.all(np.isfinite(want))
    off = padded_model(G, ctxs["plain"], layers, prior=prior)
    on = padded_model(G, ctxs["latency"], layers, prior=prior)
    for r in (1, 70, 129, 1018):
        a = run(torch, G, ctxs["plain"], off, x[:r + 6], subtract_prior=True)
        b = run(torch, G, ctxs["latency"], on, x[:r + 6], subtract_prior=True)
        assert first_diff(b, a) is None, f"rows={r}: {first_diff(b, a)}"
        assert np.abs(a - want[:r]).max() <= 1e-4, r


# ------------------------------------------------------------ no pad leaks --

def guarded(torch, rows, n, n_pad):
    """(flat, view): rows x n output rows at ld = n, with one padded row
    width of sentinel behind them."""
    flat = torch.full((rows * n + n_pad,), float(SENTINEL), dtype=torch.float32, device="cuda")
    return flat, flat[:rows * n].view(rows, n)


def assert_exactly_the_rows_changed(flat, rows, n, want, what):
    host = flat.cpu().numpy()
    changed = bits(host) != bits(SENTINEL)
    assert changed[:rows * n].all() and not changed[rows * n:].any(), \
        f"{what}: {int(changed.sum())} values changed, expected exactly {rows * n}"
    assert first_diff(host[:rows * n].reshape(rows, n), want) is None, what


@pytest.mark.parametrize("mode", list(MODES) + ["bf16"])
def test_no_pad_column_reaches_a_caller_buffer(torch, G, ctxs, global_stats, mode):
    """nnet_propagate with and without a final LogSoftmax, propagate_blocks
    and score on a padded P1: exactly rows x 37 values of the caller's buffer
    change, and they are the values an unguarded call returns."""
    from catears_amd import synth
    flavour, gemm = MODES.get(mode, ("plain", "bf16"))
    ctx = ctxs[flavour]
    prior = netgen.prior(37, 79)
    for log_softmax in (True, False):
        layers = p1_net(5300, log_softmax=log_softmax)
        model = padded_model(G, ctx, layers, gemm, prior=prior)
        for r in (17, 70):
            x = dev(torch, netgen.real_input(layers, r, 5800 + r))
            want = G.nnet_propagate(ctx, model, x, subtract_prior=True).cpu().numpy()
            flat, out = guarded(torch, r, 37, 40)
            G.nnet_propagate(ctx, model, x, subtract_prior=True, out=out)
            assert_exactly_the_rows_changed(flat, r, 37, want, f"nnet_propagate rows={r} log_softmax={log_softmax}")
        blocks = [70, 33, 5]
        packed = dev(torch, np.concatenate([netgen.real_input(layers, n, 5900 + n) for n in blocks]))
        want = G.nnet_propagate_blocks(ctx, model, packed, [n + 6 for n in blocks]).cpu().numpy()
        flat, out = guarded(torch, sum(blocks), 37, 40)
        G.nnet_propagate_blocks(ctx, model, packed, [n + 6 for n in blocks], out=out)
        assert_exactly_the_rows_changed(flat, sum(blocks), 37, want, f"propagate_blocks log_softmax={log_softmax}")
    waves = [synth.pcm(5950 + i, n) for i, n in enumerate([8000, 560, 16000])]
    plan = G.Plan(ctx, [len(w) for w in waves], model, max_rows=64)
    pcm, gs = dev(torch, np.concatenate(waves)), dev(torch, global_stats)
    want = G.score(ctx, model, plan, pcm, gs).cpu().numpy()
    flat, out = guarded(torch, plan.total_frames, 37, 40)
    G.score(ctx, model, plan, pcm, gs, out=out)
    assert plan.n_chunks > 1
    assert_exactly_the_rows_changed(flat, plan.total_frames, 37, want, "score")


# ---------------------------------------------------------------- sessions --

def stream(torch, G, sess, wave, counts):
    """One slot fed counts[i] samples per push, the last push carrying the
    EOS; (rows, debug counters after every push)."""
    frames_want, rows_want = G.Sessions.schedule(sess.model.left, sess.model.right, counts, len(counts) - 1)
    pcm, at, rows, seen = dev(torch, wave), 0, [], []
    for i, c in enumerate(counts):
        out, n = sess.push([0], pcm[at:at + c], [c], eos=[i == len(counts) - 1])
        assert int(n[0]) == rows_want[i], (i, c)
        rows.append(out.cpu().numpy())
        seen.append(G.debug_counters())
        at += c
    return np.concatenate(rows), seen


@pytest.mark.parametrize("mode", ["bf16x6", "latency", "bf16"])
def test_sessions_give_the_one_shot_rows(torch, G, ctxs, global_stats, mode):
    """A padded P1-shaped model (40-dim input, prior, LogSoftmax): plain and
    incremental sets stream the rows of ce_gpu_score bit for bit at chunks of
    160, 161, 400, 1600 samples and the whole utterance, and once warm a push
    allocates nothing."""
    from catears_amd import synth
    flavour, gemm = MODES.get(mode, ("plain", "bf16"))
    ctx = ctxs[flavour]
    model = padded_model(G, ctx, p1_net(5400), gemm, prior=netgen.prior(37, 80))
    gs = dev(torch, global_stats)
    wave = synth.pcm(5450, 8000)
    plan = G.Plan(ctx, [len(wave)], model)
    ref = G.score(ctx, model, plan, dev(torch, wave), gs).cpu().numpy()
    assert ref.shape == (48, 37)
    for incremental in (False, True):
        for chunk in (160, 161, 400, 1600, 8000):
            counts = [min(chunk, len(wave) - at) for at in range(0, len(wave), chunk)]
            sess = G.Sessions(ctx, model, 1, chunk, gs, incremental=incremental)
            try:
                got, seen = stream(torch, G, sess, wave, counts)
            finally:
                sess.close()
            assert first_diff(got, ref) is None, (incremental, chunk, first_diff(got, ref))
            assert all(s == seen[min(1, len(seen) - 1)] for s in seen[1:]), (incremental, chunk, seen[1], seen[-1])


def test_reserve_covers_the_padded_widths(torch, G, global_stats):
    """tests/test_gpu_sessions.py's reserve test on a padded model: one set,
    the model switched through every mode with latency off and on; the
    workspaces grown at create (sized from the padded widths) cover them all."""
    from catears_amd import synth
    c = G.Context(0)
    m = padded_model(G, c, p1_net(5500), prior=netgen.prior(37, 81))
    gs = dev(torch, global_stats)
    pcm = dev(torch, synth.pcm(5550, 4 * 1600))
    seen = []
    sess = G.Sessions(c, m, 1, 1600, gs)
    try:
        for lat in (False, True):
            for mode in ("fp32", "bf16x6", "bf16x6p", "f16x3", "bf16"):
                c.set_latency(lat)
                m.set_gemm(mode)
                for t in range(4):
                    sess.push([0], pcm[1600 * t:1600 * (t + 1)], [1600], eos=[t == 3])
                    seen.append(G.debug_counters())
                sess.reset(0)
    finally:
        sess.close()
    assert len(seen) == 40 and seen[1] == seen[-1] and seen[1][0] > 0, (seen[1], seen[-1])


# ------------------------------------------------------------- calibration --

def test_calibrate_folds_the_true_columns_only(torch, G, ctxs):
    """An exact-integer net whose BatchNorm offsets keep every true hidden
    activation >= 1: the padded model's ranges (bf16x6 mode) are the unpadded
    model's (fp32 mode) -- a pad column would bring a minimum of 0."""
    ctx = ctxs["plain"]
    in_d, widths, splices, _ = padnet.GEOMETRIES["P1"]
    layers = netgen.int_net(in_d, widths, splices, [netgen.RB, netgen.RB, ()], netgen.WIDE, seed=5600, bn_scales=(1.0,))
    for L in layers:
        if L["kind"] == "batchnorm":
            L["offset"] = np.abs(L["offset"]) + np.float32(1.0)
    frames = [30, 7]
    feats = [netgen._ints(np.random.default_rng(5650 + i), -7, 7, (n, 40)) for i, n in enumerate(frames)]
    for f in feats:  # the block the plan builds: edge frames repeated
        netgen.check_exact_budget(layers, np.concatenate([np.repeat(f[:1], 3, 0), f, np.repeat(f[-1:], 3, 0)]))
    plain = G.Model(ctx, image=netgen.image(layers))
    padded = padded_model(G, ctx, layers)
    assert (plain.gemm, padded.gemm) == ("fp32", "bf16x6")
    plan = G.Plan(ctx, [400 + 160 * (n - 1) for n in frames], plain)
    assert plan.total_frames == sum(frames)
    d_feats = dev(torch, np.concatenate(feats))
    want = plain.calibrate(ctx, plan, d_feats)
    got = padded.calibrate(ctx, plan, d_feats)
    assert want.shape == (3, 2) and np.all(want[1:, 0] >= 1.0), want
    assert np.array_equal(bits(got), bits(want)), (got, want)
    assert np.array_equal(bits(padded.set_gemm("fp32").calibrate(ctx, plan, d_feats)), bits(want))


# ---------------------------------------------------------------- refusals --

def test_quantize_and_padding_exclude_each_other(torch, G, ctxs):
    ctx = ctxs["plain"]
    _, layers, x = padnet.exact_cases("P1")[0]
    ranges = np.array([[-7.0, 7.0], [-100.0, 100.0], [-100.0, 100.0]], np.float32)
    model = padded_model(G, ctx, layers)
    before = run(torch, G, ctx, model, x[:23])
    with pytest.raises(G.CatearsError, match="EINVAL"):
        model.quantize(ctx)
    with pytest.raises(G.CatearsError, match="EINVAL"):
        model.quantize_static(ctx, ranges)
    assert model.gemm == "bf16x6" and first_diff(run(torch, G, ctx, model, x[:23]), before) is None
    for quantize in (lambda m: m.quantize(ctx), lambda m: m.quantize_static(ctx, ranges)):
        m8 = quantize(G.Model(ctx, image=netgen.image(layers)))
        with pytest.raises(G.CatearsError, match="EINVAL"):
            m8.pad_widths(ctx)
        assert m8.padded_widths()[1].tolist() == [100, 100, 37]


def test_an_unfused_row_op_is_not_supported(torch, G, ctxs):
    """A second BatchNorm behind a Linear stays a row op of its own: ENOTSUP,
    and the model scores as before."""
    ctx = ctxs["plain"]
    _, layers, x = padnet.exact_cases("P1")[0]
    at = next(i for i, L in enumerate(layers) if L["kind"] == "batchnorm")
    layers = layers[:at + 1] + [{"kind": "batchnorm", "scale": np.ones(100, np.float32),
                                 "offset": np.ones(100, np.float32)}] + layers[at + 1:]
    model = G.Model(ctx, image=netgen.image(layers))
    before = run(torch, G, ctx, model, x[:23])
    with pytest.raises(G.CatearsError, match="ENOTSUP"):
        model.pad_widths(ctx)
    assert model.gemm == "fp32" and model.padded_widths()[1].tolist() == [100, 100, 37]
    assert first_diff(run(torch, G, ctx, model, x[:23]), before) is None
    assert first_diff(before, netgen.exact(layers, x[:23])) is None


# ------------------------------------------------------------------ config --

@pytest.fixture(scope="module")
def p1_files(tmp_path_factory):
    """A P1-shaped real model on disk: (directory, layers, prior, config text
    without this implementation's own keys)."""
    from catears_amd import formats
    d = tmp_path_factory.mktemp("p1")
    layers = p1_net(5700)
    prior = netgen.prior(37, 82)
    (d / "p1.nnet").write_bytes(netgen.image(layers))
    (d / "p1.prior").write_bytes(formats.vec_bytes(prior))
    (d / "p1.tid2pdf").write_bytes(formats.vec_bytes(np.arange(5, dtype=np.int32), np.int32))
    (d / "p1.ranges").write_bytes(formats.vec_bytes(np.array([-9, 9, -9, 9, -9, 9], np.float32)))
    base = (f"nnet = {d / 'p1.nnet'}\nprior = {d / 'p1.prior'}\ntid2pdf = {d / 'p1.tid2pdf'}\nleft_context = 3\n"
            "right_context = 3\nnum_pdfs = 37\n")
    return d, layers, prior, base


def write_conf(d, name, base, chunk, extra):
    p = d / name
    p.write_text(base + f"chunk_size = {chunk}\n" + extra)
    return p


def load_fails(G, ctx, conf):
    h = ctypes.c_void_p(1)
    rc = G.lib().ce_gpu_model_load_config(ctx.h, str(conf).encode(), ctypes.byref(h))
    assert not h.value
    return rc, G.lib().ce_gpu_last_error().decode()


def test_load_config_key(torch, G, ctxs, p1_files):
    d, layers, prior, base = p1_files
    ctx = ctxs["plain"]
    x = netgen.real_input(layers, 70, 5750)
    m = G.Model(ctx, str(write_conf(d, "ok.conf", base, 50, "gpu_pad_widths = 1\ngpu_gemm = bf16\n")))
    assert m.gemm == "bf16" and m.padded_widths()[1].tolist() == [128, 128, 40] and m.num_pdfs == 37
    want = run(torch, G, ctx, padded_model(G, ctx, layers, "bf16", prior=prior), x, subtract_prior=True)
    assert first_diff(run(torch, G, ctx, m, x, subtract_prior=True), want) is None
    # 0 keeps the model as loaded: gpu_gemm = bf16 is then refused, as without the key
    assert G.Model(ctx, str(write_conf(d, "zero.conf", base, 50, "gpu_pad_widths = 0\n"))).gemm == "fp32"
    rc, msg = load_fails(G, ctx, write_conf(d, "zero16.conf", base, 50, "gpu_pad_widths = 0\ngpu_gemm = bf16\n"))
    assert rc == -6 and "gpu_gemm" in msg, (rc, msg)
    rc, msg = load_fails(G, ctx, write_conf(d, "two.conf", base, 50, "gpu_pad_widths = 2\n"))
    assert rc == -2 and "gpu_pad_widths" in msg and "2" in msg, (rc, msg)
    rc, msg = load_fails(G, ctx, write_conf(d, "both.conf", base, 50,
                                            f"gpu_pad_widths = 1\ngpu_int8_ranges = {d / 'p1.ranges'}\n"))
    assert rc == -2 and "gpu_pad_widths" in msg and "gpu_int8_ranges" in msg, (rc, msg)


@pytest.mark.parametrize("chunk", [7, 50])
def test_am_read_key_gives_the_c_abi_rows(torch, G, ctxs, tmp_path, p1_files, chunk):
    """The drop-in AcousticModel::Read applies gpu_pad_widths before gpu_gemm:
    its streamed chunks (latency mode on by default, and off with two batched
    streams) are the C-ABI model's rows of the whole padded utterance."""
    d, layers, prior, base = p1_files
    ctx = ctxs["plain"]
    feats = netgen.real_input(layers, 200, 5760)[3:-3]
    block = np.concatenate([np.repeat(feats[:1], 3, 0), feats, np.repeat(feats[-1:], 3, 0)])
    want = run(torch, G, ctx, padded_model(G, ctx, layers, "bf16", prior=prior), block, subtract_prior=True)
    x = _put(tmp_path, "x.f32", feats)
    for i, extra in enumerate(("", "gpu_latency_mode = 0\ngpu_batch_streams = 2\n")):
        conf = write_conf(tmp_path, f"am{i}.conf", base, chunk, "gpu_pad_widths = 1\ngpu_gemm = bf16\n" + extra)
        out = tmp_path / f"am{i}.bin"
        _run("am", conf, x, len(feats), out)
        got = _load(out)
        assert got.shape == want.shape == (200, 37)
        assert first_diff(got, want) is None, first_diff(got, want)


def test_am_read_refuses_bad_values(tmp_path, p1_files):
    d, layers, prior, base = p1_files
    x = _put(tmp_path, "x.f32", np.zeros((10, 40), np.float32))
    for name, extra, words in (("two", "gpu_pad_widths = 2\n", ("gpu_pad_widths", "2")),
                               ("both", f"gpu_pad_widths = 1\ngpu_int8_ranges = {d / 'p1.ranges'}\n",
                                ("gpu_pad_widths", "gpu_int8_ranges"))):
        conf = write_conf(tmp_path, f"{name}.conf", base, 50, extra)
        r = subprocess.run([DRIVER, "am", str(conf), str(x), "10", str(tmp_path / "o.bin")], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode != 0
        assert all(w in r.stdout + r.stderr for w in words), r.stderr[-2000:]
        assert not (tmp_path / "o.bin").exists()
