"""The plain bf16 GEMM mode (CE_GPU_GEMM_BF16, kernels/gemm_bf16.hip) on the
GPU.  tests/bf16ref.py restates the definition; tests/test_gemm_bf16.py proves
on the CPU that its fp64 walk is a zero-tolerance oracle for the exact leg.

Exact leg: every exact-integer case, bit for bit, over both tile shapes, odd
K-tile counts and ragged widths.

Real-valued leg: one Linear against the fp64 walk at the project's bar for
split modes; whole nets against the spread of three CPU evaluations of the
same definition (a last-place difference in a hidden y can flip bf16(y), so
no tolerance is fixed in advance); bit-for-bit invariance to the row block,
the plan, the context's latency / wide-tile settings; sessions; the gpu_gemm
configuration key; refusals."""
import ctypes
import functools
import subprocess

import numpy as np
import pytest

import bf16ref
import netgen
from test_dropin import DRIVER, _am_config, _load, _put, _run
from test_gpu_gemm_shapes import first_diff
from test_gpu_parity import bits, dev

pytestmark = pytest.mark.gpu

EXACT_GEOMS = ("A", "B", "C", "D", "F4100", "G9", "G20", "G25")


def exact_params():
    """(geometry, output rows) of the exact leg: rows 1 / 17 / 70 / 129, plus
    3000 for netgen's BIG geometries."""
    return [(g, r) for g in EXACT_GEOMS
            for r in netgen.ROWS + ((netgen.BIG_ROWS,) if g in netgen.BIG else ())]


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


def bf16_model(G, ctx, layers, prior=None):
    model = G.Model(ctx, image=netgen.image(layers), prior=prior)
    assert model.gemm == "bf16x6"          # never a default
    model.set_gemm("bf16")
    assert model.gemm == "bf16"
    return model


def run(torch, G, ctx, model, x, **kw):
    return G.nnet_propagate(ctx, model, dev(torch, x), **kw).cpu().numpy()


# ------------------------------------------------------ exact-integer leg --

@functools.lru_cache(maxsize=None)
def exact_cases(geom):
    out = []
    for name, layers, x in netgen.one_plane_mode_cases(geom):
        want = bf16ref.walk(layers, x, np.float64)
        want.setflags(write=False)
        out.append((name, layers, x, want))
    return out


def test_exact_params_reach_every_tile_variant():
    seen = set()
    for geom, rows in exact_params():
        seen.update(bf16ref.tiles(netgen.exact_cases(geom)[0][1], rows))
    for shape in ("b16_32x32", "b16_128x128"):
        assert any(s == shape and kt % 2 == 1 for s, kt, _ in seen), shape
        assert any(s == shape and kt % 2 == 0 for s, kt, _ in seen), shape
        assert any(s == shape and n % 128 != 0 for s, _, n in seen), shape
    assert {36, 100, 772, 1028, 4100} <= {n for _, _, n in seen}


@pytest.mark.parametrize("geom", EXACT_GEOMS)
def test_exact_integer_nets(torch, G, ctx, geom):
    failures = []
    for name, layers, x, want in exact_cases(geom):
        model = bf16_model(G, ctx, layers)
        c = model.left + model.right
        for g, r in exact_params():
            if g != geom:
                continue
            got = run(torch, G, ctx, model, x[:r + c])
            d = first_diff(got, want[:r])
            if d:
                failures.append(f"{geom} {name} rows={r} {bf16ref.tiles(layers, r)}: {d}")
    assert not failures, "\n".join(failures)


def test_b2_equals_bf16x6(torch, G, ctx):
    """B2's operands fit one bf16 plane: nothing is rounded, so the mode gives
    bf16x6's bits."""
    (name, layers, x), = netgen.exact_cases("B2")
    model = G.Model(ctx, image=netgen.image(layers))
    c = model.left + model.right
    for r in netgen.ROWS:
        x6 = run(torch, G, ctx, model.set_gemm("bf16x6"), x[:r + c])
        b16 = run(torch, G, ctx, model.set_gemm("bf16"), x[:r + c])
        assert first_diff(b16, x6) is None, first_diff(b16, x6)
        assert first_diff(b16, netgen.exact(layers, x)[:r]) is None


# -------------------------------------------------------- real-valued leg --

ONE_LINEAR = {200: (40, netgen.S5), 800: (160, netgen.S5), 3072: (1024, [-1, 0, 2])}


@pytest.mark.parametrize("n", [96, 772])
@pytest.mark.parametrize("k", sorted(ONE_LINEAR))
def test_one_linear_vs_fp64_walk(torch, G, ctx, k, n):
    """One Linear, no rounding cascade: the GPU and the fp64 walk round the
    same operands, so they differ by the fp32 accumulation order alone.  Bar:
    the project's rule for split modes, max(2 x the fp32 mode's error against
    fp64 on the same net, 2e-5)."""
    in_dim, splice = ONE_LINEAR[k]
    layers = netgen.real_net(in_dim, [n], [splice], [()], seed=3000 + k + n, log_softmax=False)
    assert netgen.linears(layers)[0]["k"] == k
    x = netgen.real_input(layers, 129, 3500 + k + n)
    want = bf16ref.walk(layers, x, np.float64)
    model = G.Model(ctx, image=netgen.image(layers))
    fp32_err = float(np.abs(run(torch, G, ctx, model.set_gemm("fp32"), x) - netgen.eval_f64(layers, x)).max())
    got = run(torch, G, ctx, model.set_gemm("bf16"), x)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"K={k} n={n}: bf16 vs fp64 walk {err:.3g}, fp32 mode vs fp64 {fp32_err:.3g}")
    assert got.shape == want.shape
    assert err <= max(2.0 * fp32_err, 2e-5), (err, fp32_err)
    # and it is the bf16 mode: far from the unrounded net
    assert np.abs(got - netgen.eval_f64(layers, x)).max() > 100 * err


def whole_net(which):
    from catears_amd import synth
    if which in synth.MODELS:
        spec = synth.MODELS[which]
        layers, left, right, _ = synth.tdnn_layers(spec["hidden"], spec["pdfs"])
        x = np.random.default_rng(4000 + spec["hidden"]).normal(0.0, 1.0, size=(300 + left + right, 40))
        return layers, x.astype(np.float32)
    in_d, widths, splices, post = netgen.GEOMETRIES[which]
    seed = 2000 + sorted(netgen.GEOMETRIES).index(which)
    layers = netgen.real_net(in_d, widths, splices, post, seed)
    return layers, netgen.real_input(layers, 300, seed + 500)


@pytest.mark.parametrize("which", ["tdnn-xs", "tdnn-s", "A", "C", "D"])
def test_whole_nets_within_the_spread_of_the_definition(torch, G, ctx, which):
    """Three CPU evaluations of the definition (fp32 accumulation on K
    ascending, on K reversed, fp64) disagree with each other wherever a
    last-place difference flips a bf16(y).  Their pairwise spread D on the
    input being scored sets the bar: p99.9 |GPU - fp64 walk| <= 2 p99.9(D) and
    max <= 4 max(D) (the MFMA's order is a fourth order, and the maximum of a
    flip-driven error is heavy-tailed)."""
    layers, x = whole_net(which)
    w64 = bf16ref.walk(layers, x, np.float64)
    w32a = bf16ref.walk(layers, x, np.float32)
    w32d = bf16ref.walk(layers, x, np.float32, k_reversed=True)
    D = np.concatenate([np.abs(a - b).ravel() for a, b in ((w64, w32a), (w64, w32d), (w32a, w32d))])
    d_max, d_p999 = float(D.max()), float(np.quantile(D, 0.999))
    model = bf16_model(G, ctx, layers)
    got = run(torch, G, ctx, model, x).astype(np.float64)
    assert got.shape == w64.shape == (300, netgen.linears(layers)[-1]["n"])
    e = np.abs(got - w64)
    e_max, e_p999 = float(e.max()), float(np.quantile(e, 0.999))
    agree = float((got.argmax(axis=1) == w64.argmax(axis=1)).mean())
    far = float(np.abs(got - netgen.eval_f64(layers, x)).max())
    print(f"{which}: |GPU - fp64 walk| max {e_max:.3g} p99.9 {e_p999:.3g}; spread D max {d_max:.3g} "
          f"p99.9 {d_p999:.3g}; argmax agreement {agree:.4f}; |GPU - unrounded fp64| max {far:.3g}")
    assert d_max > 0.0
    assert e_p999 <= 2.0 * d_p999, (e_p999, d_p999)
    assert e_max <= 4.0 * d_max, (e_max, d_max)


BLOCKS = [70, 33, 151]


def test_row_block_invariance(torch, G, ctx):
    """A row scored alone, with one more row, in blocks of 70 / 33 / 151 and
    inside a 3000-row block carries the same bits -- across the tile switch."""
    in_d, widths, splices, post = netgen.GEOMETRIES["A"]
    layers = netgen.real_net(in_d, widths, splices, post, 2100)
    x = netgen.real_input(layers, netgen.BIG_ROWS, 2600)
    assert {s for s, _, _ in bf16ref.tiles(layers, netgen.BIG_ROWS)} == {"b16_32x32", "b16_128x128"}
    assert {s for s, _, _ in bf16ref.tiles(layers, 151)} == {"b16_32x32"}
    model = bf16_model(G, ctx, layers)
    c = model.left + model.right
    big = run(torch, G, ctx, model, x)
    assert big.shape == (netgen.BIG_ROWS, widths[-1]) and np.all(np.isfinite(big))
    for r in (1, 2, 70, 71):
        part = run(torch, G, ctx, model, x[:r + c])
        assert first_diff(part, big[:r]) is None, (r, first_diff(part, big[:r]))
    starts = np.concatenate([[0], np.cumsum(BLOCKS)])
    packed = np.concatenate([x[s:s + n + c] for s, n in zip(starts, BLOCKS)])
    blocks = G.nnet_propagate_blocks(ctx, model, dev(torch, packed), [n + c for n in BLOCKS]).cpu().numpy()
    assert first_diff(blocks, big[:sum(BLOCKS)]) is None, first_diff(blocks, big[:sum(BLOCKS)])
    # latency mode and wide tiles are ignored in this mode: the same bits
    for flavour in ("latency", "wide"):
        c2 = G.Context(0)
        c2.set_latency(True) if flavour == "latency" else c2.set_wide_tiles(True)
        m2 = bf16_model(G, c2, layers)
        for r in (70, netgen.BIG_ROWS):
            other = run(torch, G, c2, m2, x[:r + c])
            assert first_diff(other, big[:r]) is None, (flavour, r, first_diff(other, big[:r]))


@pytest.fixture(scope="module")
def xs_bf16(G, ctx, xs_config):
    return G.Model(ctx, xs_config).set_gemm("bf16")


def test_plan_max_rows_invariance(torch, G, ctx, xs_bf16, global_stats):
    from catears_amd import synth
    waves = [synth.pcm(700 + i, n) for i, n in enumerate([48000, 16000, 560, 100000])]
    pcm, gs = dev(torch, np.concatenate(waves)), dev(torch, global_stats)
    outs = []
    for max_rows in (4096, 512):
        plan = G.Plan(ctx, [len(w) for w in waves], xs_bf16, max_rows=max_rows)
        outs.append(G.score(ctx, xs_bf16, plan, pcm, gs).cpu().numpy())
    assert outs[0].shape[0] == sum(G.num_frames(len(w)) for w in waves)
    assert first_diff(outs[1], outs[0]) is None, first_diff(outs[1], outs[0])


def test_sessions_give_the_one_shot_rows(torch, G, ctx, xs_config, xs_bf16, global_stats):
    """TDNN-XS, three slots, chunks of 777 and 1600 samples, with CMVN: the
    streamed rows are ce_gpu_score's in bf16 mode, and warm pushes allocate
    nothing."""
    from catears_amd import synth
    from test_gpu_sessions import check_jobs, run_jobs
    gs = dev(torch, global_stats)
    jobs = {0: [(synth.pcm(710, 24000), 777)], 1: [(synth.pcm(711, 32000), 1600)],
            2: [(synth.pcm(712, 16000), 777), (synth.pcm(713, 12000), 1600)]}
    sess = G.Sessions(ctx, xs_bf16, 3, 1600, gs)
    seen = {}

    def on_tick(t):
        seen[t] = G.debug_counters()
    try:
        got = run_jobs(torch, G, sess, jobs, on_tick=on_tick)
    finally:
        sess.close()
    ticks = sorted(seen)
    assert len(ticks) >= 20 and all(seen[t] == seen[2] for t in ticks[1:]), seen
    check_jobs(torch, G, ctx, xs_bf16, gs, jobs, got)
    # the reference of check_jobs is this mode's one-shot score, which differs from bf16x6's
    m6 = G.Model(ctx, xs_config)
    wave = jobs[0][0][0]
    plan = G.Plan(ctx, [len(wave)], m6)
    x6 = G.score(ctx, m6, plan, dev(torch, wave), gs).cpu().numpy()
    assert x6.shape == got[(0, 0)].shape and not np.array_equal(bits(x6), bits(got[(0, 0)]))
    assert np.abs(x6 - got[(0, 0)]).max() < 0.1


# ------------------------------------------------------------------ config --

@pytest.fixture(scope="module")
def utterance(torch, G, ctx, oracle, xs_config, xs_bf16):
    """Features of one utterance, the block AcousticModel pads it to, and its
    rows in bf16 mode through Python."""
    from catears_amd import formats, synth
    feats = oracle.Fbank().compute(synth.pcm(5, 16000 * 2 + 123))
    am = formats.read_am(xs_config)
    block = np.concatenate([np.repeat(feats[:1], am["left"], 0), feats, np.repeat(feats[-1:], am["right"], 0)], 0)
    want = run(torch, G, ctx, xs_bf16, block, subtract_prior=True)
    x6 = run(torch, G, ctx, G.Model(ctx, xs_config), block, subtract_prior=True)
    assert want.shape == (len(feats), am["num_pdfs"]) and not np.array_equal(bits(want), bits(x6))
    return {"feats": feats, "block": block, "want": want}


def test_load_config_key(torch, G, ctx, tmp_path, xs_config, utterance):
    conf = _am_config(tmp_path, xs_config, 50, extra="gpu_gemm = bf16\n")
    m = G.Model(ctx, str(conf))
    assert m.gemm == "bf16"
    got = run(torch, G, ctx, m, utterance["block"], subtract_prior=True)
    assert first_diff(got, utterance["want"]) is None
    bad = _am_config(tmp_path, xs_config, 7, extra="gpu_gemm = bogus\n")
    h = ctypes.c_void_p(1)
    rc = G.lib().ce_gpu_model_load_config(ctx.h, str(bad).encode(), ctypes.byref(h))
    assert rc == -2 and not h.value
    msg = G.lib().ce_gpu_last_error().decode()
    assert "gpu_gemm" in msg and "bogus" in msg, msg


def test_load_config_key_refuses_a_program_that_cannot_run_it(G, ctx, tmp_path):
    """Geometry E is not an x6 program: gpu_gemm = bf16 is CE_GPU_ENOTSUP,
    gpu_gemm = fp32 loads."""
    from catears_amd import formats
    in_d, widths, splices, post = netgen.GEOMETRIES["E"]
    layers = netgen.real_net(in_d, widths, splices, post, 9)
    left, right = netgen.context(layers)
    (tmp_path / "e.nnet").write_bytes(netgen.image(layers))
    (tmp_path / "e.prior").write_bytes(formats.vec_bytes(netgen.prior(widths[-1], 3)))
    (tmp_path / "e.tid2pdf").write_bytes(formats.vec_bytes(np.arange(5, dtype=np.int32), np.int32))
    for name, rc_want in (("bf16", -6), ("fp32", 0)):
        conf = tmp_path / f"e_{name}.conf"
        conf.write_text(f"nnet = e.nnet\nprior = e.prior\ntid2pdf = e.tid2pdf\nleft_context = {left}\n"
                        f"right_context = {right}\nchunk_size = 50\nnum_pdfs = {widths[-1]}\ngpu_gemm = {name}\n")
        h = ctypes.c_void_p()
        rc = G.lib().ce_gpu_model_load_config(ctx.h, str(conf).encode(), ctypes.byref(h))
        assert rc == rc_want, (name, rc, G.lib().ce_gpu_last_error())
        if rc == 0:
            G.lib().ce_gpu_model_destroy(h)
        else:
            msg = G.lib().ce_gpu_last_error().decode()
            assert not h.value and "gpu_gemm" in msg and "bf16" in msg, msg


@pytest.mark.parametrize("chunk", [7, 50])
def test_am_config_key_gives_the_bf16_rows(tmp_path, xs_config, utterance, chunk):
    """The drop-in AcousticModel::Read applies gpu_gemm; its streamed chunks
    are the rows of the whole padded utterance (rows do not depend on the
    block), with latency mode on (the drop-in's default) and off."""
    feats, want = utterance["feats"], utterance["want"]
    x = _put(tmp_path, "x.f32", feats)
    for extra in ("gpu_gemm = bf16\n", "gpu_gemm = bf16\ngpu_latency_mode = 0\ngpu_batch_streams = 2\n"):
        out = tmp_path / "am.bin"
        _run("am", _am_config(tmp_path, xs_config, chunk, extra=extra), x, len(feats), out)
        got = _load(out)
        assert got.shape == want.shape
        diff = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
        assert diff.size == 0, f"{diff.size} frames differ, first {diff[0]}"


def test_am_read_refuses_an_unknown_mode(tmp_path, xs_config, utterance):
    conf = _am_config(tmp_path, xs_config, 50, extra="gpu_gemm = bogus\n")
    x = _put(tmp_path, "x.f32", utterance["feats"])
    r = subprocess.run([DRIVER, "am", str(conf), str(x), str(len(utterance["feats"])), str(tmp_path / "o.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "gpu_gemm" in r.stdout + r.stderr and "bogus" in r.stdout + r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "o.bin").exists()


def test_int8_ranges_win_over_gpu_gemm(torch, G, ctx, tmp_path, xs_config, utterance):
    """Together with gpu_int8_ranges the key is accepted and has no effect."""
    from catears_amd import formats, synth
    m = G.Model(ctx, xs_config)
    waves = [synth.pcm(60 + i, 16000 * 2) for i in range(2)]
    plan = G.Plan(ctx, [len(w) for w in waves], m)
    ranges = m.calibrate(ctx, plan, G.fbank(ctx, plan, dev(torch, np.concatenate(waves))))
    (tmp_path / "r.vec0").write_bytes(formats.vec_bytes(ranges.reshape(-1)))
    outs = []
    for extra in ("", "gpu_gemm = bf16\n"):
        conf = _am_config(tmp_path, xs_config, 50 if extra else 51, extra=f"gpu_int8_ranges = {tmp_path / 'r.vec0'}\n" + extra)
        m8 = G.Model(ctx, str(conf))
        assert m8.quant_params()[0].size == m8.num_linear
        outs.append(run(torch, G, ctx, m8, utterance["block"], subtract_prior=True))
    assert first_diff(outs[1], outs[0]) is None


# ---------------------------------------------------------------- refusals --

def test_calibrate_refuses_the_mode(torch, G, ctx, xs_bf16):
    from catears_amd import synth
    wave = synth.pcm(61, 16000)
    plan = G.Plan(ctx, [len(wave)], xs_bf16)
    feats = G.fbank(ctx, plan, dev(torch, wave))
    with pytest.raises(G.CatearsError, match="ENOTSUP"):
        xs_bf16.calibrate(ctx, plan, feats)


def test_set_gemm_refuses_a_program_off_the_planes(G, ctx):
    (name, layers, x), = [c for c in netgen.exact_cases("E") if c[0] == "wide"]
    assert not netgen.x6_ok(layers)
    model = G.Model(ctx, image=netgen.image(layers))
    with pytest.raises(G.CatearsError, match="ENOTSUP"):
        model.set_gemm("bf16")
    assert model.gemm == "fp32"
    assert G.lib().ce_gpu_model_set_gemm(model.h, 5) == -2
