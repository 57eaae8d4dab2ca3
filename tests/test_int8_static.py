"""Calibrated static int8 (ce_gpu_quant_params_from_range,
ce_gpu_model_calibrate, ce_gpu_model_quantize_static,
ce_gpu_model_quant_params): one frozen (scale, zero point) per Linear, so
every output row depends on its own input rows only.

The oracle is restated here from oracle/pyoracle.py's public pieces
(static_oracle): per Linear, Quantize's parameters of the two-element tensor
[min, max], Quantize's elementwise step with them, MatMat_U8U8F32, bias; every
other layer through layer_forward.  Everything before a final LogSoftmax is
exact arithmetic, so the bar is bit for bit; with the LogSoftmax (a float sum
in another order) it is the project's 1e-4.
"""
import ctypes

import numpy as np
import pytest

LOGLIK_TOL = 1e-4
FLT_MIN = np.float32(np.finfo(np.float32).tiny)
FLT_MAX = np.float32(np.finfo(np.float32).max)


# ------------------------------------------------------ the restated oracle --

def fold_range(x):
    """FindMinMax of a block: seeds FLT_MAX / FLT_MIN (matrix.cc:331-345)."""
    x = np.asarray(x, np.float32)
    return np.float32(min(FLT_MAX, x.min())), np.float32(max(FLT_MIN, x.max()))


def fp32_ranges(oracle, layers, x):
    """(num_linear, 2): the range of every Linear's input in an fp32 forward
    of x (the spliced block: the same extremes as the block entering the
    Splice, whose held rows it all reads)."""
    x = np.ascontiguousarray(x, np.float32)
    out = []
    for layer in layers:
        if layer["kind"] == "linear":
            out.append(fold_range(x))
        x = oracle.layer_forward(layer, x, gemm=lambda a, W: (a @ W).astype(np.float32))
    return np.array(out, np.float32)


def central_half(ranges):
    r = np.asarray(ranges, np.float64)
    mid, quarter = (r[:, 0] + r[:, 1]) / 2, (r[:, 1] - r[:, 0]) / 4
    return np.stack([mid - quarter, mid + quarter], 1).astype(np.float32)


def static_oracle(oracle, layers, x, ranges, taps=None):
    """Nnet::Propagate with Linear i as Quantize (frozen parameters of
    ranges[i]) + MatMat_U8U8F32 + bias.  taps: list that receives every
    Linear's quantized input."""
    x = np.ascontiguousarray(x, np.float32)
    li = 0
    for layer in layers:
        if layer["kind"] != "linear":
            x = oracle.layer_forward(layer, x)
            continue
        _, s, z = oracle.quantize(np.float32([ranges[li][0], ranges[li][1]]))
        xq = oracle._quantize_with(x, s, z)
        if taps is not None:
            taps.append(xq)
        wq, sw, zw = oracle.quantize(layer["W"])
        # the float64 form is exact while the int32 accumulator cannot wrap
        k = xq.shape[1]
        small = k * (255 + abs(z)) * (255 + abs(zw)) < 2 ** 31 and 0 <= z <= 255 and 0 <= zw <= 255
        y = (oracle.gemm_u8u8f32_f64 if small else oracle.gemm_u8u8f32)(xq, s, z, wq, sw, zw)
        x = (y + np.asarray(layer["b"], np.float32)[None, :]).astype(np.float32)
        li += 1
    return x


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------- CPU ----

def _seeded_ranges():
    rng = np.random.default_rng(20250701)
    out = []
    for scale in (1e-3, 1.0, 37.0, 1e6, 1e27):
        a = (rng.normal(0.0, 1.0, 600) * scale).astype(np.float32)
        w = (np.abs(rng.normal(0.0, 1.0, 600)) * scale + scale * 1e-3).astype(np.float32)
        out += list(zip(a, (a + w).astype(np.float32)))
    neg = -(np.abs(rng.normal(0.0, 5.0, 300)) + 0.01).astype(np.float32)
    out += [(np.float32(2.0) * v, v) for v in neg]  # all negative: max becomes FLT_MIN
    out += [(np.float32(0.0), FLT_MIN), (np.float32(0.0), np.float32(0.0)), (np.float32(-1e27), np.float32(2e27)),
            (np.float32(9.5e26), np.float32(1.05e27)), (np.float32(-3.0), np.float32(0.0))]
    return [(np.float32(a), np.float32(b)) for a, b in out if a < b or b <= 0]


def test_quant_params_from_range_matches_oracle(oracle):
    """The CPU entry equals Quantize's parameter choice for a tensor holding
    just the two extremes, exactly, over a few thousand seeded ranges."""
    from catears_amd import gpu
    cases = _seeded_ranges()
    assert len(cases) > 3000
    assert any(b < 0 for _, b in cases) and any(a > 1e26 for a, _ in cases)
    for mn, mx in cases:
        _, s, z = oracle.quantize(np.float32([mn, mx]))
        gs, gz = gpu.quant_params_from_range(mn, mx)
        assert np.float32(s).view(np.uint32) == np.float32(gs).view(np.uint32) and z == gz, (mn, mx, s, z, gs, gz)
    # [0, FLT_MIN]: a denormal scale, zero point 0
    s, z = gpu.quant_params_from_range(0.0, FLT_MIN)
    assert 0 < s < FLT_MIN and z == 0
    # an all-negative range takes FindMinMax's FLT_MIN as its max
    assert gpu.quant_params_from_range(-8.0, -2.0) == gpu.quant_params_from_range(-8.0, FLT_MIN)


@pytest.mark.parametrize("mn,mx", [(float("nan"), 1.0), (0.0, float("nan")), (float("-inf"), 1.0),
                                   (0.0, float("inf")), (2.0, 1.0), (3.0, 3.0), (-3.4e38, 3.4e38)])
def test_quant_params_from_range_rejects(mn, mx):
    from catears_amd import gpu
    with pytest.raises(gpu.CatearsError) as e:
        gpu.quant_params_from_range(mn, mx)
    assert e.value.code == -2
    s, z = ctypes.c_float(), ctypes.c_int32()
    assert gpu.lib().ce_gpu_quant_params_from_range(0.0, 1.0, None, ctypes.byref(z)) == -2
    assert gpu.lib().ce_gpu_quant_params_from_range(0.0, 1.0, ctypes.byref(s), None) == -2


def test_abi_lists_the_static_int8_entries():
    from catears_amd import gpu
    for name in ("ce_gpu_quant_params_from_range", "ce_gpu_model_calibrate", "ce_gpu_model_quantize_static",
                 "ce_gpu_model_quant_params"):
        assert name in gpu.ABI and hasattr(gpu.lib(), name)
    assert b" 0.7 " in gpu.lib().ce_gpu_version()


# ------------------------------------------------------------------- GPU ----

on_gpu = pytest.mark.gpu


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


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _tdnn(hidden, pdfs, seed=3):
    from catears_amd import synth
    layers, left, right, _ = synth.tdnn_layers(hidden, pdfs, seed=seed)
    return [L for L in layers if L["kind"] != "log_softmax"], left, right


def _inputs(rows, seed):
    return np.random.default_rng(seed).normal(9.0, 3.0, size=(rows, 40)).astype(np.float32)


# (hidden, pdfs): 64 every layer pre-spliced / unfused; 128 fused, one column
# tile; 384 fused, three column tiles (a row's sum crosses blocks); 97 pdfs:
# the scalar epilogue on the last layer
NETS = [(64, 96), (128, 96), (384, 100), (128, 97)]


@pytest.fixture(scope="module")
def nets(oracle):
    """(hidden, pdfs) -> (layers, left, right, ranges): ranges from the fp32
    activations of an input the tests do not score."""
    out = {}
    for hidden, pdfs in NETS:
        layers, left, right = _tdnn(hidden, pdfs)
        out[(hidden, pdfs)] = (layers, left, right, fp32_ranges(oracle, layers, _inputs(300, 4242)))
    return out


def _static_model(G, ctx, layers, left, right, ranges):
    from catears_amd import formats
    return G.Model(ctx, image=formats.nnet_bytes(layers, left, right)).quantize_static(ctx, ranges)


@on_gpu
@pytest.mark.parametrize("rows", [21, 300, 1100])
@pytest.mark.parametrize("net", NETS)
def test_static_block_bit_exact(torch, G, ctx, oracle, nets, net, rows):
    layers, left, right, ranges = nets[net]
    model = _static_model(G, ctx, layers, left, right, ranges)
    x = _inputs(rows, rows)
    got = G.nnet_propagate(ctx, model, dev(torch, x)).cpu().numpy()
    want = static_oracle(oracle, layers, x, ranges)
    assert got.shape == want.shape == (rows - left - right, net[1])
    diff = np.flatnonzero(bits(got) != bits(want))
    assert diff.size == 0, f"{diff.size} elements differ, first at {np.unravel_index(diff[0], got.shape)}"


@on_gpu
@pytest.mark.parametrize("net", NETS)
def test_static_clamps_both_ends(torch, G, ctx, oracle, nets, net):
    """Ranges shrunk to their central half: every layer's quantized input
    holds byte 0, byte 255 and interior bytes (asserted on the oracle's bytes
    alone), and the GPU clamps to the same bits."""
    layers, left, right, ranges = nets[net]
    half = central_half(ranges)
    x = _inputs(300, 300)
    taps = []
    want = static_oracle(oracle, layers, x, half, taps)
    assert len(taps) == len(half)
    for i, q in enumerate(taps):
        assert (q == 0).any() and (q == 255).any() and ((q > 0) & (q < 255)).any(), i
    model = _static_model(G, ctx, layers, left, right, half)
    got = G.nnet_propagate(ctx, model, dev(torch, x)).cpu().numpy()
    assert same(got, want)


@on_gpu
@pytest.mark.parametrize("hidden", [64, 128])
@pytest.mark.parametrize("case", ["dead_layer", "wide_range"])
def test_static_edge_ranges(torch, G, ctx, oracle, case, hidden):
    """As test_int8_quantize_edge_ranges with frozen parameters.  dead_layer:
    a Linear whose ReLU output is all zero, so the next Linear's range is
    [0, FLT_MIN], its scale a denormal and every quotient the division
    fallback's.  wide_range: a Linear scaled by 2^90.  hidden 64: the
    quantize pass; 128: the requantize epilogue."""
    layers, left, right = _tdnn(hidden, 96)
    lin = [i for i, L in enumerate(layers) if L["kind"] == "linear"]
    i = lin[1]
    if case == "dead_layer":
        layers[i] = dict(layers[i], W=np.zeros_like(layers[i]["W"]), b=np.full_like(layers[i]["b"], -1.0))
        bn = next(j for j in range(i, len(layers)) if layers[j]["kind"] == "batchnorm")
        layers[bn] = dict(layers[bn], offset=np.zeros_like(layers[bn]["offset"]))
    else:
        layers[i] = dict(layers[i], W=(layers[i]["W"] * np.float32(2.0 ** 90)).astype(np.float32))
    ranges = fp32_ranges(oracle, layers, _inputs(300, 4242))
    if case == "dead_layer":
        assert tuple(ranges[2]) == (np.float32(0.0), FLT_MIN)
    else:
        assert ranges[2][1] > 1e26
    model = _static_model(G, ctx, layers, left, right, ranges)
    x = _inputs(300, 5)
    got = G.nnet_propagate(ctx, model, dev(torch, x)).cpu().numpy()
    want = static_oracle(oracle, layers, x, ranges)
    assert same(got, want)


@on_gpu
def test_static_row_ops_between_gemms(torch, G, ctx, oracle, nets):
    """A second BatchNorm and a ReLU behind a hidden layer's fused pair run as
    row ops of their own, so that GEMM writes fp32 and the next Linear takes
    the quantize pass, in the middle of an otherwise fused net."""
    layers, left, right, _ = nets[(128, 96)]
    bn = [i for i, L in enumerate(layers) if L["kind"] == "batchnorm"][2]
    layers = layers[:bn + 1] + [dict(layers[bn]), {"kind": "relu"}] + layers[bn + 1:]
    ranges = fp32_ranges(oracle, layers, _inputs(300, 4242))
    model = _static_model(G, ctx, layers, left, right, ranges)
    x = _inputs(300, 6)
    got = G.nnet_propagate(ctx, model, dev(torch, x)).cpu().numpy()
    assert same(got, static_oracle(oracle, layers, x, ranges))


@pytest.fixture(scope="module")
def xs_static(torch, G, ctx, xs_config):
    """TDNN-XS (hidden 256: fused) calibrated on three utterances' fbank
    features; (model, ranges)."""
    from catears_amd import synth
    m = G.Model(ctx, xs_config)
    waves = [synth.pcm(60 + i, 16000 * 3) for i in range(3)]
    plan = G.Plan(ctx, [len(w) for w in waves], m)
    feats = G.fbank(ctx, plan, dev(torch, np.concatenate(waves)))
    ranges = m.calibrate(ctx, plan, feats)
    assert ranges.shape == (m.num_linear, 2) and np.all(ranges[:, 0] < ranges[:, 1])
    return m.quantize_static(ctx, ranges), ranges


@on_gpu
def test_static_rows_do_not_depend_on_the_batch(torch, G, ctx, xs_static):
    from catears_amd import synth
    model, _ = xs_static
    waves = [synth.pcm(70 + i, n) for i, n in enumerate([16000 + 77, 24000, 32000 - 5])]
    lens = [len(w) for w in waves]
    plan = G.Plan(ctx, lens, model)
    assert plan.n_chunks == 1
    together = G.score(ctx, model, plan, dev(torch, np.concatenate(waves))).cpu().numpy()
    assert np.isfinite(together).all()
    # 256: every utterance in a chunk of its own; 128: utterances cut into
    # overlapping windows as well
    for max_rows, chunks in ((256, 3), (128, 5)):
        small = G.Plan(ctx, lens, model, max_rows=max_rows)
        assert small.n_chunks >= chunks, (max_rows, small.n_chunks)
        windowed = G.score(ctx, model, small, dev(torch, np.concatenate(waves))).cpu().numpy()
        assert same(windowed, together), max_rows
    off = plan.frame_offsets
    for u, w in enumerate(waves):
        alone = G.score(ctx, model, G.Plan(ctx, [len(w)], model), dev(torch, w)).cpu().numpy()
        assert same(alone, together[off[u]:off[u + 1]]), u


@on_gpu
def test_static_blocks_equal_each_block_alone(torch, G, ctx, xs_static):
    model, _ = xs_static
    rng = np.random.default_rng(77)
    sizes = [70, 33, 151]
    blocks = [rng.normal(9.0 + 4 * i, 1.0 + 2 * i, size=(n, 40)).astype(np.float32) for i, n in enumerate(sizes)]
    got = G.nnet_propagate_blocks(ctx, model, dev(torch, np.concatenate(blocks)), sizes).cpu().numpy()
    at = 0
    for b in blocks:
        alone = G.nnet_propagate(ctx, model, dev(torch, b)).cpu().numpy()
        assert same(got[at:at + len(alone)], alone)
        at += len(alone)
    assert at == len(got)


@on_gpu
def test_static_sessions_match_one_shot(torch, G, ctx, xs_static, global_stats):
    """Three slots, ragged pushes (0-sample pushes among them), each
    utterance's EOS, one slot reset and reused: the concatenated rows are the
    one-shot ce_gpu_score's bits, and no push allocates or frees."""
    from catears_amd import synth
    model, _ = xs_static
    gs = dev(torch, global_stats)
    waves = {0: synth.pcm(930, 16000 + 77), 1: synth.pcm(931, 9000), 2: synth.pcm(932, 24000)}
    reuse = synth.pcm(933, 8000)
    rng = np.random.default_rng(934)
    sess = G.Sessions(ctx, model, 3, 4000, gs)
    try:
        before = G.debug_counters()
        pos = {k: 0 for k in waves}
        rows = {k: [] for k in waves}
        done, reused, zero_pushes = {}, False, 0
        while waves:
            slots, counts, eos, pieces = [], [], [], []
            for k in sorted(waves):
                left = len(waves[k]) - pos[k]
                c = min(left, int(rng.choice([0, 1, 160, 399, 1600, 3000, 4000])))
                zero_pushes += c == 0
                slots.append(k), counts.append(c), eos.append(c == left)
                pieces.append(waves[k][pos[k]:pos[k] + c])
                pos[k] += c
            out, n = sess.push(slots, dev(torch, np.concatenate(pieces)), counts, eos=eos)
            out = out.cpu().numpy()
            at = 0
            for k, r, e in zip(slots, n, eos):
                rows[k].append(out[at:at + r])
                at += r
                if e:
                    wave = waves.pop(k)
                    done[(k, len(wave))] = (wave, np.concatenate(rows[k]))
                    if k == 1 and not reused:
                        reused = True
                        sess.reset(1)
                        waves[1], pos[1], rows[1] = reuse, 0, []
        assert G.debug_counters() == before
        assert zero_pushes >= 1 and reused and len(done) == 4
    finally:
        sess.close()
    for (k, _), (wave, got) in done.items():
        ref = G.score(ctx, model, G.Plan(ctx, [len(wave)], model), dev(torch, wave), gs).cpu().numpy()
        assert same(got, ref), k


@on_gpu
def test_dynamic_int8_still_refused_in_sessions(torch, G, ctx, xs_config):
    m8 = G.Model(ctx, xs_config).quantize(ctx)
    with pytest.raises(G.CatearsError) as e:
        G.Sessions(ctx, m8, 1, 1600)
    assert e.value.code == -6
    assert m8.quant_params()[0].size == 0


def _frames_to_samples(frames):
    return 400 + 160 * (frames - 1)


@pytest.fixture(scope="module")
def int_case():
    """Geometry A of tests/netgen.py as an exact-integer net and two integer
    utterances (feature rows), with every Linear's exact input range."""
    import netgen
    in_d, widths, splices, post = netgen.GEOMETRIES["A"]
    layers = netgen.int_net(in_d, widths, splices, post, netgen.WIDE, 1000)
    left, right = netgen.context(layers)
    rng = np.random.default_rng(1500)
    utts = [rng.integers(-7, 8, size=(t, in_d)).astype(np.float32) for t in (37, 64)]

    def ranges_of(us):
        r = [[FLT_MAX, FLT_MIN] for _ in widths]
        for u in us:
            block = np.concatenate([np.repeat(u[:1], left, 0), u, np.repeat(u[-1:], right, 0)], 0)
            netgen.check_exact_budget(layers, block)
            seen = []
            netgen._walk(layers, block, lambda L, a: seen.append(a) if L is not None and L["kind"] == "linear" else None)
            assert len(seen) == len(r)
            for i, a in enumerate(seen):
                mn, mx = fold_range(a.astype(np.float32))
                r[i] = [min(r[i][0], mn), max(r[i][1], mx)]
        return np.array(r, np.float32)

    return layers, utts, ranges_of


@on_gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16x6"])
def test_calibrate_returns_the_exact_ranges(torch, G, ctx, int_case, mode):
    import netgen
    layers, utts, ranges_of = int_case
    model = G.Model(ctx, image=netgen.image(layers)).set_gemm(mode)
    lens = [_frames_to_samples(len(u)) for u in utts]
    both = G.Plan(ctx, lens, model)
    assert both.total_frames == sum(len(u) for u in utts)
    got = model.calibrate(ctx, both, dev(torch, np.concatenate(utts)))
    want = ranges_of(utts)
    assert same(got, want), (got, want)
    # batch by batch: accumulate over two plans == one plan holding both
    first = model.calibrate(ctx, G.Plan(ctx, lens[:1], model), dev(torch, utts[0]))
    assert same(first, ranges_of(utts[:1]))
    second = model.calibrate(ctx, G.Plan(ctx, lens[1:], model), dev(torch, utts[1]), ranges=first)
    assert same(second, got)
    # the frozen parameters are the CPU function's
    model.quantize_static(ctx, got)
    s, z = model.quant_params()
    cpu = [G.quant_params_from_range(mn, mx) for mn, mx in got]
    assert same(s, np.array([c[0] for c in cpu], np.float32)) and list(z) == [c[1] for c in cpu]


@on_gpu
def test_static_error_paths(torch, G, ctx, oracle, nets):
    from catears_amd import formats
    layers, left, right, ranges = nets[(64, 96)]
    image = formats.nnet_bytes(layers, left, right)
    x = dev(torch, _inputs(60, 9))
    model = G.Model(ctx, image=image)
    fp32 = G.nnet_propagate(ctx, model, x).cpu().numpy()
    with pytest.raises(G.CatearsError) as e:
        model.quantize_static(ctx, ranges[:-1])
    assert e.value.code == -2
    bad = ranges.copy()
    bad[3, 1] = np.nan
    with pytest.raises(G.CatearsError) as e:
        model.quantize_static(ctx, bad)
    assert e.value.code == -2
    # unchanged: still the fp32 model, bit for bit
    assert model.quant_params()[0].size == 0
    assert same(G.nnet_propagate(ctx, model, x).cpu().numpy(), fp32)
    # static after dynamic
    dyn = G.Model(ctx, image=image).quantize(ctx)
    with pytest.raises(G.CatearsError) as e:
        dyn.quantize_static(ctx, ranges)
    assert e.value.code == -2
    # dynamic after static, and calibrating a quantized model
    model.quantize_static(ctx, ranges)
    with pytest.raises(G.CatearsError) as e:
        model.quantize(ctx)
    assert e.value.code == -2
    assert same(G.nnet_propagate(ctx, model, x).cpu().numpy(),
                static_oracle(oracle, layers, _inputs(60, 9), ranges))


@on_gpu
def test_static_tracks_fp32(torch, G, ctx, xs_config, xs_static):
    """As test_int8_tracks_fp32, same bound: calibrated on three utterances
    (xs_static), scored on three others."""
    from catears_amd import synth
    m32 = G.Model(ctx, xs_config)
    m8, _ = xs_static
    waves = [synth.pcm(50 + i, 16000 * 3) for i in range(3)]
    plan = G.Plan(ctx, [len(w) for w in waves], m32)
    pcm = dev(torch, np.concatenate(waves))
    a = G.score(ctx, m32, plan, pcm).cpu().numpy()
    b = G.score(ctx, m8, plan, pcm).cpu().numpy()
    agree = float(np.mean(a.argmax(1) == b.argmax(1)))
    print("argmax agreement with fp32:", agree)
    assert agree > 0.5, agree
    assert np.isfinite(b).all()
