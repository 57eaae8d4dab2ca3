"""Static int8 on the GPU with row steps that write the next Linear's bytes
(rowop_chain_kernel's byte form, kernels/rowops.hip; run_steps_i8_static).

Every bar is bit for bit and derived: the byte is qbyte's one definition
(csrc/i8_ops.h) applied to fp32 values the existing chain kernel gives bit for
bit, the row sum an integer sum.  The kernel alone is held against the fp32
chain (ce_gpu_debug_rowop_chain) followed by the oracle's Quantize; whole nets
against tests/i8rowref.py; a final LogSoftmax (a float sum in another order)
against the project's 1e-4."""
import functools

import numpy as np
import pytest

import i8rowref
import netgen
import quantties
import rownet
from test_gpu_gemm_shapes import first_diff
from test_gpu_parity import LOGLIK_TOL, bits, dev

pytestmark = pytest.mark.gpu


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
    c = {"plain": G.Context(0), "latency": G.Context(0)}
    c["latency"].set_latency(True)
    return c


# ---------------------------------------------------------- the kernel alone --

WIDTHS = (128, 384, 1152, 4224)   # NJ = 4, 16, 64 columns per lane, and the loop kernel
CHAINS = [(), ("normalize",), ("relu", "normalize"), ("batchnorm", "relu", "normalize"),
          ("relu", "batchnorm", "relu", "normalize")]
# [3, 9]: a zero point outside [0, 255] (the reference does not clamp it); [0, 510]: scale 2, so
# the odd integers of the input sit on n + 0.5 ties
RANGES = [(-4.0, 4.0), (0.0, 1.5), (3.0, 9.0), (0.0, 510.0)]
Q_FILL, RS_FILL, ZERO_FILL = 0x55, 123456, -7


def kernel_rows(dim, rows, seed):
    """Seeded normals with values that clamp at both ends and odd integers
    (byte ties under scale 2) among them; BatchNorm vectors."""
    rng = np.random.default_rng(9100 + dim + seed)
    x = rng.normal(0.0, 2.0, size=(rows, dim)).astype(np.float32)
    x[:, 3::17] = rng.integers(-3, 260, size=x[:, 3::17].shape) * 2 + 1
    x[:, 5::31] = 1e4
    x[:, 6::31] = -1e4
    vec = [(rng.normal(1.0, 0.2, dim).astype(np.float32), rng.normal(0.0, 0.3, dim).astype(np.float32))
           for _ in range(4)]
    return x, vec


def run_q(torch, G, ctx, chain, x, dvec, s, z, pad):
    """One launch of the byte form on a copy of x; (bytes of every row of the
    buffer, row sums, cleared words, the fp32 rows afterwards)."""
    rows, dim = x.shape
    src = dev(torch, x)
    q = torch.full((rows + 2, dim + pad), Q_FILL, dtype=torch.int8, device="cuda")
    rs = torch.full((rows + 3,), RS_FILL, dtype=torch.int32, device="cuda")
    zero = torch.full((rows + 3,), ZERO_FILL, dtype=torch.int32, device="cuda")
    G.debug_rowop_chain_q(ctx, chain, src, s, z, q[:rows], rs, zero, vectors=dvec)
    return q.cpu().numpy(), rs.cpu().numpy(), zero.cpu().numpy(), src.cpu().numpy()


def check_q(got, want_bytes, rows, dim, pad, what):
    q, rs, zero, _ = got
    assert np.array_equal(q[:rows, :dim], want_bytes), (what, first_diff(q[:rows, :dim].astype(np.float32),
                                                                          want_bytes.astype(np.float32)))
    assert np.all(q[:rows, dim:] == 0), (what, "pad bytes")
    assert np.all(q[rows:] == Q_FILL), (what, "wrote behind the last row")
    assert np.array_equal(rs[:rows], want_bytes.astype(np.int32).sum(axis=1)), (what, "row sums")
    assert np.all(rs[rows:] == RS_FILL), (what, "row sums behind the last row")
    assert np.all(zero[:rows] == 0) and np.all(zero[rows:] == ZERO_FILL), (what, "cleared words")


@pytest.mark.parametrize("dim", WIDTHS)
def test_kernel_matches_chain_then_quantize(torch, G, ctxs, oracle, dim):
    ctx = ctxs["plain"]
    spans = []
    for rows in (1, 5):   # 5: one full block of four waves and a partial one
        x, vec = kernel_rows(dim, rows, rows)
        dvec = [(dev(torch, s), dev(torch, o)) for s, o in vec]
        for chain in CHAINS:
            f32 = G.rowop_chain(ctx, list(chain), dev(torch, x), vectors=dvec).cpu().numpy()
            assert np.all(np.isfinite(f32))
            for mn, mx in RANGES:
                s, z = G.quant_params_from_range(mn, mx)
                want = (oracle._quantize_with(f32, s, z).astype(np.int16) - 128).astype(np.int8)
                u = want.astype(np.int16) + 128
                spans.append(u.min() == 0 and u.max() == 255 and bool(np.any((u > 0) & (u < 255))))
                if not chain and (mn, mx) == (0.0, 510.0):
                    assert s == 2.0 and z == 0 and np.any((f32 / 2) % 1 == 0.5)
                for pad in (0, 64):
                    got = run_q(torch, G, ctx, list(chain), x, dvec, s, z, pad)
                    check_q(got, want, rows, dim, pad, (dim, rows, chain, (mn, mx), pad))
                    if dim <= 4096:   # beyond, the fp32 rows are working memory
                        assert np.array_equal(bits(got[3]), bits(x)), (dim, chain, "the fp32 rows changed")
    # under some of the parameters the bytes clamp at both ends and lie between
    assert any(spans)


def emulated_bytes(values, s, z):
    """qbyte of fp32 values by tests/quantties.py's exact emulation of the
    kernels' quotient (Inf included: both clamps are comparisons, so +Inf is
    byte 255 and -Inf byte 0).  It has no NaN: there qbyte's clamps --
    (255 < v) ? 255 : v, then (0 < v) ? v : 0, the reference's std::min /
    std::max argument order -- are both false, which leaves 0."""
    values = np.asarray(values, np.float32)
    out = np.zeros(len(values), np.uint8)
    fin = ~np.isnan(values)
    out[fin] = quantties.bytes_of(values[fin], s, z, rule=quantties.RULE_FIXED)
    return out


@pytest.mark.parametrize("dim", WIDTHS)
def test_kernel_on_non_finite_rows(torch, G, ctxs, oracle, dim):
    """An all-zero row (Normalize: 0 * sqrt(dim / 0) = NaN everywhere) and a
    row holding +Inf (Normalize: 0 elsewhere, NaN at the Inf) between two
    ordinary rows."""
    ctx = ctxs["plain"]
    x, vec = kernel_rows(dim, 4, 99)
    x[1] = 0.0
    x[2, dim // 2] = np.inf
    for chain in ((), ("normalize",), ("relu", "normalize")):
        f32 = G.rowop_chain(ctx, list(chain), dev(torch, x)).cpu().numpy()
        if chain:
            assert np.all(np.isnan(f32[1])) and np.isnan(f32[2, dim // 2]) and np.all(f32[2, :dim // 2] == 0)
        else:
            assert np.isinf(f32[2, dim // 2])
        for mn, mx in RANGES[:3]:
            s, z = G.quant_params_from_range(mn, mx)
            want = (oracle._quantize_with(f32, s, z).astype(np.int16) - 128).astype(np.int8)
            # the two special rows, exactly emulated: every distinct value among them
            for r in (1, 2):
                vals = np.unique(bits(f32[r]))
                pick = np.union1d(vals[:40], vals[~np.isfinite(vals.view(np.float32))])
                emu = dict(zip(pick.tolist(), emulated_bytes(pick.view(np.float32), s, z).tolist()))
                for c in np.flatnonzero(np.isin(bits(f32[r]), pick)):
                    assert int(want[r, c]) + 128 == emu[int(bits(f32[r])[c])], (dim, chain, r, c)
            got = run_q(torch, G, ctx, list(chain), x, None, s, z, 0)
            check_q(got, want, 4, dim, 0, (dim, chain, (mn, mx)))


# --------------------------------------------------------------------- nets --

PDFS = 52
ROWS = (1, 70, 300)   # 300: past the 256-row GEMM tile and the 280-row latency crossover


@functools.lru_cache(maxsize=None)
def renorm(hidden):
    layers, left, right = rownet.renorm_tdnn(hidden, PDFS)
    assert layers[-1]["kind"] == "log_softmax"
    x = np.random.default_rng(9200 + hidden).normal(0.0, 1.0, size=(ROWS[-1] + left + right, 40)).astype(np.float32)
    x.setflags(write=False)
    return layers, x


_RANGES = {}


def calibrated(torch, G, ctx, hidden):
    """Ranges of the renorm net from Model.calibrate on seeded features the
    tests do not score (computed once)."""
    if hidden not in _RANGES:
        layers, _ = renorm(hidden)
        model = G.Model(ctx, image=netgen.image(layers))
        frames = [150, 90]
        feats = np.random.default_rng(9300 + hidden).normal(0.0, 1.0, size=(sum(frames), 40)).astype(np.float32)
        plan = G.Plan(ctx, [400 + 160 * (n - 1) for n in frames], model)
        r = model.calibrate(ctx, plan, dev(torch, feats))
        assert r.shape == (7, 2) and np.all(r[:, 0] < r[:, 1])
        r.setflags(write=False)
        _RANGES[hidden] = r
    return _RANGES[hidden]


_WANT = {}


def wanted(oracle, hidden, ranges):
    """The rows ahead of the LogSoftmax at ROWS[-1] rows (computed once)."""
    if hidden not in _WANT:
        layers, x = renorm(hidden)
        w = i8rowref.static_rows(oracle, i8rowref.without_final_log_softmax(layers), x, ranges)
        w.setflags(write=False)
        _WANT[hidden] = w
    return _WANT[hidden]


def static_model(G, ctx, layers, ranges, prior=None):
    return G.Model(ctx, image=netgen.image(layers), prior=prior).quantize_static(ctx, ranges)


def run(torch, G, ctx, model, x, **kw):
    return G.nnet_propagate(ctx, model, dev(torch, np.array(x)), **kw).cpu().numpy()


@pytest.mark.parametrize("flavour", ["plain", "latency"])
@pytest.mark.parametrize("hidden", [128, 96])
def test_renorm_nets_bit_for_bit(torch, G, ctxs, oracle, hidden, flavour):
    """128: every boundary takes the storing chain; 96: every boundary the
    chain in place and the quantize pass."""
    ctx = ctxs[flavour]
    layers, x = renorm(hidden)
    ranges = calibrated(torch, G, ctxs["plain"], hidden)
    want = wanted(oracle, hidden, ranges)
    body = static_model(G, ctx, i8rowref.without_final_log_softmax(layers), ranges)
    full = static_model(G, ctx, layers, ranges)
    c = body.left + body.right
    for r in ROWS:
        got = run(torch, G, ctx, body, x[:r + c])
        assert got.shape == (r, PDFS)
        assert first_diff(got, want[:r]) is None, (hidden, flavour, r, first_diff(got, want[:r]))
        ll = run(torch, G, ctx, full, x[:r + c])
        err = float(np.abs(ll - i8rowref.log_softmax_f64(want[:r])).max())
        assert err <= LOGLIK_TOL, (hidden, flavour, r, err)


@pytest.mark.parametrize("flavour", ["plain", "latency"])
def test_second_batchnorm_net_on_the_fallback(torch, G, ctxs, oracle, flavour):
    """Hidden widths 64 / 96: a BatchNorm and a ReLU as row steps, one chain
    launch in place, the quantize pass behind it."""
    ctx = ctxs[flavour]
    layers, x = rownet.exact_cases()["second-bn"]
    ranges = np.array([[-7.0, 7.0], [-300.0, 300.0], [-300.0, 300.0]], np.float32)
    assert i8rowref.launch_counts(layers) == (3, 1, 0)
    want = i8rowref.static_rows(oracle, layers, x[:70 + 4], ranges)
    model = static_model(G, ctx, layers, ranges)
    c = model.left + model.right
    got = run(torch, G, ctx, model, x[:len(want) + c])
    assert first_diff(got, want) is None, first_diff(got, want)


def test_rows_do_not_depend_on_the_batch(torch, G, ctxs, oracle):
    layers, x = renorm(128)
    ranges = calibrated(torch, G, ctxs["plain"], 128)
    want = wanted(oracle, 128, ranges)
    body = i8rowref.without_final_log_softmax(layers)
    models = {f: static_model(G, ctxs[f], body, ranges) for f in ctxs}
    c = models["plain"].left + models["plain"].right
    for f, model in models.items():
        ctx = ctxs[f]
        for r in (0, 37, 69):
            alone = run(torch, G, ctx, model, x[r:r + 1 + c])
            assert first_diff(alone, want[r:r + 1]) is None, (f, r)
        for n in (70, 300):
            assert first_diff(run(torch, G, ctx, model, x[:n + c]), want[:n]) is None, (f, n)
        sizes = [70, 1, 129]
        starts = np.concatenate([[0], np.cumsum(sizes)])
        packed = np.concatenate([x[s:s + n + c] for s, n in zip(starts, sizes)])
        blocks = G.nnet_propagate_blocks(ctx, model, dev(torch, packed), [n + c for n in sizes]).cpu().numpy()
        assert first_diff(blocks, want[:sum(sizes)]) is None, (f, first_diff(blocks, want[:sum(sizes)]))
    # through plans of two segmentations (ce_gpu_am_forward pads every utterance with its edge frames)
    ctx = ctxs["plain"]
    full = static_model(G, ctx, layers, ranges, prior=netgen.prior(PDFS, 91))
    frames = [400, 250]
    feats = np.concatenate([np.array(x[10 * i:10 * i + 50]).repeat(8, 0)[:n] + np.float32(i) for i, n in enumerate(frames)])
    outs = {}
    for max_rows in (4096, 512):
        plan = G.Plan(ctx, [400 + 160 * (n - 1) for n in frames], full, max_rows=max_rows)
        assert plan.total_frames == sum(frames) and (plan.n_chunks > 1) == (max_rows == 512)
        outs[max_rows] = G.am_forward(ctx, full, plan, dev(torch, feats)).cpu().numpy()
    assert np.all(np.isfinite(outs[4096])) and first_diff(outs[512], outs[4096]) is None


@pytest.mark.parametrize("incremental", [False, True])
def test_sessions_match_one_shot(torch, G, ctxs, oracle, global_stats, incremental):
    """Three slots fed pieces of 160, 1600 and 4000 samples up to each
    utterance's EOS: ce_gpu_score's rows bit for bit, and after the first push
    no push allocates or frees."""
    from catears_amd import synth
    ctx = ctxs["plain"]
    layers, _ = renorm(128)
    model = static_model(G, ctx, layers, calibrated(torch, G, ctx, 128), prior=netgen.prior(PDFS, 92))
    gs = dev(torch, global_stats)
    waves = [synth.pcm(9400 + i, n) for i, n in enumerate((4077, 6000, 8000))]
    refs = [G.score(ctx, model, G.Plan(ctx, [len(w)], model), dev(torch, w), gs).cpu().numpy() for w in waves]
    assert all(np.all(np.isfinite(r)) for r in refs)
    for piece in (160, 1600, 4000):
        sess = G.Sessions(ctx, model, 3, piece, gs, incremental=incremental)
        try:
            pos, rows, seen = [0, 0, 0], [[], [], []], []
            while any(p < len(w) for p, w in zip(pos, waves)):
                slots = [k for k in range(3) if pos[k] < len(waves[k])]
                counts = [min(piece, len(waves[k]) - pos[k]) for k in slots]
                eos = [pos[k] + n == len(waves[k]) for k, n in zip(slots, counts)]
                pcm = np.concatenate([waves[k][pos[k]:pos[k] + n] for k, n in zip(slots, counts)])
                out, n_rows = sess.push(slots, dev(torch, pcm), counts, eos=eos)
                out, at = out.cpu().numpy(), 0
                for k, n, r in zip(slots, counts, n_rows):
                    rows[k].append(out[at:at + r])
                    at += r
                    pos[k] += n
                seen.append(G.debug_counters())
        finally:
            sess.close()
        assert len(seen) >= 2 and all(s == seen[0] for s in seen[1:]), (piece, seen[0], seen[-1])
        for k in range(3):
            got = np.concatenate(rows[k])
            assert first_diff(got, refs[k]) is None, (incremental, piece, k, first_diff(got, refs[k]))


def test_the_program_took_the_new_path(torch, G, ctxs):
    ctx = ctxs["plain"]
    for hidden, expect in ((128, (1, 6, 6)), (96, (7, 6, 0))):
        layers, x = renorm(hidden)
        assert i8rowref.launch_counts(layers) == expect
        model = static_model(G, ctx, layers, calibrated(torch, G, ctx, hidden))
        d_x = dev(torch, np.array(x[:70 + model.left + model.right]))
        before = G.debug_i8_static_launches()
        G.nnet_propagate(ctx, model, d_x)
        after = G.debug_i8_static_launches()
        assert tuple(a - b for a, b in zip(after, before)) == expect, (hidden, before, after)


def test_dynamic_int8_rows_through_the_chain(torch, G, ctxs, oracle):
    """ce_gpu_model_quantize on the 128-wide renorm net: the rows of the net
    evaluated layer by layer -- every Linear as the oracle's Quantize of the
    block + MatMat_U8U8F32 + bias (oracle.nnet_propagate_int8's steps), every
    other layer by ce_gpu_rowwise on the device -- bit for bit."""
    ctx = ctxs["plain"]
    layers, x = renorm(128)
    body = i8rowref.without_final_log_softmax(layers)
    model = G.Model(ctx, image=netgen.image(body)).quantize(ctx)
    c = model.left + model.right
    block = np.array(x[:70 + c])
    got = run(torch, G, ctx, model, block)
    v, pre = block, None
    for L in body:
        k = L["kind"]
        if k == "splice":
            pre, v = v, oracle.layer_forward(L, v)
        elif k == "narrow":
            v = oracle.layer_forward(L, v)
        elif k == "linear":
            _, sx, zx = oracle.quantize(pre if pre is not None else v)
            wq, sw, zw = oracle.quantize(L["W"])
            y = oracle.gemm_u8u8f32(oracle._quantize_with(v, sx, zx), sx, zx, wq, sw, zw)
            v, pre = (y + np.asarray(L["b"], np.float32)[None, :]).astype(np.float32), None
        else:
            t = dev(torch, v)
            G.rowwise(ctx, k, t)
            v, pre = t.cpu().numpy(), None
    assert got.shape == v.shape == (70, PDFS)
    assert first_diff(got, v) is None, first_diff(got, v)
