"""ce_gpu_model_admit_row_ops on the GPU: nets with row steps of their own
(tests/rownet.py; tests/test_rownet.py proves the exact cases on the CPU) in
the fp32, bf16x6 (latency mode on and off) and plain bf16 programs.

Exact cases carry zero tolerance against rownet.walk (the bf16 mode against
its restatement, the Normalize output rounded once).  The kernel alone is
compared bit for bit with ce_gpu_rowwise on the same rows.  Real nets meet
the project's 1e-4 bar against fp64 and, in bf16, the spread of the
definition (tests/test_gpu_gemm_bf16.py's method).  Then padding, sessions,
the refusals and the configuration key."""
import functools
import subprocess

import numpy as np
import pytest

import bf16ref
import netgen
import rownet
from test_dropin import DRIVER, _load, _put, _run
from test_gpu_gemm_shapes import first_diff
from test_gpu_pad_widths import load_fails, stream, write_conf
from test_gpu_parity import LOGLIK_TOL, bits, dev

pytestmark = pytest.mark.gpu

MODES = {"fp32": ("plain", "fp32"), "bf16x6": ("plain", "bf16x6"), "latency": ("latency", "bf16x6"),
         "bf16": ("plain", "bf16")}


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


def admitted(G, ctx, layers, gemm=None, prior=None, pad=False):
    """`layers` loaded (fp32: a row step keeps it there), admitted, then
    padded if asked: bf16x6."""
    model = G.Model(ctx, image=netgen.image(layers), prior=prior)
    assert model.gemm == "fp32" and rownet.has_row_steps(layers)
    assert model.admit_row_ops(ctx) is model
    if pad:
        assert model.gemm == "fp32" and model.pad_widths(ctx) is model
    assert model.gemm == "bf16x6"
    return model.set_gemm(gemm) if gemm else model


def run(torch, G, ctx, model, x, **kw):
    return G.nnet_propagate(ctx, model, dev(torch, np.array(x)), **kw).cpu().numpy()


@functools.lru_cache(maxsize=None)
def wanted(name, bf16):
    """The rows a case must give (read-only, computed once)."""
    layers, x = (rownet.big_case() if name == "big" else
                 rownet.pad_cases()[name[4:]] if name.startswith("pad-") else rownet.exact_cases()[name])
    want = rownet.walk(layers, x, rnd=bf16ref.rne_bf16) if bf16 else rownet.check_exact(layers, x)
    want.setflags(write=False)
    return layers, x, want


# -------------------------------------------------------------- exact cases --

@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", sorted(rownet.exact_cases()))
def test_exact_cases(torch, G, ctxs, name, mode):
    """Zero tolerance at 1, 23, 70, 129 and 300 rows, in blocks, and through
    plans of two segmentations: a row's bits do not depend on its block."""
    flavour, gemm = MODES[mode]
    ctx = ctxs[flavour]
    layers, x, want = wanted(name, mode == "bf16")
    model = admitted(G, ctx, layers, gemm)
    c = model.left + model.right
    for r in rownet.ROWS:
        got = run(torch, G, ctx, model, x[:r + c])
        assert first_diff(got, want[:r]) is None, f"{name} {mode} rows={r}: {first_diff(got, want[:r])}"
    sizes = [70, 23, 129]
    starts = np.concatenate([[0], np.cumsum(sizes)])
    packed = np.concatenate([x[s:s + n + c] for s, n in zip(starts, sizes)])
    blocks = G.nnet_propagate_blocks(ctx, model, dev(torch, packed), [n + c for n in sizes]).cpu().numpy()
    assert first_diff(blocks, want[:sum(sizes)]) is None, f"{name} {mode} blocks: {first_diff(blocks, want[:sum(sizes)])}"
    # ce_gpu_am_forward (it needs a prior) pads every utterance with its edge frames
    model = admitted(G, ctx, layers, gemm, prior=netgen.prior(want.shape[1], 87))
    frames = [150, 41]
    feats = [np.array(x[40 * i:40 * i + n]) for i, n in enumerate(frames)]
    ref = np.concatenate([run(torch, G, ctx, model, np.concatenate(
        [np.repeat(f[:1], model.left, 0), f, np.repeat(f[-1:], model.right, 0)]), subtract_prior=True)
        for f in feats])
    for max_rows in (4096, 64):
        plan = G.Plan(ctx, [400 + 160 * (n - 1) for n in frames], model, max_rows=max_rows)
        assert plan.total_frames == sum(frames) and (plan.n_chunks > 1) == (max_rows == 64)
        got = G.am_forward(ctx, model, plan, dev(torch, np.concatenate(feats))).cpu().numpy()
        assert first_diff(got, ref) is None, f"{name} {mode} max_rows={max_rows}: {first_diff(got, ref)}"


@pytest.mark.parametrize("mode", list(MODES))
def test_exact_case_at_1024_by_1024(torch, G, ctxs, mode):
    """A hidden width of 1024 at 1024 rows: the large GEMM tiles write the
    fp32 hidden block ahead of the Normalize."""
    flavour, gemm = MODES[mode]
    layers, x, want = wanted("big", mode == "bf16")
    model = admitted(G, ctxs[flavour], layers, gemm)
    got = run(torch, G, ctxs[flavour], model, x)
    assert first_diff(got, want) is None, f"{mode} {netgen.kernels(layers, 1024, mode if mode != 'bf16' else 'bf16x6')}: " \
                                         f"{first_diff(got, want)}"
    part = run(torch, G, ctxs[flavour], model, x[:70 + model.left + model.right])
    assert first_diff(part, want[:70]) is None


# ---------------------------------------------------------- the kernel alone --

WIDTHS = (32, 96, 1000, 1024, 4096, 4128)   # 4128: the loop path (beyond 64 columns per lane)
CHAINS = [("relu",), ("batchnorm",), ("normalize",), ("softmax",), ("log_softmax",), ("relu", "normalize"),
          ("batchnorm", "relu", "normalize"), ("batchnorm", "relu", "batchnorm", "softmax")]


def real_rows(dim, rows=9, seed=0):
    rng = np.random.default_rng(8500 + dim + seed)
    x = rng.normal(0.0, 2.0, size=(rows, dim)).astype(np.float32)
    vec = [(rng.normal(1.0, 0.2, dim).astype(np.float32), rng.normal(0.0, 0.3, dim).astype(np.float32))
           for _ in range(4)]
    return x, vec


def by_rowwise(torch, G, ctx, chain, x, vec, dim=None):
    """The chain as one ce_gpu_rowwise call per op on a dense copy of the
    true columns."""
    dim = x.shape[1] if dim is None else dim
    t = dev(torch, np.ascontiguousarray(x[:, :dim]))
    for q, op in enumerate(chain):
        sc, of = (dev(torch, vec[q][0][:dim]), dev(torch, vec[q][1][:dim])) if op == "batchnorm" else (None, None)
        G.rowwise(ctx, op, t, sc, of)
    return t.cpu().numpy()


def by_numpy(chain, x, vec):
    for q, op in enumerate(chain):
        x = rownet.row_op(op, x, vec[q][0][:x.shape[1]], vec[q][1][:x.shape[1]])
    return x


def check_against_numpy(chain, got, x, vec):
    """ReLU, BatchNorm and Normalize are bit for bit the numpy restatement.
    Behind an exponential the device's expf and numpy's are two
    implementations, each within 1 ulp of the true value: the same sum order
    then leaves a relative difference of at most 2 ulp per term plus one
    rounding per addition that can fall differently, (dim / 64 + 6) of them;
    the bar is that count of float32 roundings (relative for Softmax, on the
    log-sum for LogSoftmax)."""
    want = by_numpy(chain, x, vec)
    if not any(op in ("softmax", "log_softmax") for op in chain):
        assert first_diff(got, want) is None, (chain, first_diff(got, want))
        return
    eps = (x.shape[1] / 64 + 6 + 4) * 2.0 ** -23
    if chain[-1] == "softmax":
        assert np.all(np.abs(got - want) <= eps * np.abs(want) + 1e-45), chain
    else:
        assert np.all(np.abs(got - want) <= eps * np.maximum(1.0, np.abs(want))), chain


@pytest.mark.parametrize("dim", WIDTHS)
def test_kernel_matches_rowwise_bit_for_bit(torch, G, ctxs, dim):
    """Every op kind and the chains an admitted model launches, on real
    rows: the bits of ce_gpu_rowwise applied op by op, whatever the leading
    dimension and the alignment of the rows; the bf16-store form is
    rne_bf16 of that."""
    ctx = ctxs["plain"]
    x, vec = real_rows(dim)
    dvec = [(dev(torch, s), dev(torch, o)) for s, o in vec]
    for chain in CHAINS:
        want = by_rowwise(torch, G, ctx, chain, x, vec)
        check_against_numpy(chain, want, x, vec)
        for ld, shift in ((dim, 0), (dim + 3, 1)):
            flat = torch.full((x.shape[0] * ld + shift + 4,), 7.0, dtype=torch.float32, device="cuda")
            view = flat[shift:shift + x.shape[0] * ld].view(x.shape[0], ld)[:, :dim]
            view.copy_(dev(torch, x))
            G.rowop_chain(ctx, chain, view, vectors=dvec)
            assert first_diff(view.cpu().numpy(), want) is None, (chain, ld, first_diff(view.cpu().numpy(), want))
            rest = flat.cpu().numpy()
            mask = np.ones(rest.shape, bool)
            mask[shift:shift + x.shape[0] * ld].reshape(x.shape[0], ld)[:, :dim] = False
            assert np.all(rest[mask] == 7.0), (chain, ld, "wrote outside the rows")
        src = dev(torch, x)
        out16 = torch.zeros((x.shape[0], dim), dtype=torch.int16, device="cuda")
        G.rowop_chain(ctx, chain, src, vectors=dvec, out16=out16)
        got16 = (out16.cpu().numpy().view(np.uint16).astype(np.uint32) << 16).view(np.float32)
        assert first_diff(got16, bf16ref.rne_bf16(want)) is None, (chain, "bf16 store")


def test_kernel_on_a_true_width_inside_a_padded_row(torch, G, ctxs):
    """True width 100 at leading dimension 128: the sums and Normalize's D
    cover 100 columns, the 28 pad columns stay +0 (in place nothing is
    written there; the bf16 form converts them as they are)."""
    ctx = ctxs["plain"]
    x, vec = real_rows(100)
    dvec = [(dev(torch, s), dev(torch, o)) for s, o in vec]
    for chain in CHAINS:
        want = by_rowwise(torch, G, ctx, chain, x, vec)
        buf = torch.zeros((x.shape[0], 128), dtype=torch.float32, device="cuda")
        buf[:, :100].copy_(dev(torch, x))
        G.rowop_chain(ctx, chain, buf, dim=100, vectors=dvec)
        got = buf.cpu().numpy()
        assert first_diff(got[:, :100], want) is None, (chain, first_diff(got[:, :100], want))
        assert np.all(bits(got[:, 100:]) == 0), chain
        buf[:, :100].copy_(dev(torch, x))
        out16 = torch.full((x.shape[0], 128), 77, dtype=torch.int16, device="cuda")
        G.rowop_chain(ctx, chain, buf, dim=100, vectors=dvec, out16=out16)
        got16 = (out16.cpu().numpy().view(np.uint16).astype(np.uint32) << 16).view(np.float32)
        assert first_diff(got16[:, :100], bf16ref.rne_bf16(want)) is None and np.all(bits(got16[:, 100:]) == 0), chain


# ---------------------------------------------------------------- real nets --

@functools.lru_cache(maxsize=None)
def renorm_xs():
    from catears_amd import synth
    spec = synth.MODELS["tdnn-xs"]
    layers, left, right = rownet.renorm_tdnn(spec["hidden"], spec["pdfs"])
    x = np.random.default_rng(8600).normal(0.0, 1.0, size=(300 + left + right, 40)).astype(np.float32)
    return layers, x


def test_renorm_tdnn_vs_fp64(torch, G, ctxs):
    """The relu-renorm TDNN-XS shape with real weights: fp32, bf16x6 and
    latency mode within 1e-4 of the fp64 evaluation on the log-likelihoods."""
    layers, x = renorm_xs()
    want = rownet.eval_f64(layers, x)
    errs, outs = {}, {}
    for mode in ("fp32", "bf16x6", "latency"):
        flavour, gemm = MODES[mode]
        model = admitted(G, ctxs[flavour], layers, gemm)
        outs[mode] = run(torch, G, ctxs[flavour], model, x)
        assert outs[mode].shape == want.shape
        errs[mode] = float(np.abs(outs[mode] - want).max())
    print(errs)
    assert max(errs.values()) <= LOGLIK_TOL, errs
    # as loaded (fp32, launch_rowop per step) the model gives the admitted fp32 model's bits
    plain = G.Model(ctxs["plain"], image=netgen.image(layers))
    assert first_diff(run(torch, G, ctxs["plain"], plain, x), outs["fp32"]) is None


def test_renorm_tdnn_bf16_within_the_spread_of_the_definition(torch, G, ctxs):
    """tests/test_gpu_gemm_bf16.py's method on the renorm net: three CPU
    evaluations of the definition (fp64, fp32 on K ascending, fp32 on K
    reversed) set the spread D; p99.9 |GPU - fp64 walk| <= 2 p99.9(D) and
    max <= 4 max(D)."""
    layers, x = renorm_xs()

    def final(v):  # the finalize's LogSoftmax in float64 on the float32 activations, as bf16ref.walk has it
        v = v.astype(np.float64)
        m = v.max(axis=1, keepdims=True)
        return v - (m + np.log(np.exp(v - m).sum(axis=1, keepdims=True)))

    assert layers[-1]["kind"] == "log_softmax"
    body = layers[:-1]
    w64 = final(rownet.walk(body, x, rnd=bf16ref.rne_bf16))
    w32a = final(rownet.walk(body, x, rnd=bf16ref.rne_bf16, acc=np.float32))
    w32d = final(rownet.walk(body, x, rnd=bf16ref.rne_bf16, acc=np.float32, k_reversed=True))
    D = np.concatenate([np.abs(a - b).ravel() for a, b in ((w64, w32a), (w64, w32d), (w32a, w32d))])
    d_max, d_p999 = float(D.max()), float(np.quantile(D, 0.999))
    model = admitted(G, ctxs["plain"], layers, "bf16")
    e = np.abs(run(torch, G, ctxs["plain"], model, x).astype(np.float64) - w64)
    e_max, e_p999 = float(e.max()), float(np.quantile(e, 0.999))
    print(f"|GPU - fp64 walk| max {e_max:.3g} p99.9 {e_p999:.3g}; spread D max {d_max:.3g} p99.9 {d_p999:.3g}")
    assert d_max > 0.0
    assert e_p999 <= 2.0 * d_p999, (e_p999, d_p999)
    assert e_max <= 4.0 * d_max, (e_max, d_max)


# ------------------------------------------------------------------ padding --

@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", sorted(rownet.pad_cases()))
def test_admitted_nets_take_pad_widths(torch, G, ctxs, name, mode):
    """True hidden width 100, 37 pdfs: admitted, the model takes pad_widths
    and gives the unpadded fp32 rows bit for bit (bf16: its restatement's);
    num_pdfs and the output width stay."""
    flavour, gemm = MODES[mode]
    ctx = ctxs[flavour]
    layers, x, want = wanted("pad-" + name, mode == "bf16")
    plain = G.Model(ctx, image=netgen.image(layers))
    with pytest.raises(G.CatearsError, match="ENOTSUP"):
        plain.pad_widths(ctx)
    assert plain.admit_row_ops(ctx).gemm == "fp32"   # the widths still keep it outside
    model = admitted(G, ctx, layers, gemm, pad=True)
    t, p = model.padded_widths()
    assert t.tolist()[-1] == 37 and p.tolist()[-1] == 40 and set(p.tolist()[:-1]) == {128} and model.num_pdfs == 37
    c = model.left + model.right
    for r in (1, 23, 70, 129):
        got = run(torch, G, ctx, model, x[:r + c])
        assert got.shape == (r, 37)
        assert first_diff(got, want[:r]) is None, f"{name} {mode} rows={r}: {first_diff(got, want[:r])}"
    if mode != "bf16":
        unpadded = run(torch, G, ctx, plain, x[:129 + c])
        assert first_diff(unpadded, want[:129]) is None


# ----------------------------------------------------------------- sessions --

@pytest.mark.parametrize("mode", ["fp32", "bf16x6", "latency", "bf16"])
def test_sessions_give_the_one_shot_rows(torch, G, ctxs, global_stats, mode):
    """Plain and incremental sets on an admitted exact case: the rows of
    ce_gpu_score bit for bit, and once warm a push allocates nothing."""
    from catears_amd import synth
    flavour, gemm = MODES[mode]
    ctx = ctxs[flavour]
    layers, _ = rownet.exact_cases()["second-bn"]
    model = admitted(G, ctx, layers, gemm, prior=netgen.prior(rownet.PDFS, 83))
    gs = dev(torch, global_stats)
    wave = synth.pcm(8700, 8000)
    plan = G.Plan(ctx, [len(wave)], model)
    ref = G.score(ctx, model, plan, dev(torch, wave), gs).cpu().numpy()
    assert ref.shape == (48, rownet.PDFS) and np.all(np.isfinite(ref))
    for incremental in (False, True):
        for chunk in (161, 1600, 8000):
            counts = [min(chunk, len(wave) - at) for at in range(0, len(wave), chunk)]
            sess = G.Sessions(ctx, model, 1, chunk, gs, incremental=incremental)
            try:
                got, seen = stream(torch, G, sess, wave, counts)
            finally:
                sess.close()
            assert first_diff(got, ref) is None, (incremental, chunk, first_diff(got, ref))
            assert all(s == seen[min(1, len(seen) - 1)] for s in seen[1:]), (incremental, chunk, seen[1], seen[-1])


def test_sessions_on_a_normalize_net(torch, G, ctxs, global_stats):
    """The same on case 4 (a Normalize between the Linears, real-valued
    fbank input) in bf16x6 with latency mode and in bf16."""
    from catears_amd import synth
    layers, _ = rownet.exact_cases()["normalize-96"]
    gs = dev(torch, global_stats)
    wave = synth.pcm(8701, 8000)
    for mode in ("latency", "bf16"):
        flavour, gemm = MODES[mode]
        ctx = ctxs[flavour]
        model = admitted(G, ctx, layers, gemm, prior=netgen.prior(rownet.PDFS, 84))
        ref = G.score(ctx, model, G.Plan(ctx, [len(wave)], model), dev(torch, wave), gs).cpu().numpy()
        for incremental in (False, True):
            counts = [400] * 20
            sess = G.Sessions(ctx, model, 1, 400, gs, incremental=incremental)
            try:
                got, seen = stream(torch, G, sess, wave, counts)
            finally:
                sess.close()
            assert first_diff(got, ref) is None, (mode, incremental, first_diff(got, ref))
            assert all(s == seen[1] for s in seen[1:]), (mode, incremental)


def test_reserve_covers_every_mode_of_an_admitted_model(torch, G, global_stats):
    """tests/test_gpu_sessions.py's reserve test on an admitted model: one
    set, the model switched through its three modes with latency off and on;
    the workspaces grown at create (the bf16 program's fp32 block ahead of
    the row steps among them) cover them all."""
    from catears_amd import synth
    c = G.Context(0)
    layers, _ = rownet.exact_cases()["normalize-96"]
    m = admitted(G, c, layers, "fp32", prior=netgen.prior(rownet.PDFS, 88))
    gs = dev(torch, global_stats)
    pcm = dev(torch, synth.pcm(8702, 4 * 1600))
    seen = []
    sess = G.Sessions(c, m, 1, 1600, gs)
    try:
        for lat in (False, True):
            for mode in ("fp32", "bf16x6", "bf16"):
                c.set_latency(lat)
                m.set_gemm(mode)
                for t in range(4):
                    sess.push([0], pcm[1600 * t:1600 * (t + 1)], [1600], eos=[t == 3])
                    seen.append(G.debug_counters())
                sess.reset(0)
    finally:
        sess.close()
    assert len(seen) == 24 and seen[1] == seen[-1] and seen[1][0] > 0, (seen[1], seen[-1])


# --------------------------------------------------------- refusals and keys --

def test_gate(torch, G, ctxs):
    ctx = ctxs["plain"]
    layers, x = rownet.exact_cases()["second-bn"]
    model = G.Model(ctx, image=netgen.image(layers))
    assert model.gemm == "fp32"
    with pytest.raises(G.CatearsError, match="ENOTSUP"):
        model.set_gemm("bf16x6")
    before = run(torch, G, ctx, model, x[:27])
    assert model.admit_row_ops(ctx).gemm == "bf16x6"
    for name in ("bf16x6p", "f16x3"):
        with pytest.raises(G.CatearsError, match="ENOTSUP"):
            model.set_gemm(name)
    for name in ("fp32", "bf16", "bf16x6"):
        assert model.set_gemm(name).gemm == name
    # idempotent: the mode the caller chose stays
    assert model.set_gemm("bf16").admit_row_ops(ctx).gemm == "bf16"
    assert first_diff(run(torch, G, ctx, model.set_gemm("fp32"), x[:27]), before) is None
    # a model without a row step: OK, nothing changes -- it still takes the plane modes
    _, a_layers, _ = netgen.exact_cases("B")[0]
    a = G.Model(ctx, image=netgen.image(a_layers)).set_gemm("bf16x6p")
    assert a.admit_row_ops(ctx).gemm == "bf16x6p" and a.set_gemm("f16x3").gemm == "f16x3"
    # int8 of either form: EINVAL; quantize on an admitted model works as ever
    ranges = np.array([[-7.0, 7.0], [-300.0, 300.0], [-300.0, 300.0]], np.float32)
    for quantize in (lambda m: m.quantize(ctx), lambda m: m.quantize_static(ctx, ranges)):
        m8 = quantize(G.Model(ctx, image=netgen.image(layers)))
        want8 = run(torch, G, ctx, m8, x[:27])
        with pytest.raises(G.CatearsError, match="EINVAL"):
            m8.admit_row_ops(ctx)
        got8 = run(torch, G, ctx, quantize(G.Model(ctx, image=netgen.image(layers)).admit_row_ops(ctx)), x[:27])
        assert first_diff(got8, want8) is None


def test_calibrate_gives_the_same_ranges_in_fp32_and_bf16x6(torch, G, ctxs):
    """The tap sees each Linear's input after the row steps: on an exact case
    both programs fold the same values."""
    ctx = ctxs["plain"]
    layers, _ = rownet.exact_cases()["second-bn"]
    frames = [30, 7]
    feats = [netgen._ints(np.random.default_rng(8800 + i), -7, 7, (n, 40)) for i, n in enumerate(frames)]
    model = admitted(G, ctx, layers)
    plan = G.Plan(ctx, [400 + 160 * (n - 1) for n in frames], model)
    d_feats = dev(torch, np.concatenate(feats))
    got = model.calibrate(ctx, plan, d_feats)
    want = model.set_gemm("fp32").calibrate(ctx, plan, d_feats)
    assert want.shape == (3, 2) and np.array_equal(bits(got), bits(want)), (got, want)
    as_loaded = G.Model(ctx, image=netgen.image(layers)).calibrate(ctx, plan, d_feats)
    assert np.array_equal(bits(as_loaded), bits(want))
    # Linear 1's input is the row steps' output: BatchNorm then ReLU, so its minimum is 0
    assert want[1, 0] == 0.0 and want[1, 1] > 0.0


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from catears_amd import formats
    d = tmp_path_factory.mktemp("rowops")
    layers, left, right = rownet.renorm_tdnn(64, rownet.PDFS)
    prior = netgen.prior(rownet.PDFS, 85)
    (d / "r.nnet").write_bytes(netgen.image(layers))
    (d / "r.prior").write_bytes(formats.vec_bytes(prior))
    (d / "r.tid2pdf").write_bytes(formats.vec_bytes(np.arange(5, dtype=np.int32), np.int32))
    n_lin = sum(L["kind"] == "linear" for L in layers)
    (d / "r.ranges").write_bytes(formats.vec_bytes(np.array([-9, 9] * n_lin, np.float32)))
    base = (f"nnet = {d / 'r.nnet'}\nprior = {d / 'r.prior'}\ntid2pdf = {d / 'r.tid2pdf'}\nleft_context = {left}\n"
            f"right_context = {right}\nnum_pdfs = {rownet.PDFS}\n")
    return d, layers, prior, base


def test_load_config_key(torch, G, ctxs, files):
    d, layers, prior, base = files
    ctx = ctxs["plain"]
    x = netgen.real_input(layers, 70, 8900)
    m = G.Model(ctx, str(write_conf(d, "ok.conf", base, 50, "gpu_row_ops = 1\ngpu_gemm = bf16\n")))
    assert m.gemm == "bf16"
    want = run(torch, G, ctx, admitted(G, ctx, layers, "bf16", prior=prior), x, subtract_prior=True)
    assert first_diff(run(torch, G, ctx, m, x, subtract_prior=True), want) is None
    assert G.Model(ctx, str(write_conf(d, "one.conf", base, 50, "gpu_row_ops = 1\n"))).gemm == "bf16x6"
    assert G.Model(ctx, str(write_conf(d, "zero.conf", base, 50, "gpu_row_ops = 0\n"))).gemm == "fp32"
    rc, msg = load_fails(G, ctx, write_conf(d, "zero16.conf", base, 50, "gpu_row_ops = 0\ngpu_gemm = bf16\n"))
    assert rc == -6 and "gpu_gemm" in msg, (rc, msg)
    rc, msg = load_fails(G, ctx, write_conf(d, "two.conf", base, 50, "gpu_row_ops = 2\n"))
    assert rc == -2 and "gpu_row_ops = 2" in msg, (rc, msg)
    # beside gpu_int8_ranges: accepted, no effect
    outs = []
    for i, extra in enumerate(("", "gpu_row_ops = 1\n")):
        m8 = G.Model(ctx, str(write_conf(d, f"i8_{i}.conf", base, 50, f"gpu_int8_ranges = {d / 'r.ranges'}\n" + extra)))
        assert m8.quant_params()[0].size == m8.num_linear
        outs.append(run(torch, G, ctx, m8, x, subtract_prior=True))
    assert first_diff(outs[1], outs[0]) is None


def test_load_config_key_before_pad_widths(torch, G, ctxs, tmp_path):
    """gpu_row_ops is applied before gpu_pad_widths, which is applied before
    gpu_gemm: a net outside the envelope by a row step and by its widths."""
    from catears_amd import formats
    ctx = ctxs["plain"]
    layers, x = rownet.pad_cases()["normalize"]
    (tmp_path / "p.nnet").write_bytes(netgen.image(layers))
    (tmp_path / "p.prior").write_bytes(formats.vec_bytes(netgen.prior(37, 86)))
    (tmp_path / "p.tid2pdf").write_bytes(formats.vec_bytes(np.arange(5, dtype=np.int32), np.int32))
    left, right = netgen.context(layers)
    base = (f"nnet = p.nnet\nprior = p.prior\ntid2pdf = p.tid2pdf\nleft_context = {left}\nright_context = {right}\n"
            "num_pdfs = 37\n")
    m = G.Model(ctx, str(write_conf(tmp_path, "ok.conf", base, 50, "gpu_gemm = bf16x6\ngpu_pad_widths = 1\ngpu_row_ops = 1\n")))
    assert m.gemm == "bf16x6" and m.padded_widths()[1].tolist() == [128, 40]
    assert first_diff(run(torch, G, ctx, m, x[:70 + left + right]), wanted("pad-normalize", False)[2][:70]) is None
    rc, msg = load_fails(G, ctx, write_conf(tmp_path, "no.conf", base, 50, "gpu_pad_widths = 1\n"))
    assert rc == -6 and "gpu_pad_widths" in msg, (rc, msg)


@pytest.mark.parametrize("chunk", [7, 50])
def test_am_read_key_gives_the_c_abi_rows(torch, G, ctxs, tmp_path, files, chunk):
    """The drop-in AcousticModel::Read applies gpu_row_ops before gpu_gemm:
    its streamed chunks are the admitted C-ABI model's rows of the whole
    utterance -- with latency mode on (the drop-in's default; bf16x6's
    split-K order, so the reference is a latency-mode context) and off with
    two batched streams."""
    d, layers, prior, base = files
    left, right = netgen.context(layers)
    feats = netgen.real_input(layers, 200, 8910)[left:-right]
    block = np.concatenate([np.repeat(feats[:1], left, 0), feats, np.repeat(feats[-1:], right, 0)])
    x = _put(tmp_path, "x.f32", feats)
    for i, (flavour, extra) in enumerate((("latency", ""), ("plain", "gpu_latency_mode = 0\ngpu_batch_streams = 2\n"))):
        ctx = ctxs[flavour]
        want = run(torch, G, ctx, admitted(G, ctx, layers, "bf16x6", prior=prior), block, subtract_prior=True)
        conf = write_conf(tmp_path, f"am{i}.conf", base, chunk, "gpu_row_ops = 1\ngpu_gemm = bf16x6\n" + extra)
        out = tmp_path / f"am{i}.bin"
        _run("am", conf, x, len(feats), out)
        got = _load(out)
        assert got.shape == want.shape == (200, rownet.PDFS)
        assert first_diff(got, want) is None, first_diff(got, want)


def test_am_read_refuses_a_bad_value(tmp_path, files):
    d, layers, prior, base = files
    x = _put(tmp_path, "x.f32", np.zeros((10, 40), np.float32))
    conf = write_conf(tmp_path, "two.conf", base, 50, "gpu_row_ops = 2\n")
    r = subprocess.run([DRIVER, "am", str(conf), str(x), "10", str(tmp_path / "o.bin")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0
    assert "gpu_row_ops = 2" in r.stdout + r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "o.bin").exists()
