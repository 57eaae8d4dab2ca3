"""Latency mode of the plain bf16 GEMM on the GPU (kernels/gemm_bf16_lat.hip):
on a context with ce_gpu_ctx_set_latency a bf16 model's Linears run on
gemm_bf16_lat_kernel up to ce_gpu_bf16_latency_max_rows rows -- and give the
bits of the mode off, since the kernel keeps the MFMA, the K order, the single
accumulator and the epilogue.

tests/bf16lat.py restates the dispatch rule; tests/test_bf16_latency.py shows
on the CPU that the real-valued cases here would tell a split or reordered K
sum (at least one output in four differs), and that the exact inputs here
keep the fp64 walk a zero-tolerance oracle.  ce_gpu_debug_bf16_latency_launches
shows which kernel a call took; no test reads kernel code."""
import ctypes
import functools
import subprocess

import numpy as np
import pytest

import bf16lat
import bf16ref
import netgen
import rownet
from test_dropin import _am_config, _load, _put
from test_gpu_gemm_bf16 import EXACT_GEOMS, ONE_LINEAR
from test_gpu_gemm_shapes import first_diff
from test_gpu_parity import bits, dev

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
    """One throughput context and one latency context for the module."""
    c = {"thr": G.Context(0), "lat": G.Context(0)}
    c["lat"].set_latency(True)
    return c


@pytest.fixture(scope="module")
def R(G):
    r = G.bf16_latency_max_rows()
    assert r == bf16lat.MAX_ROWS >= 70
    return r


def bf16_model(G, ctx, layers=None, conf=None, prior=None):
    model = G.Model(ctx, conf) if conf else G.Model(ctx, image=netgen.image(layers), prior=prior)
    return model.set_gemm("bf16")


def run(torch, G, ctx, model, x, **kw):
    return G.nnet_propagate(ctx, model, dev(torch, np.array(x)), **kw).cpu().numpy()


class Counter:
    """The latency kernel's launches since construction / the last take()."""

    def __init__(self, G):
        self.G, self.at = G, G.debug_bf16_latency_launches()

    def take(self):
        now = self.G.debug_bf16_latency_launches()
        d, self.at = now - self.at, now
        return d


# ----------------------------------------------------- 1. exact-integer nets --

@functools.lru_cache(maxsize=None)
def exact_cases(geom):
    """[(name, layers, x, want)]: netgen's one-plane cases on an input of
    kB16LatMaxRows + 1 rows, with the fp64 walk's rows (read-only)."""
    out = []
    for name, layers, _ in netgen.one_plane_mode_cases(geom):
        c = sum(netgen.context(layers))
        x = bf16lat.exact_input(layers, name, bf16lat.MAX_ROWS + 1 - c, 9100)
        want = bf16ref.walk(layers, x, np.float64)
        want.setflags(write=False)
        out.append((name, layers, x, want))
    return out


@pytest.mark.parametrize("geom", EXACT_GEOMS)
def test_exact_integer_nets_on_the_latency_context(torch, G, ctxs, R, geom):
    """Zero tolerance at 1, 17, 70, R - c and R - c + 1 output rows; the
    launch counter advances by the number of Linears while the block has at
    most R rows and by nothing at R + 1 (the throughput kernel, same bits)."""
    failures = []
    for name, layers, x, want in exact_cases(geom):
        model = bf16_model(G, ctxs["lat"], layers)
        c = model.left + model.right
        nlin = len(netgen.linears(layers))
        for r in (1, 17, 70, R - c, R - c + 1):
            count = Counter(G)
            got = run(torch, G, ctxs["lat"], model, x[:r + c])
            launched = count.take()
            assert launched == bf16lat.latency_launches(layers, r) == (nlin if r + c <= R else 0), (geom, name, r, launched)
            d = first_diff(got, want[:r])
            if d:
                failures.append(f"{geom} {name} rows={r}: {d}")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------ 2. real-valued nets --

def real_case(which, s_config=None, xs_config=None):
    """(layers or None, conf or None, x of R rows, kwargs)."""
    if which == "A":
        in_d, widths, splices, post = netgen.GEOMETRIES["A"]
        layers = netgen.real_net(in_d, widths, splices, post, 2100)
        return layers, None, netgen.real_input(layers, bf16lat.MAX_ROWS, 2600), {}
    if which == "one-linear-3072":
        in_dim, splice = ONE_LINEAR[3072]
        layers = netgen.real_net(in_dim, [96], [splice], [()], seed=3072 + 96, log_softmax=False)
        assert netgen.linears(layers)[0]["k"] == 3072
        return layers, None, netgen.real_input(layers, bf16lat.MAX_ROWS, 3600), {}
    conf = xs_config if which == "tdnn-xs" else s_config
    x = np.random.default_rng(4100).normal(0.0, 1.0, size=(bf16lat.MAX_ROWS, 40)).astype(np.float32)
    return None, conf, x, {"subtract_prior": True}


@pytest.mark.parametrize("which", ["A", "one-linear-3072", "tdnn-xs", "tdnn-s"])
def test_real_valued_nets_give_the_throughput_bits(torch, G, ctxs, R, xs_config, s_config, which):
    """The latency context's rows equal the throughput context's, bit for bit,
    at 1, 2, 15, 16, 17, 70 and R - c output rows (TDNN-S: 70), and the new
    kernel computed them.  tests/test_bf16_latency.py: a K sum in another
    order would differ in at least one output in four of these Linears."""
    layers, conf, x, kw = real_case(which, s_config, xs_config)
    thr, lat = bf16_model(G, ctxs["thr"], layers, conf), bf16_model(G, ctxs["lat"], layers, conf)
    c = lat.left + lat.right
    for r in (70,) if which == "tdnn-s" else (1, 2, 15, 16, 17, 70, R - c):
        count = Counter(G)
        want = run(torch, G, ctxs["thr"], thr, x[:r + c], **kw)
        assert count.take() == 0
        got = run(torch, G, ctxs["lat"], lat, x[:r + c], **kw)
        assert count.take() == lat.num_linear > 0
        assert got.shape == (r, lat.num_pdfs) and np.all(np.isfinite(got))
        assert first_diff(got, want) is None, (which, r, first_diff(got, want))


# ------------------------------------- 3. block and window independence --

def test_blocks_and_windows(torch, G, ctxs, R):
    """propagate_blocks over 33 / 70 / 40 rows (packed below R: one latency
    launch per Linear for all of them): every block's rows are its rows
    alone.  And rows scored at m <= R equal the same rows inside a block of
    m > R, which the same context runs on the throughput kernel."""
    layers, _, _, _ = real_case("A")
    x = netgen.real_input(layers, R + 40, 2601)
    model = bf16_model(G, ctxs["lat"], layers)
    c = model.left + model.right
    sizes = [33 - c, 70 - c, 40 - c]
    assert sum(sizes) + 3 * c < R and min(sizes) > 0
    starts = np.concatenate([[0], np.cumsum(sizes)])
    packed = np.concatenate([x[s:s + n + c] for s, n in zip(starts, sizes)])
    count = Counter(G)
    blocks = G.nnet_propagate_blocks(ctxs["lat"], model, dev(torch, packed), [n + c for n in sizes]).cpu().numpy()
    assert count.take() == model.num_linear
    for s, n in zip(starts, sizes):
        alone = run(torch, G, ctxs["lat"], model, x[s:s + n + c])
        assert first_diff(blocks[s:s + n], alone) is None, (s, n)
    assert count.take() == 3 * model.num_linear
    big = run(torch, G, ctxs["lat"], model, x)      # R + 40 + c rows: beyond the crossover
    assert count.take() == 0 and big.shape[0] == R + 40
    small = run(torch, G, ctxs["lat"], model, x[:70 + c])
    assert count.take() == model.num_linear
    assert first_diff(small, big[:70]) is None
    assert first_diff(blocks, big[:sum(sizes)]) is None


# ------------------------------------------------------------ 4. output forms --

def test_row_steps_behind_a_hidden_linear(torch, G, ctxs):
    """An admitted model with Normalize behind a hidden Linear: that Linear
    writes fp32, the row steps hand the next one bf16."""
    layers, x = rownet.exact_cases()["normalize-96"]
    models = {}
    for k in ("thr", "lat"):
        m = G.Model(ctxs[k], image=netgen.image(layers))
        models[k] = m.admit_row_ops(ctxs[k]).set_gemm("bf16")
    c = models["lat"].left + models["lat"].right
    for r in (1, 70, 129):
        count = Counter(G)
        want = run(torch, G, ctxs["thr"], models["thr"], x[:r + c])
        got = run(torch, G, ctxs["lat"], models["lat"], x[:r + c])
        assert count.take() == models["lat"].num_linear == 2
        assert first_diff(got, want) is None, (r, first_diff(got, want))
    assert first_diff(got, rownet.walk(layers, x, rnd=bf16ref.rne_bf16)[:129]) is None


def test_padded_widths(torch, G, ctxs):
    """A net of hidden width 330 and 101 outputs (the 650-wide TDNN's shape,
    smaller), moved onto padded widths by pad_widths."""
    layers = netgen.real_net(40, [330, 330, 101], [netgen.S5, [-1, 0, 2], [0]], [netgen.RB, netgen.BR, ()], 5100)
    x = netgen.real_input(layers, 129, 5101)
    models = {k: G.Model(ctxs[k], image=netgen.image(layers)).pad_widths(ctxs[k]).set_gemm("bf16") for k in ctxs}
    c = models["lat"].left + models["lat"].right
    for r in (1, 70, 129):
        count = Counter(G)
        want = run(torch, G, ctxs["thr"], models["thr"], x[:r + c])
        got = run(torch, G, ctxs["lat"], models["lat"], x[:r + c])
        assert count.take() == 3 and got.shape == (r, 101)
        assert first_diff(got, want) is None, (r, first_diff(got, want))


def test_caller_buffers(torch, G, ctxs):
    """Input rows 47 floats apart (ld_in > width) and an output that starts
    one row into its allocation."""
    layers, _, x, _ = real_case("A")
    models = {k: bf16_model(G, ctxs[k], layers) for k in ctxs}
    c = models["lat"].left + models["lat"].right
    r = 70
    want = run(torch, G, ctxs["thr"], models["thr"], x[:r + c])
    wide = torch.full((r + c, 47), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :40] = dev(torch, np.ascontiguousarray(x[:r + c]))
    store = torch.full((r + 2, models["lat"].num_pdfs), 7.0, dtype=torch.float32, device="cuda")
    count = Counter(G)
    G.nnet_propagate(ctxs["lat"], models["lat"], wide[:, :40], out=store[1:r + 1])
    assert count.take() == 3
    got = store.cpu().numpy()
    assert first_diff(got[1:r + 1], want) is None
    assert np.all(got[0] == 7.0) and np.all(got[r + 1] == 7.0)


# ---------------------------------------------------------------- 5. sessions --

@pytest.mark.parametrize("incremental", [False, True])
def test_sessions_on_the_latency_context(torch, G, ctxs, xs_config, global_stats, incremental):
    """TDNN-XS, three slots, chunks of 777 and 1600 samples with CMVN: the
    streamed rows are the throughput context's one-shot score; warm pushes
    allocate nothing; the pushes ran on the latency kernel."""
    from catears_amd import synth
    from test_gpu_sessions import check_jobs, run_jobs
    gs = dev(torch, global_stats)
    jobs = {0: [(synth.pcm(710, 24000), 777)], 1: [(synth.pcm(711, 32000), 1600)],
            2: [(synth.pcm(712, 16000), 777), (synth.pcm(713, 12000), 1600)]}
    c = G.Context(0)  # a session set is one per context
    c.set_latency(True)
    sess = G.Sessions(c, bf16_model(G, c, conf=xs_config), 3, 1600, gs, incremental=incremental)
    seen = {}
    count = Counter(G)
    try:
        got = run_jobs(torch, G, sess, jobs, on_tick=lambda t: seen.__setitem__(t, G.debug_counters()))
    finally:
        sess.close()
    assert count.take() > 0
    ticks = sorted(seen)
    assert len(ticks) >= 20 and all(seen[t] == seen[2] for t in ticks[1:]), seen
    check_jobs(torch, G, ctxs["thr"], bf16_model(G, ctxs["thr"], conf=xs_config), gs, jobs, got)
    assert count.take() == 0   # the reference ran on the throughput context


# ----------------------------------------------------------------- 6. drop-in --

@pytest.mark.parametrize("chunk", [7, 50])
def test_dropin_latency_key_reaches_the_bf16_gemms(torch, G, ctxs, oracle, tmp_path, xs_config, chunk):
    """AcousticModel with gpu_gemm = bf16: the streamed chunks run on the
    latency kernel with gpu_latency_mode = 1 (the default) and never with 0 --
    the driver reports the library's counter -- and both give the rows of the
    whole padded utterance on the throughput context."""
    import os
    from catears_amd import formats, synth
    from conftest import ROOT
    driver = os.path.join(ROOT, "catears_amd", "lib", "pk_am_launches")
    assert os.path.exists(driver), "pk_am_launches not built"
    feats = oracle.Fbank().compute(synth.pcm(5, 16000 + 123))
    am = formats.read_am(xs_config)
    block = np.concatenate([np.repeat(feats[:1], am["left"], 0), feats, np.repeat(feats[-1:], am["right"], 0)], 0)
    want = run(torch, G, ctxs["thr"], bf16_model(G, ctxs["thr"], conf=xs_config), block, subtract_prior=True)
    x = _put(tmp_path, "x.f32", feats)
    launches = {}
    for mode in (1, 0):
        d = tmp_path / f"mode{mode}"
        d.mkdir()
        conf = _am_config(d, xs_config, chunk, extra=f"gpu_gemm = bf16\ngpu_latency_mode = {mode}\n")
        out = tmp_path / f"am{mode}.bin"
        r = subprocess.run([driver, str(conf), str(x), str(len(feats)), str(out)], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        words = r.stdout.split()
        launches[mode] = int(words[words.index("bf16_latency_launches") + 1])
        got = _load(out)
        assert got.shape == want.shape
        diff = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
        assert diff.size == 0, f"mode {mode}: {diff.size} frames differ, first {diff[0]}"
    # at least one launch per streamed chunk with the mode on, none with it off
    assert launches[0] == 0 and launches[1] >= -(-len(feats) // chunk), launches


# --------------------------------------------------- 7. refusals and no-ops --

def test_other_modes_never_take_the_kernel(torch, G, ctxs, xs_config):
    """fp32, bf16x6 and static int8 models on the latency context leave the
    counter alone; NULL is CE_GPU_EINVAL."""
    from catears_amd import synth
    lat = ctxs["lat"]
    x = np.random.default_rng(4200).normal(0.0, 1.0, size=(70, 40)).astype(np.float32)
    count = Counter(G)
    m = G.Model(lat, xs_config)
    for mode in ("fp32", "bf16x6"):
        run(torch, G, lat, m.set_gemm(mode), x)
    assert count.take() == 0
    waves = [synth.pcm(60 + i, 16000 * 2) for i in range(2)]
    plan = G.Plan(lat, [len(w) for w in waves], m)
    ranges = m.calibrate(lat, plan, G.fbank(lat, plan, dev(torch, np.concatenate(waves))))
    i8 = G.debug_i8_latency_launches()
    run(torch, G, lat, m.quantize_static(lat, ranges), x)
    assert count.take() == 0 and G.debug_i8_latency_launches() > i8
    run(torch, G, lat, bf16_model(G, lat, conf=xs_config), x)
    assert count.take() > 0
    # the mode off: the same model form never takes it
    run(torch, G, ctxs["thr"], bf16_model(G, ctxs["thr"], conf=xs_config), x)
    assert count.take() == 0
    assert G.lib().ce_gpu_bf16_latency_max_rows(None) == -2
    n = ctypes.c_int(-1)
    assert G.lib().ce_gpu_bf16_latency_max_rows(ctypes.byref(n)) == 0 and n.value == bf16lat.MAX_ROWS
