"""Values the other tests never feed: full-scale integer signals through the
three fbank entries, and a NaN or an Inf that must stay inside the rows that
read it -- in fbank (eight frames share a wave and an LDS region), in CMVN
and in every nnet GEMM mode.

Full scale.  The frame's DC sum is combined across lanes in no fixed order
(csrc/fbank8_ops.h lane_sum); that is exact only while every partial sum of a
frame's samples is an integer below 2^24, which 400 int16 samples guarantee
(400 * 32768 < 2^24; asserted on the signals below).  So the exact mode's
pre-log mel energies are the oracle's bit for bit at full scale too, the
int16 entry gives the float entry's bits, and the fast mode stays at the bar
of tests/test_gpu_fbank_fast.py.

Isolation.  One NaN (or +Inf) sample makes NaN of every frame whose 400
samples cover it, in all 40 bands, as the oracle's; every other row of the
batch carries the bits of the same batch without it.  The same for one NaN
feature row under CMVN (its utterance's later rows follow the oracle's mask)
and for one NaN input row of an nnet block.
"""
import functools

import numpy as np
import pytest

import netgen
from test_gpu_fbank_fast import SYNTH_TOL
from test_gpu_parity import FEAT_TOL, bits, dev

pytestmark = pytest.mark.gpu

HI, LO = 32767, -32768


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
def fctx(torch, G):
    c = G.Context(0)
    c.set_fbank("fast")
    return c


def fbank(torch, G, ctx, waves, dtype=np.float32):
    """(plan, feats, mel) of a batch through the float or the int16 entry."""
    plan = G.Plan(ctx, [len(w) for w in waves])
    feats = torch.empty((plan.total_frames, 40), dtype=torch.float32, device="cuda")
    mel = torch.empty_like(feats)
    G.fbank(ctx, plan, dev(torch, np.concatenate(waves).astype(dtype)), feats, mel)
    return plan, feats.cpu().numpy(), mel.cpu().numpy()


# -------------------------------------------------------------- full scale --

def square(n, period):
    """Full-scale square wave: high for the first half of each period (the
    longer half of an odd period)."""
    i = np.arange(n)
    return np.where((i % period) * 2 < period, HI, LO).astype(np.int16)


def impulse(n, *at):
    w = np.zeros(n, np.int16)
    w[list(at)] = HI
    return w


@functools.lru_cache(maxsize=None)
def full_scale_batches():
    """Two batches of six int16 utterances of 1 to 2 s."""
    alt = np.where(np.arange(17777) % 2 == 0, LO, HI).astype(np.int16)
    step = np.concatenate([np.zeros(8123, np.int16), np.full(16000, HI, np.int16)])   # silence, then full scale
    a = [np.full(16000, LO, np.int16), alt, square(16000, 2), square(20001, 3), square(24000, 160), square(32000, 400)]
    # impulses: the first sample, frame 0's last, the last sample of the last frame, a pair across frame 0's end
    b = [impulse(16000, 0), impulse(16400, 399), impulse(16400, 16399), impulse(16000, 399, 400),
         step, square(16161, 400)[::-1].copy()]
    for w in a + b:
        assert 16000 <= len(w) <= 32000 and w.dtype == np.int16
        # lane_sum's premise: every partial sum of a frame's samples is an integer below 2^24
        c = np.concatenate([[0], np.cumsum(np.abs(w.astype(np.int64)))])
        assert (c[400:] - c[:-400]).max() < 2 ** 24
    assert any((w == LO).any() for w in a) and any((w == HI).any() for w in a)
    return a, b


@functools.lru_cache(maxsize=None)
def full_scale_oracle(which):
    from oracle import pyoracle
    fb = pyoracle.Fbank()
    out = [fb.compute(w.astype(np.float32), with_mel=True) for w in full_scale_batches()[which]]
    for f, m in out:
        f.setflags(write=False), m.setflags(write=False)
    return out


@pytest.mark.parametrize("which", [0, 1])
def test_full_scale_signals(torch, G, ctx, fctx, oracle, which):
    waves = full_scale_batches()[which]
    want = full_scale_oracle(which)
    plan, f, m = fbank(torch, G, ctx, waves)
    off = plan.frame_offsets
    for u, (of, om) in enumerate(want):
        assert off[u + 1] - off[u] == len(of) > 0
        assert np.array_equal(bits(m[off[u]:off[u + 1]]), bits(om)), f"utt {u}: pre-log mel not bit-exact"
        assert np.abs(f[off[u]:off[u + 1]] - of).max() <= FEAT_TOL, f"utt {u}"
    _, f16, m16 = fbank(torch, G, ctx, waves, np.int16)
    assert np.array_equal(bits(f16), bits(f)) and np.array_equal(bits(m16), bits(m))
    _, ff, _ = fbank(torch, G, fctx, waves)
    _, ff16, _ = fbank(torch, G, fctx, waves, np.int16)
    assert np.array_equal(bits(ff16), bits(ff))
    errs = [float(np.abs(ff[off[u]:off[u + 1]] - of).max()) for u, (of, _) in enumerate(want)]
    print("fast mode vs oracle, per utterance:", " ".join(f"{e:.3g}" for e in errs))
    assert max(errs) <= SYNTH_TOL, errs


# ------------------------------------------------------- isolation: fbank --

def frames_covering(sample, n_frames):
    return [i for i in range(n_frames) if 160 * i <= sample < 160 * i + 400]


@functools.lru_cache(maxsize=None)
def clean_waves():
    from catears_amd import synth
    return tuple(synth.pcm(8800 + i, n) for i, n in enumerate([16000, 24000, 17777, 32000, 20001]))


# mid-frame; the first sample of frame 37 (and the last but 239 of 36, ...);
# the last sample of frame 50
BAD_SAMPLES = (160 * 41 + 77, 160 * 37, 160 * 50 + 399)


@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_fbank_keeps_a_bad_sample_in_its_frames(torch, G, ctx, fctx, oracle, bad, mode):
    c = ctx if mode == "exact" else fctx
    waves = list(clean_waves())
    plan, f0, m0 = fbank(torch, G, c, waves)
    assert np.isfinite(f0).all() and np.isfinite(m0).all()
    off = plan.frame_offsets
    fb = oracle.Fbank()
    for u, s in zip((2, 0, 4), BAD_SAMPLES):
        dirty = [w.copy() for w in waves]
        dirty[u][s] = bad
        _, f, m = fbank(torch, G, c, dirty)
        n = off[u + 1] - off[u]
        hit = off[u] + np.array(frames_covering(s, n))
        assert 1 <= len(hit) <= 3
        of, om = fb.compute(dirty[u], with_mel=True)
        # the oracle's mask: every band of the covering frames, nothing else
        want_nan = np.zeros(f.shape, bool)
        want_nan[hit] = True
        assert np.array_equal(np.isnan(of), want_nan[off[u]:off[u + 1]]) and np.array_equal(np.isnan(om), np.isnan(of))
        assert np.array_equal(np.isnan(f), want_nan) and np.array_equal(np.isnan(m), want_nan), (u, s)
        keep = ~want_nan
        assert np.array_equal(bits(f)[keep], bits(f0)[keep]) and np.array_equal(bits(m)[keep], bits(m0)[keep]), (u, s)


# -------------------------------------------------------- isolation: CMVN --

def test_cmvn_keeps_a_nan_row_in_its_utterance(torch, G, ctx, oracle, global_stats):
    waves = list(clean_waves())
    plan, f0, _ = fbank(torch, G, ctx, waves)
    off = plan.frame_offsets
    gs = dev(torch, global_stats)
    clean = G.cmvn(ctx, plan, gs, dev(torch, f0)).cpu().numpy()
    assert np.isfinite(clean).all()
    for u, t in ((1, 0), (3, 57), (4, int(off[5] - off[4]) - 1)):
        dirty = f0.copy()
        dirty[off[u] + t] = np.nan
        got = G.cmvn(ctx, plan, gs, dev(torch, dirty)).cpu().numpy()
        want = oracle.cmvn(global_stats, dirty[off[u]:off[u + 1]])
        mine = got[off[u]:off[u + 1]]
        assert np.isnan(want[t]).all() and np.array_equal(np.isnan(mine), np.isnan(want)), (u, t)
        fin = ~np.isnan(want)
        assert np.array_equal(bits(mine)[fin], bits(want)[fin]), (u, t)
        others = np.ones(len(got), bool)
        others[off[u]:off[u + 1]] = False
        assert np.array_equal(bits(got)[others], bits(clean)[others]), (u, t)


# -------------------------------------------------------- isolation: nnet --

NNET_MODES = {"fp32": ("plain", "fp32"), "bf16x6": ("plain", "bf16x6"), "bf16x6p": ("plain", "bf16x6p"),
              "bf16": ("plain", "bf16"), "latency": ("latency", "bf16x6")}


@functools.lru_cache(maxsize=None)
def nnet_case():
    """Geometry A with real weights, a 70-row block and the same block with a
    NaN in one input row; the float64 evaluation's NaN rows."""
    in_d, widths, splices, post = netgen.GEOMETRIES["A"]
    layers = netgen.real_net(in_d, widths, splices, post, 8900)
    left, right = netgen.context(layers)
    x = netgen.real_input(layers, 70, 8901)
    dirty = x.copy()
    dirty[31, 7] = np.nan
    want = netgen.eval_f64(layers, dirty)
    nan_rows = np.isnan(want).any(axis=1)
    # the output rows whose context covers input row 31, and all of each
    assert nan_rows.tolist() == [31 - left - right <= j <= 31 for j in range(70)] and nan_rows.sum() == left + right + 1
    assert np.isnan(want[nan_rows]).all()
    return layers, x, dirty, nan_rows


@pytest.mark.parametrize("mode", list(NNET_MODES))
def test_nnet_keeps_a_nan_row_in_its_context(torch, G, ctx, mode):
    layers, x, dirty, nan_rows = nnet_case()
    flavour, gemm = NNET_MODES[mode]
    c = ctx
    if flavour == "latency":
        c = G.Context(0)
        c.set_latency(True)
    model = G.Model(c, image=netgen.image(layers)).set_gemm(gemm)
    assert model.gemm == gemm
    clean = G.nnet_propagate(c, model, dev(torch, x)).cpu().numpy()
    assert clean.shape == (70, 772) and np.isfinite(clean).all()
    got = G.nnet_propagate(c, model, dev(torch, dirty)).cpu().numpy()
    assert np.isnan(got[nan_rows]).all()
    assert np.array_equal(bits(got[~nan_rows]), bits(clean[~nan_rows]))
