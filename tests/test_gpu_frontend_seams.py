"""The front-end kernels at their seams, against the oracle (which
tests/test_oracle_vs_reference.py ties to the reference's own code).

cmvn_kernel walks the rounding chain in three phases (t < 599, t = 599,
t >= 600) in tiles of 48 frames, prefetching the next tile from a clamped base
and finishing with a per-row clamped partial tile; cmvn_resume_kernel continues
it from any frame in tiles of 4; the fbank kernel gives the eight frames of a
wave to whatever utterances they belong to.  The cases sit on both sides of
every one of those boundaries (tests/seams.py), with the global counts that
take both sides of the alpha select (g_count 200: alpha == 1.0f) and an alpha
above 1.
"""
import numpy as np
import pytest

import seams
from catears_amd import synth

pytestmark = pytest.mark.gpu

FEAT_TOL = 1e-5    # log-mel, as tests/test_gpu_parity.py
SYNTH_TOL = 2e-4   # the fast fbank mode on synthetic audio, as tests/test_gpu_fbank_fast.py


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


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def samples_for(frames):
    return 400 + 160 * (frames - 1) if frames else 0


# ------------------------------------------------------------ ce_gpu_cmvn --

# the 26 seam frame counts with three zero-frame utterances (0, 399 and 1
# samples) between them
CMVN_SAMPLES = [samples_for(t) for t in seams.SEAM_T]
for _at, _n in ((3, 0), (14, 399), (23, 1)):
    CMVN_SAMPLES.insert(_at, _n)


@pytest.fixture(scope="module")
def cmvn_rows():
    """Feature rows ~ N(12, 4) of their own per utterance (the kernel cannot
    pass by reading a neighbour's rows).  Read-only."""
    rng = np.random.default_rng(77)
    out = []
    for n in CMVN_SAMPLES:
        x = rng.normal(12.0, 4.0, size=(0 if n < 400 else 1 + (n - 400) // 160, 40)).astype(np.float32)
        x.setflags(write=False)
        out.append(x)
    return out


def run_cmvn(torch, G, ctx, g, feats, samples):
    plan = G.Plan(ctx, samples)
    assert plan.total_frames == sum(len(x) for x in feats)
    out = G.cmvn(ctx, plan, dev(torch, g), dev(torch, np.concatenate(feats)))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    off = plan.frame_offsets
    return [o[off[u]:off[u + 1]] for u in range(len(feats))]


@pytest.mark.parametrize("count", seams.GPU_COUNTS)
def test_cmvn_seam_frame_counts(torch, G, ctx, oracle, global_stats, cmvn_rows, count):
    """One launch, one wave per utterance: every utterance's rows are the
    oracle's bits, and the same bits when the batch is reversed."""
    g = seams.rescaled_stats(global_stats, count)
    assert [len(x) for x in cmvn_rows if len(x)] == list(seams.SEAM_T) and sum(len(x) == 0 for x in cmvn_rows) == 3
    got = run_cmvn(torch, G, ctx, g, cmvn_rows, CMVN_SAMPLES)
    for u, x in enumerate(cmvn_rows):
        want = oracle.cmvn(g, x)
        bad = np.flatnonzero((bits(got[u]) != bits(want)).any(axis=1)) if got[u].shape == want.shape else [-1]
        assert not len(bad), f"g_count {count}, T {len(x)}: {len(bad)} rows differ, first {bad[0]}"
    back = run_cmvn(torch, G, ctx, g, cmvn_rows[::-1], CMVN_SAMPLES[::-1])[::-1]
    for u, x in enumerate(cmvn_rows):
        assert same(back[u], got[u]), f"g_count {count}, T {len(x)}: depends on the batch order"


# --------------------------------------------------------------- sessions --

SESSION_FRAMES = 700


def session_pushes():
    """Per slot the frame count of every push, 700 frames in all: 13 rounds of
    1 .. 9 (585 frames), a connecting push, small pushes through the regime
    changes, then 1 .. 9 again.  Between them the three slots start a push at
    every frame from 592 to 608."""
    through = {0: [7, 1, 2, 3, 4, 5], 1: [9, 2, 3, 2, 3, 2], 2: [9, 3, 3, 3, 2, 3]}
    out = []
    for slot in range(3):
        ks = list(range(1, 10)) * 13 + through[slot]
        i = 0
        while sum(ks) < SESSION_FRAMES:
            ks.append(min(1 + i % 9, SESSION_FRAMES - sum(ks)))
            i += 1
        out.append(ks)
    return out


def test_session_pushes_cover_the_seams():
    starts, near = set(), []
    for ks in session_pushes():
        assert sum(ks) == SESSION_FRAMES and set(ks) == set(range(1, 10))
        t0 = np.cumsum([0] + ks[:-1]).tolist()
        starts |= set(t0)
        near += [(t, k) for t, k in zip(t0, ks) if 592 <= t <= 608]
    assert set(range(592, 609)) <= starts
    # cmvn_resume_kernel's tiles of 4 start at the push's first frame: every
    # start residue, and a last tile of every size
    assert {t % 4 for t, _ in near} == {0, 1, 2, 3} and {k % 4 for _, k in near} == {0, 1, 2, 3}
    # pushes that end on, start on and straddle t = 599 (plain) and t = 600
    assert any(t + k == 599 for t, k in near) and any(t < 599 < t + k - 1 for t, k in near)
    assert any(t + k == 600 for t, k in near) and any(t == 600 for t, k in near)


def test_sessions_resume_across_the_regimes(torch, G, ctx, oracle, global_stats, xs_config):
    """Three slots streamed through frames 592 .. 608 with a push starting at
    every one of them, on to 700 frames (the raw ring of 600 + a push's
    frames wraps): the rows are the one-shot score's bits; and the one-shot
    CMVN of the same audio is the oracle's, with alpha == 1.0f."""
    g = seams.rescaled_stats(global_stats, 200.0)
    gs = dev(torch, g)
    model = G.Model(ctx, xs_config)
    waves = [synth.pcm(930 + s, samples_for(SESSION_FRAMES)) for s in range(3)]
    pushes = session_pushes()
    refs = []
    for w in waves:
        plan = G.Plan(ctx, [len(w)], model)
        pcm = dev(torch, w)
        refs.append(G.score(ctx, model, plan, pcm, gs).cpu().numpy())
        feats = G.fbank(ctx, plan, pcm)
        normed = G.cmvn(ctx, plan, gs, feats).cpu().numpy()
        assert same(normed, oracle.cmvn(g, feats.cpu().numpy()))
    sess = G.Sessions(ctx, model, 3, samples_for(9), gs)
    try:
        got = [[] for _ in range(3)]
        at = [0, 0, 0]
        for i in range(max(len(ks) for ks in pushes)):
            slots = [s for s in range(3) if i < len(pushes[s])]
            counts, eos = [], []
            for s in slots:
                k = pushes[s][i]
                counts.append(samples_for(k) if at[s] == 0 else 160 * k)
                eos.append(i == len(pushes[s]) - 1)
            pcm = dev(torch, np.concatenate([waves[s][at[s]:at[s] + c] for s, c in zip(slots, counts)]))
            out, rows = sess.push(slots, pcm, counts, eos=eos)
            out = out.cpu().numpy()
            r0 = 0
            for s, c, r in zip(slots, counts, rows):
                at[s] += c
                got[s].append(out[r0:r0 + int(r)])
                r0 += int(r)
    finally:
        sess.close()
    for s in range(3):
        assert at[s] == len(waves[s])
        rows = np.concatenate(got[s])
        assert refs[s].shape == (SESSION_FRAMES, 512) and same(rows, refs[s]), f"slot {s}"


# ----------------------------------------------------- fbank wave sharing --

def run_fbank(torch, G, ctx, waves, dtype=np.float32):
    plan = G.Plan(ctx, [len(w) for w in waves])
    feats = torch.empty((max(plan.total_frames, 1), 40), dtype=torch.float32, device="cuda")
    mel = torch.empty_like(feats)
    G.fbank(ctx, plan, dev(torch, np.concatenate(waves).astype(dtype)), feats, mel)
    torch.cuda.synchronize()
    off = plan.frame_offsets
    f, m = feats.cpu().numpy(), mel.cpu().numpy()
    return [(f[off[u]:off[u + 1]], m[off[u]:off[u + 1]]) for u in range(len(waves))]


@pytest.fixture(scope="module")
def short_utts(oracle):
    """200 utterances of 0 .. 9 frames (every few frames another utterance,
    often several inside one wave's eight), six zero-frame ones in a row, and
    the eight candidates for a last utterance; with the oracle's rows."""
    rng = np.random.default_rng(41)
    frames = rng.integers(0, 10, size=200)
    frames[90:96] = 0
    assert set(frames.tolist()) == set(range(10))
    slack = rng.integers(0, 160, size=208)      # samples past the last whole frame
    sizes = [samples_for(int(t)) + int(s) if t else int(s) * 2 for t, s in zip(frames, slack)]
    waves = [synth.pcm(7000 + i, n) for i, n in enumerate(sizes)]
    lasts = [synth.pcm(7300 + k, samples_for(k + 1) + int(slack[200 + k])) for k in range(8)]
    fb = oracle.Fbank()
    want = [fb.compute(w, with_mel=True) for w in waves + lasts]
    assert [len(f) for f, _ in want[:200]] == frames.tolist()
    return waves, lasts, want[:200], want[200:]


@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "s16"])
def test_fbank_waves_shared_between_utterances(torch, G, ctx, short_utts, dtype):
    """Eight plans that differ in their last utterance only, so that the last
    wave holds 1 .. 8 live frames: pre-log mel bit for bit, log-mel within
    FEAT_TOL, through the float and the int16 entry points."""
    waves, lasts, want, want_last = short_utts
    seen = set()
    for k, last in enumerate(lasts):
        got = run_fbank(torch, G, ctx, waves + [last], dtype)
        seen.add(sum(len(f) for f, _ in got) % 8)
        for u, ((f, m), (of, om)) in enumerate(zip(got, want + [want_last[k]])):
            assert same(m, om), f"last {k}, utt {u} ({len(of)} frames): pre-log mel"
            assert not len(of) or np.abs(f - of).max() <= FEAT_TOL, f"last {k}, utt {u}"
    assert seen == set(range(8))


def test_fbank_fast_mode_on_shared_waves(torch, G, short_utts):
    waves, lasts, want, want_last = short_utts
    fctx = G.Context(0)
    fctx.set_fbank("fast")
    got = run_fbank(torch, G, fctx, waves + [lasts[2]])
    for u, ((f, _), (of, _)) in enumerate(zip(got, want + [want_last[2]])):
        assert f.shape == of.shape and (not len(of) or np.abs(f - of).max() <= SYNTH_TOL), f"utt {u}"


# ------------------------------------------------------- second grid pass --

def test_fbank_second_grid_pass(torch, G, ctx, oracle):
    """34 utterances of 998 frames: 33 932 frames, past the 32 768 the grid
    covers in one pass, so the grid-stride loop runs a second time (until now
    only the 998 000-frame test reached it)."""
    base = [synth.pcm(7500 + i, 160000) for i in range(4)]
    fb = oracle.Fbank()
    want = [fb.compute(w, with_mel=True) for w in base]
    got = run_fbank(torch, G, ctx, [base[u % 4] for u in range(34)])
    assert sum(len(f) for f, _ in got) == 33932 > 512 * 64
    for u, (f, m) in enumerate(got):
        of, om = want[u % 4]
        assert same(m, om), f"utt {u}: pre-log mel"
        assert np.abs(f - of).max() <= FEAT_TOL, f"utt {u}"
