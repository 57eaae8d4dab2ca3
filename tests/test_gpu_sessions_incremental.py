"""Incremental session sets (CE_GPU_SESSIONS_INCREMENTAL: per-layer context
caches, k + H packed rows per slot and push instead of k + L + R;
catears_amd/csrc/sessions.cc, session_ctx_exchange_kernel).

The contract is the plain set's: whatever the pushes, a slot's rows are, bit
for bit, the one-shot ce_gpu_score rows of its samples on the same context.
Comparisons are on uint32 views, zero tolerance."""
import ctypes

import numpy as np
import pytest

from test_gpu_parity import dev
from test_gpu_sessions import (L, R, check_jobs, constant_chunks, one_shot, run_jobs, same, samples_for, slot_jobs,
                               stream_one)
from test_sessions_incremental_cpu import ASYM

pytestmark = pytest.mark.gpu

H = 6  # TDNN-XS / TDNN-S: spans 4, 2, 2, 6, 6, 0, 0


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
def model(G, ctx, xs_config):
    m = G.Model(ctx, xs_config)
    assert (m.left, m.right) == (L, R)
    return m


@pytest.fixture(scope="module")
def gs(torch, global_stats):
    return dev(torch, global_stats)


def inc_set(G, ctx, model, n_slots, max_chunk, gstats):
    sess = G.Sessions(ctx, model, n_slots, max_chunk, gstats, incremental=True)
    assert sess.stats() == {"lead_rows": H, "pushes": 0, "packed_rows": 0, "chunks": 0}
    return sess


# ------------------------------------------------- 1. against the one-shot --

@pytest.fixture(scope="module")
def utt3s(torch, G, ctx, model, gs):
    from catears_amd import synth
    wave = synth.pcm(1900, 48000)
    return wave, one_shot(torch, G, ctx, model, wave, gs)


@pytest.mark.parametrize("chunk", [160, 161, 400, 1600, 48000])
def test_chunk_sizes(torch, G, ctx, model, gs, utt3s, chunk):
    wave, ref = utt3s
    counts = constant_chunks(len(wave), chunk)
    sess = inc_set(G, ctx, model, 1, chunk, gs)
    try:
        got = stream_one(torch, G, sess, 0, wave, counts)
        st = sess.stats()
    finally:
        sess.close()
    assert ref.shape == (298, 512) and same(got, ref)
    want = G.Sessions.packed_rows(L, R, H, counts, len(counts) - 1, True)
    assert st["packed_rows"] == sum(want) and st["pushes"] == len(counts)
    assert st["chunks"] == sum(1 for w in want if w)


def test_chunk_one_sample(torch, G, ctx, model, gs):
    from catears_amd import synth
    wave = synth.pcm(1901, 1000)
    ref = one_shot(torch, G, ctx, model, wave, gs)
    sess = inc_set(G, ctx, model, 1, 1, gs)
    try:
        got = stream_one(torch, G, sess, 0, wave, [1] * 1000)
    finally:
        sess.close()
    assert ref.shape[0] == 4 and same(got, ref)


def test_chunks_ragged_with_empty_pushes(torch, G, ctx, model, gs, utt3s):
    wave, ref = utt3s
    rng = np.random.default_rng(1902)
    counts, left = [], len(wave)
    while left:
        c = min(left, int(rng.choice([0, 0, 1, 37, 160, 399, 400, 1599, 3000])))
        counts.append(c)
        left -= c
    assert counts.count(0) >= 3
    sess = inc_set(G, ctx, model, 1, 3000, gs)
    try:
        got = stream_one(torch, G, sess, 0, wave, counts)
    finally:
        sess.close()
    assert same(got, ref)


@pytest.mark.parametrize("frames", [0, 1, 2, R, R + 1])
def test_edge_utterances(torch, G, ctx, model, gs, frames):
    """Utterances up to one frame longer than the right context (with at most
    R frames nothing is out before the EOS), pushed three ways: a frame at a
    time with the EOS on a push without samples, everything with the EOS in
    the first push, and the same again after a reset of the used slot."""
    from catears_amd import synth
    wave = synth.pcm(1920 + frames, samples_for(frames) if frames else 399)
    ref = one_shot(torch, G, ctx, model, wave, gs)
    assert ref.shape[0] == frames
    steps = ([400] + [160] * (frames - 1) if frames else [399]) + [0]
    sess = inc_set(G, ctx, model, 2, 4000, gs)
    try:
        a = stream_one(torch, G, sess, 0, wave, steps)
        held = min(frames, R)  # R + 1 frames: one row is out before the EOS
        assert G.Sessions.schedule(L, R, steps, len(steps) - 1)[1][-2:] == ([frames - held, held] if frames else [0, 0])
        b = stream_one(torch, G, sess, 1, wave, [len(wave)])
        sess.reset(0)
        c = stream_one(torch, G, sess, 0, wave, [len(wave)])
    finally:
        sess.close()
    assert same(a, ref) and same(b, ref) and same(c, ref)


# ---------------------------------------------------------- 2. the slot mix --

def test_slot_mix(torch, G, ctx, model, gs):
    """37 slots; every tick pushes a random subset with random counts (some
    empty), slots skip ticks, some are reset in mid-utterance and reused."""
    from catears_amd import synth
    rng = np.random.default_rng(1930)
    n_slots, sizes = 37, [0, 1, 160, 399, 400, 801, 1600]
    todo = {s: 2 for s in range(n_slots)}
    cur, rows, done, seed, dropped = {}, {}, [], 0, 0
    sess = inc_set(G, ctx, model, n_slots, 1600, gs)
    try:
        while todo or cur:
            slots, counts, eos, pieces = [], [], [], []
            for s in range(n_slots):
                if s not in cur:
                    if s not in todo:
                        continue
                    todo[s] -= 1
                    if not todo[s]:
                        del todo[s]
                    seed += 1
                    cur[s], rows[s] = [synth.pcm(2000 + seed, int(rng.integers(300, 9000))), 0], []
                    sess.reset(s)
                if rng.random() < 0.3:
                    continue  # the slot skips this tick
                wave, at = cur[s]
                if at > 2000 and rng.random() < 0.03:  # abandoned in mid-utterance
                    del cur[s]
                    dropped += 1
                    todo[s] = todo.get(s, 0) + 1
                    continue
                c = min(len(wave) - at, int(rng.choice(sizes)))
                slots.append(s), counts.append(c), eos.append(at + c == len(wave)), pieces.append(wave[at:at + c])
                cur[s][1] += c
            if not slots:
                continue
            order = rng.permutation(len(slots))
            slots, counts, eos, pieces = ([v[i] for i in order] for v in (slots, counts, eos, pieces))
            pcm = np.concatenate(pieces) if sum(counts) else np.zeros(1, np.float32)
            out, n = sess.push(slots, dev(torch, pcm), counts, eos=eos)
            out = out.cpu().numpy()
            at = 0
            for s, r, e in zip(slots, n, eos):
                rows[s].append(out[at:at + r])
                at += int(r)
                if e:
                    done.append((s, cur.pop(s)[0], np.concatenate(rows[s])))
            assert at == len(out)
    finally:
        sess.close()
    assert len(done) == 2 * n_slots and dropped >= 1
    for s, wave, got in done:
        assert same(got, one_shot(torch, G, ctx, model, wave, gs)), (s, len(wave))


# ---------------------------------------------------------- 3. chunk seams --

def test_push_of_two_chunks(torch, G, ctx, model, gs):
    """300 running slots x 1600 samples: 300 blocks of 10 + 6 rows, so the
    push runs as two chunks (256 blocks fill the first); then the EOS of all
    of them on a push without samples (10 + 6 rows again)."""
    from catears_amd import synth
    base = [synth.pcm(2100 + i, 4000) for i in range(4)]
    waves = [np.roll(base[s % 4], 7 * s) for s in range(300)]
    slots = list(range(300))
    sess = inc_set(G, ctx, model, 300, 2400, gs)
    try:
        _, n0 = sess.push(slots, dev(torch, np.concatenate([w[:2400] for w in waves])), [2400] * 300)
        before = sess.stats()
        out1, n1 = sess.push(slots, dev(torch, np.concatenate([w[2400:] for w in waves])), [1600] * 300)
        st = sess.stats()
        out2, n2 = sess.push(slots, None, [0] * 300, eos=[True] * 300)
        out1, out2 = out1.cpu().numpy(), out2.cpu().numpy()
    finally:
        sess.close()
    assert list(n0) == [3] * 300 and list(n1) == [10] * 300 and list(n2) == [10] * 300
    assert st["packed_rows"] - before["packed_rows"] == 300 * 16 and st["chunks"] - before["chunks"] == 2
    for s in (0, 1, 2, 3, 254, 255, 256, 257, 299):  # both sides of the seam among them
        ref = one_shot(torch, G, ctx, model, waves[s], gs)
        assert same(out1[10 * s:10 * s + 10], ref[3:13]) and same(out2[10 * s:10 * s + 10], ref[13:]), s


def test_block_larger_than_a_chunk(torch, G, ctx, model, gs):
    from catears_amd import synth
    wave = synth.pcm(2110, 660000)
    sess = inc_set(G, ctx, model, 1, 660000, gs)
    try:
        out, rows = sess.push([0], dev(torch, wave), [660000], eos=[True])
        got = out.cpu().numpy()
        st = sess.stats()
    finally:
        sess.close()
    assert list(rows) == [4123]
    assert st["chunks"] == 2 and st["packed_rows"] == 4123 + L + R + 2 * H
    assert st["packed_rows"] == G.Sessions.packed_rows(L, R, H, [660000], 0, True)[0]
    assert same(got, one_shot(torch, G, ctx, model, wave, gs))


# ---------------------------------------------------------------- 4. modes --

def calibrated(torch, G, c, m):
    from catears_amd import synth
    waves = [synth.pcm(60 + i, 16000 * 3) for i in range(3)]
    plan = G.Plan(c, [len(w) for w in waves], m)
    ranges = m.calibrate(c, plan, G.fbank(c, plan, dev(torch, np.concatenate(waves))))
    return m.quantize_static(c, ranges)


@pytest.mark.parametrize("mode", ["fp32", "latency", "bf16", "i8", "i8_latency", "fast_fbank", "no_cmvn", "s16"])
def test_modes(torch, G, xs_config, gs, mode):
    c = G.Context(0)
    m = G.Model(c, xs_config)
    if mode in ("latency", "i8_latency"):
        c.set_latency(True)
    if mode in ("fp32", "bf16"):
        m.set_gemm(mode)
    if mode in ("i8", "i8_latency"):
        calibrated(torch, G, c, m)
    if mode == "fast_fbank":
        c.set_fbank("fast")
    gstats = None if mode == "no_cmvn" else gs
    jobs = slot_jobs(3)
    launches = G.debug_i8_latency_launches()
    sess = inc_set(G, c, m, 3, 1600, gstats)
    try:
        got = run_jobs(torch, G, sess, jobs, s16=mode == "s16")
    finally:
        sess.close()
    if mode == "i8_latency":  # the split-K pair did run
        assert G.debug_i8_latency_launches() > launches
    check_jobs(torch, G, c, m, gstats, jobs, got)


# ------------------------------------------- 5. a net off the TDNN shapes --

def stream_any(torch, sess, wave, counts):
    """stream_one for any context: rows of slot 0, the EOS with the last push."""
    got, at = [], 0
    pcm = dev(torch, wave)
    for i, c in enumerate(counts):
        out, rows = sess.push([0], pcm[at:at + c], [c], eos=[i == len(counts) - 1])
        got.append(out.cpu().numpy())
        at += c
    assert at == len(wave)
    return np.concatenate(got)


@pytest.mark.parametrize("mode", ["bf16x6", "bf16", "i8"])
def test_asymmetric_net(torch, G, gs, mode):
    """L = 7, R = 8, H = 6: spans 4, 5, 0, 6, 0 -- asymmetric offsets, a
    zero-span layer in mid-chain; hidden 128, so the static int8 form has a
    pre-spliced first layer, fused boundaries and a layer read through
    shifted offsets."""
    from catears_amd import formats, synth
    layers, left, right, prior = synth.tdnn_layers(128, 96, splices=ASYM)
    c = G.Context(0)
    m = G.Model(c, image=formats.nnet_bytes(layers, left, right), prior=prior)
    assert (m.left, m.right) == (7, 8)
    if mode == "i8":
        calibrated(torch, G, c, m)
    else:
        m.set_gemm(mode)
    wave = synth.pcm(2200, samples_for(33))
    ref = G.score(c, m, G.Plan(c, [len(wave)], m), dev(torch, wave), gs).cpu().numpy()
    assert ref.shape == (33, 96)
    sess = G.Sessions(c, m, 1, len(wave), gs, incremental=True)
    try:
        assert sess.stats()["lead_rows"] == 6
        frame_by_frame = stream_any(torch, sess, wave, [400] + [160] * 32)
        sess.reset(0)
        at_once = stream_any(torch, sess, wave, [len(wave)])
    finally:
        sess.close()
    assert same(frame_by_frame, ref) and same(at_once, ref)


# ------------------------------------------- 6. same pushes, two sets --

def two_sets(torch, G, config, gs, n_slots, ticks, tick_samples, prepare=None):
    """An incremental set and a plain one on two contexts get the same pushes:
    the same rows; each push's packed rows are Sessions.packed_rows', fewer
    for the incremental set at every tick both score rows after a slot's
    first (which feeds the L copies of frame 0), and fewer in all."""
    from catears_amd import synth
    ctxs = [G.Context(0), G.Context(0)]
    models = [G.Model(c, config) for c in ctxs]
    if prepare:
        for c, m in zip(ctxs, models):
            prepare(c, m)
    sets = [G.Sessions(ctxs[0], models[0], n_slots, tick_samples, gs, incremental=True),
            G.Sessions(ctxs[1], models[1], n_slots, tick_samples, gs)]
    base = [synth.pcm(2300 + i, ticks * tick_samples) for i in range(4)]
    slots = list(range(n_slots))
    total = [0, 0]
    try:
        assert [s.stats()["lead_rows"] for s in sets] == [H, 0]
        for t in range(ticks):
            at = t * tick_samples
            pcm = dev(torch, np.concatenate([np.roll(base[s % 4], 3 * s)[at:at + tick_samples] for s in slots]))
            last = t == ticks - 1
            outs = []
            for sess in sets:
                before = sess.stats()["packed_rows"]
                out, rows = sess.push(slots, pcm, [tick_samples] * n_slots, eos=[last] * n_slots)
                outs.append((out.cpu().numpy(), list(rows), sess.stats()["packed_rows"] - before))
            assert outs[0][1] == outs[1][1] and same(outs[0][0], outs[1][0]), t
            for (_, _, packed), inc in zip(outs, (True, False)):
                per_slot = G.Sessions.packed_rows(L, R, H, [tick_samples] * (t + 1), t if last else None, inc)[-1]
                assert packed == n_slots * per_slot, (t, inc)
            total = [total[0] + outs[0][2], total[1] + outs[1][2]]
            if t > 0 and outs[1][2] > 0:
                assert outs[0][2] < outs[1][2], t
        assert total[0] < total[1], total
    finally:
        for sess in sets:
            sess.close()


def test_two_sets_tdnn_xs(torch, G, xs_config, gs):
    two_sets(torch, G, xs_config, gs, 5, 8, 480)


def test_two_sets_tdnn_s(torch, G, s_config, gs):
    two_sets(torch, G, s_config, gs, 64, 3, 1600)


# ------------------------------------------- 7. no allocation once warm --

def test_no_allocation_once_warm(torch, G, ctx, model, gs):
    from catears_amd import synth
    jobs = {s: [(synth.pcm(2400 + s, 21 * 1600), 1600)] for s in range(3)}
    seen = {}

    def on_tick(t):
        if t in (1, 21):
            seen[t] = G.debug_counters()
    sess = inc_set(G, ctx, model, 3, 1600, gs)
    try:
        got = run_jobs(torch, G, sess, jobs, on_tick=on_tick)
    finally:
        sess.close()
    assert sorted(seen) == [1, 21] and seen[1] == seen[21], seen
    check_jobs(torch, G, ctx, model, gs, jobs, got)


# ------------------------------------------------------------ 8. refusals --

def test_refusals(torch, G, xs_config, gs):
    from catears_amd import synth
    c = G.Context(0)
    m = G.Model(c, xs_config)
    for planes in ("bf16x6p", "f16x3"):
        m.set_gemm(planes)
        with pytest.raises(G.CatearsError) as e:
            G.Sessions(c, m, 1, 1600, gs, incremental=True)
        assert e.value.code == -6, planes
    m.set_gemm("bf16x6")
    h = ctypes.c_void_p()
    for flags in (2, 3, 0x80000000):
        rc = G.lib().ce_gpu_sessions_create_ex(c.h, m.h, ctypes.c_void_p(gs.data_ptr()), 1, 1600, flags,
                                               ctypes.byref(h))
        assert rc == -2 and not h.value, flags
    # the GEMM mode changes under a live set: the push is refused and changes nothing
    wave = synth.pcm(2500, 8000)
    ref = one_shot(torch, G, c, m, wave, gs)
    pcm = dev(torch, wave)
    sess = G.Sessions(c, m, 1, 4000, gs, incremental=True)
    try:
        a, _ = sess.push([0], pcm[:4000], [4000])
        a = a.cpu().numpy()
        m.set_gemm("bf16")
        with pytest.raises(G.CatearsError) as e:
            sess.push([0], pcm[4000:], [4000], eos=[True])
        assert e.value.code == -2
        m.set_gemm("bf16x6")
        b, _ = sess.push([0], pcm[4000:], [4000], eos=[True])
        assert same(np.concatenate([a, b.cpu().numpy()]), ref)
    finally:
        sess.close()
    m8 = G.Model(c, xs_config).quantize(c)
    with pytest.raises(G.CatearsError) as e:
        G.Sessions(c, m8, 1, 1600, gs, incremental=True)
    assert e.value.code == -6
