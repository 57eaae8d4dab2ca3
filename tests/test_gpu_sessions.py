"""Device-resident sessions (ce_gpu_sessions_*, catears_amd/csrc/sessions.cc,
kernels/sessions.hip): live audio pushed in pieces to n_slots slots whose
sample tail, CMVN chain and nnet context stay on the device.

The contract is exact: whatever the chunking, the slot mix of a push or the
push order, the rows a slot emitted up to its end of stream are, bit for
bit, the rows the one-shot ce_gpu_score gives for the same samples on the
same context (same GEMM mode, latency and fbank settings, same CMVN stats).
That one-shot path is itself held to the oracle by the rest of the suite;
one test here pins the streamed rows to the oracle directly.  Comparisons
are on uint32 views, zero tolerance, unless stated."""
import ctypes

import numpy as np
import pytest

from test_gpu_parity import LOGLIK_TOL, bits, dev

pytestmark = pytest.mark.gpu

L = R = 10  # TDNN-XS / TDNN-S context


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


def one_shot(torch, G, ctx, model, wave, gstats):
    """ce_gpu_score of one utterance: the reference of every test here."""
    if G.num_frames(len(wave)) == 0:
        return np.zeros((0, model.num_pdfs), np.float32)
    plan = G.Plan(ctx, [len(wave)], model)
    return G.score(ctx, model, plan, dev(torch, wave), gstats).cpu().numpy()


def constant_chunks(total, chunk):
    return [min(chunk, total - at) for at in range(0, total, chunk)]


def stream_one(torch, G, sess, slot, wave, counts, eos_push=True):
    """Streams `wave` to one slot in pushes of counts[i] samples, the last one
    carrying EOS; checks the row count after every push against the contract
    and h_rows_out against Sessions.schedule.  Returns the concatenated rows."""
    assert sum(counts) == len(wave)
    frames_want, rows_want = G.Sessions.schedule(L, R, counts, len(counts) - 1 if eos_push else None)
    total = sum(rows_want)
    out = torch.empty((max(total, 1), sess.model.num_pdfs), dtype=torch.float32, device="cuda")
    pcm = dev(torch, wave) if len(wave) else torch.zeros(1, dtype=torch.float32, device="cuda")
    at = got = 0
    for i, c in enumerate(counts):
        last = eos_push and i == len(counts) - 1
        _, rows = sess.push([slot], pcm[at:at + c], [c], eos=[last], out=out[got:])
        at += c
        got += int(rows[0])
        assert int(rows[0]) == rows_want[i], (i, c)
        if not last:
            assert got == max(0, G.num_frames(at) - R), (i, c)
    assert got == total and (not eos_push or total == G.num_frames(len(wave)))
    return out[:got].cpu().numpy()


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------ 1. chunk sizes --

@pytest.fixture(scope="module")
def utt3s(torch, G, ctx, model, gs):
    from catears_amd import synth
    wave = synth.pcm(900, 48000)
    return wave, one_shot(torch, G, ctx, model, wave, gs)


@pytest.mark.parametrize("chunk", [159, 160, 161, 399, 400, 401, 777, 1600, 48000])
def test_chunk_sizes(torch, G, ctx, model, gs, utt3s, chunk):
    wave, ref = utt3s
    sess = G.Sessions(ctx, model, 1, chunk, gs)
    try:
        got = stream_one(torch, G, sess, 0, wave, constant_chunks(len(wave), chunk))
    finally:
        sess.close()
    assert ref.shape == (298, 512) and same(got, ref)


def test_chunk_one_sample(torch, G, ctx, model, gs):
    from catears_amd import synth
    wave = synth.pcm(901, 1000)
    ref = one_shot(torch, G, ctx, model, wave, gs)
    sess = G.Sessions(ctx, model, 1, 1, gs)
    try:
        got = stream_one(torch, G, sess, 0, wave, [1] * 1000)
    finally:
        sess.close()
    assert ref.shape[0] == 4 and same(got, ref)


def test_chunks_ragged_with_empty_pushes(torch, G, ctx, model, gs, utt3s):
    wave, ref = utt3s
    rng = np.random.default_rng(902)
    counts, left = [], len(wave)
    while left:
        c = min(left, int(rng.choice([0, 0, 1, 37, 160, 399, 400, 1599, 3000])))
        counts.append(c)
        left -= c
    assert counts.count(0) >= 3
    sess = G.Sessions(ctx, model, 1, 3000, gs)
    try:
        got = stream_one(torch, G, sess, 0, wave, counts)
    finally:
        sess.close()
    assert same(got, ref)


# ------------------------------------------- 2. CMVN regimes and ring wrap --

def samples_for(frames):
    return 400 + 160 * (frames - 1)


def test_cmvn_regimes_and_ring_wrap(torch, G, ctx, model, gs):
    """15 s (1498 frames): pushes ending at frames 598, 599, 600 and 601 (one
    of them a single frame) in 100 ms chunks -- the 610-row raw ring and the
    31-row normalised ring wrap many times -- and one push that crosses the
    smoothing, plain and windowed regimes at once."""
    from catears_amd import synth
    wave = synth.pcm(910, 240000)
    ref = one_shot(torch, G, ctx, model, wave, gs)
    assert ref.shape[0] == 1498
    cuts = sorted(set(range(0, 240001, 1600)) | {samples_for(f) for f in (598, 599, 600, 601)})
    counts = [b - a for a, b in zip(cuts, cuts[1:])]
    assert 160 in counts and max(counts) == 1600
    sess = G.Sessions(ctx, model, 1, 1600, gs)
    try:
        small = stream_one(torch, G, sess, 0, wave, counts)
    finally:
        sess.close()
    assert same(small, ref)
    sess = G.Sessions(ctx, model, 1, 160000, gs)
    try:
        big = stream_one(torch, G, sess, 0, wave, [160000, 80000])
    finally:
        sess.close()
    assert same(big, ref)
    # the staged path too: ce_gpu_cmvn + ce_gpu_am_forward on the one-shot fbank
    plan = G.Plan(ctx, [len(wave)], model)
    feats = G.fbank(ctx, plan, dev(torch, wave))
    staged = G.am_forward(ctx, model, plan, G.cmvn(ctx, plan, gs, feats)).cpu().numpy()
    assert same(small, staged)


# ------------------------------------------------------ 3. edge utterances --

def test_edge_utterances(torch, G, ctx, model, gs):
    from catears_amd import synth
    wave = synth.pcm(920, 400 + 160 * 9)
    sess = G.Sessions(ctx, model, 2, 4000, gs)
    try:
        # 399 samples: no frame, no row
        got = stream_one(torch, G, sess, 0, wave[:399], [399])
        assert got.shape[0] == 0
        # a push after EOS is refused, and leaves the slot as it was
        with pytest.raises(G.CatearsError) as e:
            sess.push([0], dev(torch, wave[:160]), [160])
        assert e.value.code == -2
        # 400 samples: one row
        sess.reset(0)
        got = stream_one(torch, G, sess, 0, wave[:400], [400])
        assert got.shape[0] == 1 and same(got, one_shot(torch, G, ctx, model, wave[:400], gs))
        # 10 frames (<= R): nothing until EOS, then all 10; EOS on an empty push
        sess.reset(0)
        ref = one_shot(torch, G, ctx, model, wave, gs)
        counts = [400] + [160] * 9 + [0]
        got = stream_one(torch, G, sess, 0, wave, counts)
        assert G.Sessions.schedule(L, R, counts, len(counts) - 1)[1] == [0] * 10 + [10]
        assert ref.shape[0] == 10 and same(got, ref)
        # after a reset the slot gives a fresh slot's bits (slot 1 never used)
        sess.reset(0)
        a = stream_one(torch, G, sess, 0, wave, [777, 1063])
        b = stream_one(torch, G, sess, 1, wave, [777, 1063])
        assert same(a, ref) and same(b, ref)
    finally:
        sess.close()


# ----------------------------------------------------------- 4. many slots --

def run_jobs(torch, G, sess, jobs, s16=False, on_tick=None):
    """jobs[slot] = [(wave, chunk), ...]: the utterances a slot streams one
    after another (reset between them), `chunk` samples per push.  Every
    tick pushes the slots that still have data, in an order that rotates and
    flips from tick to tick.  Returns {(slot, k): rows of its k-th utterance}."""
    state = {s: [0, 0, False] for s in jobs}  # utterance index, sample position, ended
    pieces = {}
    held = []
    tick = 0
    while True:
        active = [s for s in sorted(jobs) if state[s][0] < len(jobs[s])]
        if not active:
            break
        k = tick % len(active)
        order = active[k:] + active[:k]
        if tick % 2:
            order.reverse()
        parts, counts, eos = [], [], []
        for s in order:
            u, at, ended = state[s]
            if ended:
                sess.reset(s)
                state[s][2] = False
            wave, chunk = jobs[s][u]
            c = min(chunk, len(wave) - at)
            parts.append(wave[at:at + c])
            counts.append(c)
            eos.append(at + c == len(wave))
        pcm = np.concatenate(parts)
        pcm = pcm.astype(np.int16) if s16 else pcm
        out, rows = sess.push(order, dev(torch, pcm), counts, eos=eos)
        held.append((order, out, rows))
        for s, c, e in zip(order, counts, eos):
            state[s][1] += c
            if e:
                state[s] = [state[s][0] + 1, 0, True]
        tick += 1
        if on_tick:
            on_tick(tick)
    # split every tick's rows back to (slot, utterance): replay the bookkeeping
    state = {s: [0, 0] for s in jobs}
    for order, out, rows in held:
        host = out.cpu().numpy()
        at = 0
        for s, r in zip(order, rows):
            u = state[s][0]
            pieces.setdefault((s, u), []).append(host[at:at + r])
            at += int(r)
            wave, chunk = jobs[s][u]
            state[s][1] += min(chunk, len(wave) - state[s][1])
            if state[s][1] == len(wave):
                state[s] = [u + 1, 0]
        assert at == host.shape[0]
    return {k: np.concatenate(v) for k, v in pieces.items()}


def slot_jobs(n_slots=5):
    from catears_amd import synth
    lens = [8000, 16000, 32000, 52800, 112000][:n_slots]
    chunks = [160, 777, 1600, 4000, 333][:n_slots]
    jobs = {s: [(synth.pcm(930 + s, lens[s]), chunks[s])] for s in range(n_slots)}
    # slots 0 and 1 are reused while the others are mid-stream
    jobs[0].append((synth.pcm(940, 12000), 160))
    jobs[1].append((synth.pcm(941, 9000), 777))
    return jobs


def check_jobs(torch, G, ctx, model, gstats, jobs, got):
    assert sorted(got) == sorted((s, u) for s in jobs for u in range(len(jobs[s])))
    for (s, u), rows in got.items():
        ref = one_shot(torch, G, ctx, model, jobs[s][u][0], gstats)
        assert same(rows, ref), (s, u)


def test_many_slots(torch, G, ctx, model, gs):
    jobs = slot_jobs()
    sess = G.Sessions(ctx, model, 5, 4000, gs)
    try:
        got = run_jobs(torch, G, sess, jobs)
    finally:
        sess.close()
    check_jobs(torch, G, ctx, model, gs, jobs, got)


# ---------------------------------------------------------------- 5. modes --

@pytest.mark.parametrize("mode", ["latency", "fp32", "fast_fbank", "no_cmvn", "s16"])
def test_modes(torch, G, xs_config, gs, mode):
    c = G.Context(0)
    m = G.Model(c, xs_config)
    if mode == "latency":
        c.set_latency(True)
    if mode == "fp32":
        m.set_gemm("fp32")
    if mode == "fast_fbank":
        c.set_fbank("fast")
    gstats = None if mode == "no_cmvn" else gs
    jobs = slot_jobs(3)
    sess = G.Sessions(c, m, 3, 1600, gstats)
    try:
        got = run_jobs(torch, G, sess, jobs, s16=mode == "s16")
    finally:
        sess.close()
    check_jobs(torch, G, c, m, gstats, jobs, got)
    if mode == "s16":  # the one-shot int16 path as well
        wave = jobs[2][0][0]
        plan = G.Plan(c, [len(wave)], m)
        ref = G.score(c, m, plan, dev(torch, wave.astype(np.int16)), gs).cpu().numpy()
        assert same(got[(2, 0)], ref)


# --------------------------------------------------------------- 6. oracle --

def test_streamed_rows_vs_oracle(torch, G, ctx, model, gs, oracle, xs_config, global_stats):
    """Pinned to something other than the library: the oracle's streaming
    path (fbank -> CMVN -> AM in the model's chunk_size), the project's
    log-likelihood bar."""
    from catears_amd import formats, synth
    am = formats.read_am(xs_config)
    wave = synth.pcm(950, 32000)
    sess = G.Sessions(ctx, model, 1, 777, gs)
    try:
        got = stream_one(torch, G, sess, 0, wave, constant_chunks(len(wave), 777))
    finally:
        sess.close()
    want = oracle.am_stream(am, oracle.cmvn(global_stats, oracle.Fbank().compute(wave)), chunk_size=am["chunk"])
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= LOGLIK_TOL


# ----------------------------------------------------------- 7. large push --

def test_large_push_splits_segments(torch, G, ctx, model, gs):
    """Two slots, 60 s each in one call: 5998 rows per slot, more than the
    4096 packed rows of one nnet chunk, so each block is split into segments
    overlapping by L + R."""
    from catears_amd import synth
    waves = [synth.pcm(960 + i, 960000) for i in range(2)]
    sess = G.Sessions(ctx, model, 2, 960000, gs)
    try:
        out, rows = sess.push([1, 0], dev(torch, np.concatenate([waves[1], waves[0]])), [960000, 960000],
                              eos=[True, True])
        got = out.cpu().numpy()
    finally:
        sess.close()
    assert list(rows) == [5998, 5998]
    assert same(got[:5998], one_shot(torch, G, ctx, model, waves[1], gs))
    assert same(got[5998:], one_shot(torch, G, ctx, model, waves[0], gs))


# ------------------------------------------------ 8. TDNN-S, latency mode --

def test_tdnn_s_latency(torch, G, s_config, gs):
    from catears_amd import synth
    c = G.Context(0)
    c.set_latency(True)
    m = G.Model(c, s_config)
    assert (m.left, m.right) == (L, R)
    jobs = {s: [(synth.pcm(970 + s, 32000), 1600)] for s in range(3)}
    sess = G.Sessions(c, m, 3, 1600, gs)
    try:
        got = run_jobs(torch, G, sess, jobs)
    finally:
        sess.close()
    check_jobs(torch, G, c, m, gs, jobs, got)


# ------------------------------------------- 9. no allocation once warm --

def test_no_allocation_once_warm(torch, G, ctx, model, gs):
    """202 ticks of 100 ms for 4 slots (slot 2 ends an utterance, is reset
    and starts another): after the first two, the library's allocation and
    release counts stand still."""
    from catears_amd import synth
    n = 202 * 1600
    jobs = {s: [(synth.pcm(980 + s, n), 1600)] for s in (0, 1, 3)}
    jobs[2] = [(synth.pcm(982, 100 * 1600), 1600), (synth.pcm(984, 102 * 1600), 1600)]
    sess = G.Sessions(ctx, model, 4, 1600, gs)
    seen = {}

    def on_tick(t):
        if t in (2, 202):
            seen[t] = G.debug_counters()
    try:
        got = run_jobs(torch, G, sess, jobs, on_tick=on_tick)
    finally:
        sess.close()
    assert sorted(seen) == [2, 202] and seen[2] == seen[202], seen
    assert seen[2][0] > 0
    check_jobs(torch, G, ctx, model, gs, jobs, got)


def test_reserve_covers_every_mode(torch, G, xs_config, gs):
    """One set created with the model in its default mode, then the model
    switched through every GEMM mode with the context's latency mode off and
    on: the workspaces grown at create cover all of them, so the allocation
    and release counts stand still from the first mode's second tick to the
    last mode's last one, and every mode's rows are its one-shot rows.  The
    references are computed afterwards: a one-shot call before would size the
    context's workspaces itself."""
    from catears_amd import synth
    c = G.Context(0)
    m = G.Model(c, xs_config)
    waves = [synth.pcm(1000 + s, 4 * 1600) for s in range(2)]
    pcm = [dev(torch, w) for w in waves]
    configs = [(lat, mode) for lat in (False, True) for mode in ("fp32", "bf16x6", "bf16x6p", "f16x3", "bf16")]
    got, seen = {}, []
    sess = G.Sessions(c, m, 2, 1600, gs)
    try:
        for lat, mode in configs:
            c.set_latency(lat)
            m.set_gemm(mode)
            pieces = [[], []]
            for t in range(4):
                order = [t % 2, 1 - t % 2]
                out, rows = sess.push(order, torch.cat([pcm[s][1600 * t:1600 * (t + 1)] for s in order]), [1600, 1600],
                                      eos=[t == 3] * 2)
                host = out.cpu().numpy()
                pieces[order[0]].append(host[:rows[0]])
                pieces[order[1]].append(host[rows[0]:])
                seen.append(G.debug_counters())
            got[lat, mode] = [np.concatenate(p) for p in pieces]
            for s in range(2):
                sess.reset(s)
    finally:
        sess.close()
    assert len(seen) == 4 * len(configs) and seen[1] == seen[-1], (seen[1], seen[-1])
    assert seen[1][0] > 0
    for lat, mode in configs:
        c.set_latency(lat)
        m.set_gemm(mode)
        for s in range(2):
            assert same(got[lat, mode][s], one_shot(torch, G, c, m, waves[s], gs)), (lat, mode, s)


def test_reserve_covers_static_int8_latency_row_counts(torch, G, ctx, xs_config, gs):
    """A static int8 model on a latency-mode context: the split-K pair's slice
    rule, and with it the partials a push needs, depends on the packed row
    count.  Pushes that pack 21, 70, 81 and 40 rows allocate nothing after
    the first, and take the split-K pair."""
    from catears_amd import synth
    # calibrated on the module's context, so that nothing but the set's create
    # sizes the workspaces of the context the pushes run on
    cal = G.Model(ctx, xs_config)
    cal_waves = [synth.pcm(1010 + i, 16000) for i in range(2)]
    plan = G.Plan(ctx, [len(w) for w in cal_waves], cal)
    ranges = cal.calibrate(ctx, plan, G.fbank(ctx, plan, dev(torch, np.concatenate(cal_waves))))
    c = G.Context(0)
    c.set_latency(True)
    m = G.Model(c, xs_config).quantize_static(c, ranges)
    counts = [2000, 8000, 9760, 1600]  # 11, 50, 61 and 10 frames: 1, 50, 61 and 20 rows
    assert G.Sessions.packed_rows(L, R, 0, counts, 3, False) == [21, 70, 81, 40]
    wave = synth.pcm(1012, sum(counts))
    sess = G.Sessions(c, m, 1, max(counts), gs)
    seen = []
    lat0 = G.debug_i8_latency_launches()
    try:
        pcm, at, pieces = dev(torch, wave), 0, []
        for i, n in enumerate(counts):
            out, _ = sess.push([0], pcm[at:at + n], [n], eos=[i == 3])
            pieces.append(out.cpu().numpy())
            seen.append(G.debug_counters())
            at += n
    finally:
        sess.close()
    assert seen[0] == seen[-1], seen
    assert G.debug_i8_latency_launches() > lat0
    assert same(np.concatenate(pieces), one_shot(torch, G, c, m, wave, gs))


# ------------------------------------------------------------- 10. capacity --

def test_capacity_too_small_changes_nothing(torch, G, ctx, model, gs):
    from catears_amd import synth
    wave = synth.pcm(990, 8000)
    ref = one_shot(torch, G, ctx, model, wave, gs)
    assert ref.shape[0] == 48
    sess = G.Sessions(ctx, model, 1, 8000, gs)
    try:
        pcm = dev(torch, wave)
        out = torch.zeros((48, 512), dtype=torch.float32, device="cuda")
        p32 = ctypes.POINTER(ctypes.c_int32)
        slot, cnt, flag, rows = (np.array([v], np.int32) for v in (0, 8000, G.SESSION_EOS, -1))
        rc = G.lib().ce_gpu_sessions_push(sess.h, 1, slot.ctypes.data_as(p32), cnt.ctypes.data_as(p32),
                                          flag.ctypes.data_as(p32), ctypes.c_void_p(pcm.data_ptr()),
                                          ctypes.c_void_p(out.data_ptr()), 47, rows.ctypes.data_as(p32))
        assert rc == -2 and rows[0] == 48
        assert not out.cpu().numpy().any()
        got, rows = sess.push([0], pcm, [8000], eos=[True], out=out)
        assert list(rows) == [48] and same(got.cpu().numpy(), ref)
    finally:
        sess.close()


# ---------------------------------------------------- 11. unsupported model --

def test_quantised_model_is_not_supported(torch, G, xs_config, gs):
    c = G.Context(0)
    m = G.Model(c, xs_config).quantize(c)
    with pytest.raises(G.CatearsError) as e:
        G.Sessions(c, m, 1, 1600, gs)
    assert e.value.code == -6
