"""Reusable plans on the device: ce_gpu_plan_create_reusable /
ce_gpu_plan_assign against ce_gpu_plan_create.

After an assign the plan must be the plan ce_gpu_plan_create builds for the
same lengths: every word of the six device tables (ce_gpu_debug_plan_tables),
ce_gpu_plan_info and the frame offsets.  Nearly every test here is that
comparison -- no PCM, no nnet, milliseconds a case -- with tests/planref.py's
numpy restatement as a third party.  The rest shows that the assignments are
ordered on the stream without a synchronize, that every entry taking a plan
gives the same bits on an assigned one, that nothing is allocated once the
plan exists, and that the capacity-sized tables leak no stale word.

The model is a small synthetic TDNN with its own context (L = 5, R = 3);
fbank's block size and the ring depth are read back from the sources."""
import ctypes

import numpy as np
import pytest

import devfill
import planref

pytestmark = pytest.mark.gpu

L, R = 5, 3
SPLICES = [[-2, -1, 0, 1], [-3, 0, 2]]
PDFS = 48
FPB = planref.frames_per_block()
RING = planref.ring_depth()
MAX_ROWS = (L + R + 1, 64, 4096)
S = planref.samples
EINVAL = -2


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def G(torch):
    # behind torch: the library binds to the HIP runtime torch has loaded
    from catears_amd import gpu
    gpu.lib()
    return gpu


@pytest.fixture(scope="module")
def ctx(torch, G):
    return G.Context(0)


def new_model(G, ctx):
    from catears_amd import formats, synth
    layers, left, right, prior = synth.tdnn_layers(64, PDFS, splices=SPLICES, seed=31)
    assert (left, right) == (L, R)
    return G.Model(ctx, image=formats.nnet_bytes(layers, left, right), prior=prior)


@pytest.fixture(scope="module")
def model(G, ctx):
    return new_model(G, ctx)


def info(plan):
    return (plan.n_utt, plan.total_samples, plan.total_frames, plan.n_chunks, plan.max_chunk_rows)


def assert_same_plan(G, got, want, ref=None):
    """got (assigned) and want (ce_gpu_plan_create) are the same plan: tables,
    plan_info, frame offsets; and both are planref's, when given."""
    a, b = G.debug_plan_tables(got), G.debug_plan_tables(want)
    for name, dtype in G.PLAN_TABLES:
        assert a[name].dtype == b[name].dtype == dtype
        assert a[name].shape == b[name].shape, (name, a[name].shape, b[name].shape)
        diff = np.flatnonzero(a[name] != b[name])
        assert diff.size == 0, (name, int(diff[0]), a[name][diff[:4]], b[name][diff[:4]])
    assert info(got) == info(want)
    assert np.array_equal(got.frame_offsets, want.frame_offsets)
    if ref is not None:
        tab, inf = ref
        for name, _ in G.PLAN_TABLES:
            assert np.array_equal(b[name], tab[name]), name
        assert info(want) == inf


def check(G, ctx, plan, lengths, model=None, max_rows=4096):
    plan.assign(lengths)
    want = G.Plan(ctx, lengths, model, max_rows)
    ref = planref.tables(lengths, L if model else None, R if model else None, max_rows)
    assert_same_plan(G, plan, want, ref)
    want.close()


# ------------------------------------------------------ 1. the seam lists --

def seam_cases(max_rows):
    room = max_rows - L - R
    half = room // 2 + 1
    cases = {
        "empty": [], "s0": [0], "s399": [399], "s400": [400], "s559": [559], "s560": [560],
        "zero-first": [0, S(5), S(7)], "zero-middle": [S(5), 399, S(7)], "zero-last": [S(5), S(7), 123],
        "zero-pairs": [S(5), 0, 399, S(7), 1, 0, S(3)], "zero-only": [0, 399, 17],
        "fpb-1": [S(FPB - 1)] if FPB > 1 else [0], "fpb": [S(1), S(FPB - 1)] if FPB > 1 else [S(1)],
        "fpb+1": [S(2), S(FPB - 1, 159)], "2fpb": [S(FPB), S(FPB)],
        "room": [S(room)], "room+1": [S(room + 1)],
        "fresh-chunk": [S(half), S(half, 80), S(1)],
        "three-chunks": [S(1), S(2 * room + 1)],
        "T1": [S(1)], "T<R": [S(R - 1)], "T<L": [S(L - 1)], "short-mix": [S(1), S(R - 1), S(L - 1), S(1, 159)],
    }
    return cases


CASE_NAMES = sorted(seam_cases(64))


@pytest.fixture(scope="module")
def seam_plans(G, ctx, model):
    """One reusable plan per max_rows for all the seam lists: each case is one
    more assignment of the same plan."""
    plans = {}
    for mr in MAX_ROWS:
        cap = max(sum(v) for v in seam_cases(mr).values())
        plans[mr] = G.Plan.reusable(ctx, 8, cap, model, mr)
    yield plans
    for p in plans.values():
        p.close()


@pytest.mark.parametrize("max_rows", MAX_ROWS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_seam_lists(G, ctx, model, seam_plans, name, max_rows):
    lengths = seam_cases(max_rows)[name]
    check(G, ctx, seam_plans[max_rows], lengths, model, max_rows)
    # the lists do what their names say
    if name == "fresh-chunk":  # (with room for one frame every utterance fills its chunk)
        assert seam_plans[max_rows].n_chunks == (3 if max_rows == L + R + 1 else 2)
    if name == "three-chunks":  # the one-frame utterance's chunk, then three
        assert seam_plans[max_rows].n_chunks == 4


@pytest.mark.parametrize("name", CASE_NAMES)
def test_seam_lists_without_a_model(G, ctx, name):
    """The drop-in's kind of plan: the three fbank tables alone."""
    lengths = seam_cases(64)[name]
    plan = G.Plan.reusable(ctx, 8, max(sum(lengths), 1))  # a capacity met to the sample
    check(G, ctx, plan, lengths)
    assert G.debug_plan_tables(plan)["row_src"].size == 0
    plan.close()


def test_a_fresh_reusable_plan_is_the_empty_plan(G, ctx, model):
    plan = G.Plan.reusable(ctx, 4, 10000, model, 64)
    want = G.Plan(ctx, [], model, 64)
    assert_same_plan(G, plan, want, planref.tables([], L, R, 64))
    plan.close()
    want.close()


# ------------------------------------------------- 2. row_edge saturation --

def test_row_edge_saturates(G, ctx, model):
    max_rows = 70000
    lengths = [S(max_rows - L - R)]
    plan = G.Plan.reusable(ctx, 1, lengths[0], model, max_rows)
    check(G, ctx, plan, lengths, model, max_rows)
    edge = G.debug_plan_tables(plan)["row_edge"]
    assert edge.size == max_rows and plan.n_chunks == 1
    # rows further than 0xffff from an end carry the saturated distance
    assert edge[0] == 0xffff << 16 and edge[-1] == 0xffff and edge[0xffff + 100] & 0xffff == 0xffff
    assert edge[max_rows - 1 - 0xffff] >> 16 == 0xffff and edge[max_rows - 0xffff] >> 16 == 0xfffe
    plan.close()


# ------------------------------------------- 3. one plan, many assignments --

def test_one_plan_many_assignments(G, ctx, model):
    large_a = [S(150, 7), 0, S(90), S(1), S(64 - L - R), S(200, 100)]
    large_b = [S(31), S(260), 399, S(120, 3)]
    large_c = [S(56), S(57), S(55), S(1), S(1), S(2), S(300)]
    plan = G.Plan.reusable(ctx, 8, max(sum(large_a), sum(large_b), sum(large_c)), model, 64)
    for lengths in (large_a, [S(2)], large_b, [], large_c, [400, 0], large_a):
        check(G, ctx, plan, lengths, model, 64)
    plan.close()


# ------------------------------------------- 4. capacity and error rules --

def raw_assign(G, plan, lengths):
    ns = np.ascontiguousarray(lengths, np.int64)
    return G.lib().ce_gpu_plan_assign(plan.h, ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(ns))


def test_assign_errors_leave_the_previous_assignment(G, ctx, model):
    """The C-ABI's own checks (gpu.Plan.assign would refuse the same lists
    before the call, tests/test_plan_reusable_cpu.py)."""
    held = [S(40), 0, S(75, 33)]
    plan = G.Plan.reusable(ctx, 3, sum(held), model, 64)
    plan.assign(held)
    want = G.Plan(ctx, held, model, 64)
    for bad, limit in (([S(1), S(1), S(1), S(1)], "max_utts is 3"), ([S(40), 1, S(75, 33)], f"max_total_samples ({sum(held)})"),
                       ([sum(held) + 1], "max_total_samples"), ([S(3), -1], "negative"), ([-(2 ** 62), S(3)], "negative")):
        assert raw_assign(G, plan, bad) == EINVAL, bad
        assert limit in G.lib().ce_gpu_last_error().decode(), (bad, G.lib().ce_gpu_last_error())
        plan._refresh()
        assert_same_plan(G, plan, want)
    assert G.lib().ce_gpu_plan_assign(plan.h, None, -1) == EINVAL
    assert G.lib().ce_gpu_plan_assign(plan.h, None, 2) == EINVAL
    plan._refresh()
    assert_same_plan(G, plan, want)
    # and the plan still takes an assignment at its capacity
    check(G, ctx, plan, [sum(held)], model, 64)
    assert raw_assign(G, want, held) == EINVAL  # a plan of ce_gpu_plan_create
    assert "immutable" in G.lib().ce_gpu_last_error().decode()
    assert info(want) == planref.tables(held, L, R, 64)[1]
    plan.close()
    want.close()


def test_create_reusable_argument_errors(G, ctx, model):
    def create(m, max_utts, max_total, max_rows):
        h = ctypes.c_void_p()
        rc = G.lib().ce_gpu_plan_create_reusable(ctx.h, m.h if m else None, max_utts, max_total, max_rows, ctypes.byref(h))
        if rc == 0:
            G.lib().ce_gpu_plan_destroy(h)
        else:
            assert not h.value
        return rc

    before = G.debug_counters()
    assert create(model, 0, 1000, 64) == EINVAL and "max_utts" in G.lib().ce_gpu_last_error().decode()
    assert create(model, -3, 1000, 64) == EINVAL
    assert create(model, 4, 0, 64) == EINVAL and "max_total_samples" in G.lib().ce_gpu_last_error().decode()
    assert create(model, 4, -1, 64) == EINVAL
    assert create(model, 4, 1000, L + R) == EINVAL and "max_rows" in G.lib().ce_gpu_last_error().decode()
    assert create(model, 4, 1000, 1) == EINVAL
    assert G.debug_counters() == before  # refused before anything was reserved
    assert create(model, 4, 1000, L + R + 1) == 0
    assert create(model, 4, 1000, 0) == 0 and create(model, 4, 1000, -1) == 0  # 4096, as ce_gpu_plan_create
    assert create(None, 4, 1000, 1) == 0  # no model: no context to cover
    h = ctypes.c_void_p()
    assert G.lib().ce_gpu_plan_create_reusable(None, None, 4, 1000, 64, ctypes.byref(h)) == EINVAL
    assert G.lib().ce_gpu_plan_create_reusable(ctx.h, None, 4, 1000, 64, None) == EINVAL


# --------------------------------------------------------------- scoring --

ORDER_LISTS = ([S(120, 11), 0, S(1), S(90)], [S(2)], [S(64 - L - R), S(57), 399, S(130, 159)])
SENTINEL = -7.25


def pcm_of(torch, lengths, seed):
    rng = np.random.default_rng(seed)
    x = np.rint(rng.normal(0.0, 3000.0, size=max(sum(lengths), 1))).clip(-32768, 32767).astype(np.float32)
    return torch.from_numpy(x).cuda()


@pytest.fixture(scope="module")
def gstats(torch):
    from catears_amd import synth
    return torch.from_numpy(synth.cmvn_stats_synthetic()).cuda()


def same_bits(torch, a, b):
    return devfill.same_bits(torch, a, b)


@pytest.mark.parametrize("gemm", ["default", "fp32"])
def test_assignments_are_ordered_without_a_synchronize(torch, G, ctx, gstats, gemm):
    m = new_model(G, ctx)
    if gemm != "default":
        m.set_gemm(gemm)
    pcms = [pcm_of(torch, ls, 40 + i) for i, ls in enumerate(ORDER_LISTS)]
    wants = []
    for ls, pcm in zip(ORDER_LISTS, pcms):
        fixed = G.Plan(ctx, ls, m, 64)
        wants.append(G.score(ctx, m, fixed, pcm, gstats))
        torch.cuda.synchronize()
        fixed.close()
    rows = max(w.shape[0] for w in wants) + 9
    pairs = 2 * RING + 1
    outs = [torch.full((rows, PDFS), SENTINEL, dtype=torch.float32, device="cuda") for _ in range(pairs)]
    ws = torch.empty((2 * rows * 40 + 1,), dtype=torch.float32, device="cuda")
    plan = G.Plan.reusable(ctx, 8, max(sum(ls) for ls in ORDER_LISTS), m, 64)
    torch.cuda.synchronize()
    for i in range(pairs):  # nothing below waits for the device
        k = i % len(ORDER_LISTS)
        plan.assign(ORDER_LISTS[k])
        G.score(ctx, m, plan, pcms[k], gstats, ws=ws, out=outs[i])
    torch.cuda.synchronize()
    for i in range(pairs):
        want = wants[i % len(ORDER_LISTS)]
        n = want.shape[0]
        assert same_bits(torch, outs[i][:n], want), i
        assert bool((outs[i][n:] == SENTINEL).all()), i
    plan.close()


def test_entry_points_take_an_assigned_plan(torch, G, ctx, model, gstats):
    lengths = ORDER_LISTS[2]
    pcm = pcm_of(torch, lengths, 77)
    pcm16 = pcm.to(torch.int16)
    plan = G.Plan.reusable(ctx, 8, 2 * sum(lengths), model, 64)
    plan.assign([S(200), S(3)])
    plan.assign(lengths)
    fixed = G.Plan(ctx, lengths, model, 64)
    got, want = [], []
    for p, acc in ((plan, got), (fixed, want)):
        f16 = G.fbank(ctx, p, pcm16)
        f32 = G.fbank(ctx, p, pcm)
        norm = G.cmvn(ctx, p, gstats, f32)
        acc += [f16, f32, norm, G.am_forward(ctx, model, p, norm), G.score(ctx, model, p, pcm16, gstats)]
    torch.cuda.synchronize()
    for name, a, b in zip(("fbank_s16", "fbank", "cmvn", "am_forward", "score_s16"), got, want):
        assert a.shape[0] == plan.total_frames and same_bits(torch, a, b), name
    # calibration reads the row maps through the same plan
    assert np.array_equal(model.calibrate(ctx, plan, got[2]), model.calibrate(ctx, fixed, want[2]))
    plan.close()
    fixed.close()


def test_assign_and_score_allocate_nothing(torch, G, ctx, model, gstats):
    pcms = [pcm_of(torch, ls, 60 + i) for i, ls in enumerate(ORDER_LISTS)]
    plan = G.Plan.reusable(ctx, 8, max(sum(ls) for ls in ORDER_LISTS), model, 64)
    rows = max(sum(planref.frames(n) for n in ls) for ls in ORDER_LISTS)
    ws = torch.empty((2 * rows * 40 + 1,), dtype=torch.float32, device="cuda")
    out = torch.empty((rows, PDFS), dtype=torch.float32, device="cuda")
    largest = max(range(len(ORDER_LISTS)), key=lambda k: sum(ORDER_LISTS[k]))
    plan.assign(ORDER_LISTS[largest])
    G.score(ctx, model, plan, pcms[largest], gstats, ws=ws, out=out)  # the first round sizes the workspaces
    before = G.debug_counters()
    for i in range(50):
        k = i % len(ORDER_LISTS)
        plan.assign(ORDER_LISTS[k])
        G.score(ctx, model, plan, pcms[k], gstats, ws=ws, out=out)
    assert G.debug_counters() == before
    torch.cuda.synchronize()
    plan.close()


@pytest.mark.parametrize("word", sorted(devfill.WORDS))
def test_no_stale_table_word_is_read(torch, G, ctx, model, gstats, word):
    """The tables are sized for the capacity: after a large assignment a small
    one leaves the large one's words (and, behind them, the fill) in place.
    None of them may reach a launch."""
    large, small = ORDER_LISTS[2], ORDER_LISTS[1]
    pcm_l, pcm_s = pcm_of(torch, large, 91), pcm_of(torch, small, 92)
    G.debug_fill_allocs(False)
    try:
        with devfill.fresh_allocations(G, devfill.WORDS[word]):
            plan = G.Plan.reusable(ctx, 8, 4 * sum(large), model, 64)
        plan.assign(large)
        got_l = G.score(ctx, model, plan, pcm_l, gstats)
        plan.assign(small)
        got_s = G.score(ctx, model, plan, pcm_s, gstats)
        torch.cuda.synchronize()
    finally:
        G.debug_fill_allocs(False)
    for ls, pcm, got in ((large, pcm_l, got_l), (small, pcm_s, got_s)):
        fixed = G.Plan(ctx, ls, model, 64)
        want = G.score(ctx, model, fixed, pcm, gstats)
        torch.cuda.synchronize()
        assert same_bits(torch, got, want), (word, ls)
        fixed.close()
    check(G, ctx, plan, small, model, 64)
    plan.close()
