"""Reusable plans, the parts that need no device: the argument checks of
gpu.Plan.reusable / Plan.assign, and ce_gpu_plan_capacity -- the worst-case
frame, segment and packed-row counts ce_gpu_plan_create_reusable reserves for
(the derivation is in catears_amd/csrc/plans.cc).  The bound is checked
against tests/planref.py's restatement of ce_gpu_plan_create's packing rule:
no assignment within a capacity may exceed it, and the assignments the
derivation names must reach it."""
import numpy as np
import pytest

import planref


@pytest.fixture(scope="module")
def G():
    from catears_amd import gpu
    gpu.lib()
    return gpu


def test_reusable_refuses_a_bad_capacity_before_any_device_call(G):
    for args in ((0, 1000), (-1, 1000), (2 ** 31, 1000), (4, 0), (4, -5), (4, 2 ** 63)):
        with pytest.raises(ValueError):
            G.Plan.reusable(None, *args)  # ctx is never touched
    with pytest.raises(ValueError):
        G.Plan.reusable(None, 4, 1000, max_rows=2 ** 31)


def test_assign_checks_its_lengths_before_any_device_call(G):
    plan = G.Plan.__new__(G.Plan)
    plan.h, plan.is_reusable, plan.max_utts, plan.max_total_samples = None, True, 3, 1000
    for bad in ([1, 2, 3, 4], [-1], [400, -400, 400], [600, 401], [1001], [[1, 2]], [1.5, 2.0], 7):
        with pytest.raises(ValueError):
            plan.assign(bad)
    fixed = G.Plan.__new__(G.Plan)
    fixed.h, fixed.is_reusable = None, False
    with pytest.raises(ValueError, match="immutable"):
        fixed.assign([400])
    # what passes the checks arrives as a contiguous int64 vector
    ns = G._plan_lengths(np.array([400, 0, 600], np.int32), 3, 1000)
    assert ns.dtype == np.int64 and ns.tolist() == [400, 0, 600] and ns.flags.c_contiguous
    assert G._plan_lengths([], 3, 1000).shape == (0,)


def test_plan_capacity_argument_errors(G):
    for args in ((0, 1000, 64, 2, 2), (4, 0, 64, 2, 2), (4, 1000, 4, 2, 2), (4, 1000, 64, -1, 2)):
        with pytest.raises(G.CatearsError) as e:
            G.plan_capacity(args[0], args[1], args[3], args[4], max_rows=args[2])
        assert e.value.code == -2
    # max_rows <= 0 selects 4096, as in ce_gpu_plan_create
    assert G.plan_capacity(4, 10 ** 6, 3, 2, max_rows=0) == G.plan_capacity(4, 10 ** 6, 3, 2, max_rows=4096)


def counts(lengths, left, right, max_rows):
    segs, _ = planref.pack(lengths, left, right, max_rows)
    return sum(planref.frames(n) for n in lengths), len(segs), sum(n + left + right for _, _, n, _ in segs)


@pytest.mark.parametrize("left,right,max_rows", [(5, 3, 9), (5, 3, 64), (0, 0, 1), (13, 9, 4096), (2, 7, 10)])
def test_no_assignment_within_a_capacity_exceeds_the_bound(G, left, right, max_rows):
    rng = np.random.default_rng(left * 1000 + max_rows)
    room = max_rows - left - right
    for trial in range(300):
        max_utts = int(rng.integers(1, 9))
        cap = int(rng.integers(1, 160 * 6 * room + 3000))
        bf, bs, bp = G.plan_capacity(max_utts, cap, left, right, max_rows=max_rows)
        assert bf == planref.frames(cap)
        # lengths that use the capacity to the sample: a random split of it
        n = int(rng.integers(1, max_utts + 1))
        cuts = np.sort(rng.integers(0, cap + 1, size=n - 1))
        lengths = np.diff(np.concatenate([[0], cuts, [cap]])).tolist()
        if trial % 3 == 0:  # many utterances of one frame each: the most segments per frame
            lengths = [400] * min(max_utts, cap // 400) or [cap]
        f, s, p = counts(lengths, left, right, max_rows)
        assert f <= bf and s <= bs and p <= bp, (max_utts, cap, lengths, (f, s, p), (bf, bs, bp))


def test_the_bound_is_reached(G):
    left, right, max_rows = 5, 3, 64
    room = max_rows - left - right
    # one utterance holds every sample: the most frames; frames = 3 * room + 1
    # split into 4 segments = frames / room + 1
    cap = planref.samples(3 * room + 1, extra=159)
    assert counts([cap], left, right, max_rows) == G.plan_capacity(1, cap, left, right, max_rows=max_rows)
    # as many one-frame utterances as the samples pay for: a segment each
    bf, bs, bp = G.plan_capacity(6, 2400, left, right, max_rows=max_rows)
    f, s, p = counts([400] * 6, left, right, max_rows)
    assert (s, p) == (6, 6 * (1 + left + right)) and s <= bs and p <= bp
    assert bs - s <= bf // room + 1  # the slack is the ceiling term alone
