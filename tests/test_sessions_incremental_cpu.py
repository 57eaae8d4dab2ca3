"""Incremental sessions without a device: the scheme (tests/incref.py) equals
the one-shot evaluation bit for bit, Sessions.packed_rows equals a
brute-force count, and the ABI lists the two new entry points."""
import numpy as np
import pytest

import incref

ASYM = [[-2, -1, 0, 1, 2], [-4, 0, 1], [0], [-1, 0, 5]]  # L = 7, R = 8, H = 6, a zero-span layer in mid-chain


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def models(xs_config):
    from catears_amd import formats, synth
    layers, left, right, prior = synth.tdnn_layers(128, 96, splices=ASYM)
    asym = {"layers": layers, "left": left, "right": right, "log_prior": np.log(prior).astype(np.float32)}
    assert (left, right, incref.spans(layers)) == (7, 8, [4, 5, 0, 6, 0])
    xs = formats.read_am(xs_config)
    assert (xs["left"], xs["right"]) == (10, 10) and incref.lead_rows(xs["layers"]) == 6
    return {"xs": xs, "asym": asym}


def chunkings(frames, seed):
    """(counts, eos_at): one frame per push; random sizes (zero among them)
    with the EOS on an empty last push; everything and the EOS in one push."""
    rng = np.random.default_rng(seed)
    ragged, left = [], frames
    while left:
        c = min(left, int(rng.choice([0, 1, 1, 2, 3, 5, 9, 17])))
        ragged.append(c)
        left -= c
    return [([1] * frames, frames - 1), (ragged + [0], len(ragged)), ([frames], 0)]


@pytest.mark.parametrize("net", ["xs", "asym"])
def test_scheme_equals_one_shot(oracle, models, net):
    model = models[net]
    R, H = model["right"], incref.lead_rows(model["layers"])
    for frames in (1, 2, R, R + 1, 40):
        feats = np.random.default_rng(100 + frames).normal(9.0, 3.0, size=(frames, 40)).astype(np.float32)
        want = oracle.am_whole(model, feats)
        assert want.shape[0] == frames and np.isfinite(want).all()
        for counts, eos_at in chunkings(frames, 7 * frames):
            got, packed = incref.stream(oracle, model, feats, counts, eos_at)
            assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (net, frames, counts)
            from catears_amd import gpu
            samples = [0 if c == 0 else 160 * c for c in counts]
            samples[next(i for i, c in enumerate(counts) if c)] += 240  # the first frame takes 400 samples
            assert sum(gpu.Sessions.packed_rows(model["left"], R, H, samples, eos_at, True)) == packed
    # blocks cut at the chunk size: 40 frames in one push through chunks of 16 rows
    got, packed = incref.stream(oracle, model, feats, [40], 0, max_rows=16)
    assert np.array_equal(bits(got), bits(want))
    n = 40 + model["left"] + R
    assert packed == n + -(-n // (16 - H)) * H


def test_before_eos_rows_are_held_back(oracle, models):
    model = models["asym"]
    feats = np.random.default_rng(5).normal(9.0, 3.0, size=(30, 40)).astype(np.float32)
    want = oracle.am_whole(model, feats)
    s = incref.Stream(oracle, model)
    a = s.push(feats[:3])
    b = s.push(feats[3:21])
    c = s.push(feats[21:], eos=True)
    assert (len(a), len(b), len(c)) == (0, 21 - 8, 30 - 13)
    assert np.array_equal(bits(np.concatenate([a, b, c])), bits(want))


def brute_force(L, R, H, sample_counts, eos_at, incremental, max_rows=4096):
    """Packed rows per push, counted one row at a time."""
    ctx = H if incremental else L + R
    samples = frames = fed = 0   # fed: positions (incremental) or rows (not) so far
    out = []
    for i, c in enumerate(sample_counts):
        samples += c
        frames = 0 if samples < 400 else 1 + (samples - 400) // 160
        eos = eos_at is not None and i == eos_at
        if incremental:
            total = 0 if frames == 0 else L + frames + (R if eos else 0)
        else:
            total = frames if eos else max(0, frames - R)
        packed = in_block = 0
        for _ in range(total - fed):
            if in_block == 0 or in_block == max_rows:
                packed += ctx
                in_block = ctx
            packed += 1
            in_block += 1
        fed = total
        out.append(packed)
    return out


@pytest.mark.parametrize("incremental", [False, True])
def test_packed_rows_equals_brute_force(incremental):
    from catears_amd import gpu
    rng = np.random.default_rng(11)
    cases = [([400], 0), ([399, 1], None), ([0, 0], 1), ([1600] * 30, 29), ([160] * 50, None), ([48000], 0),
             ([660000], 0), ([960000, 960000], 1), ([700000, 0], 1)]
    for _ in range(20):
        n = int(rng.integers(1, 12))
        counts = [int(v) for v in rng.choice([0, 1, 159, 160, 400, 1600, 4000, 70000], size=n)]
        cases.append((counts, None if rng.integers(2) else n - 1))
    for L, R, H in ((10, 10, 6), (7, 8, 6), (0, 0, 0), (3, 0, 3)):
        for counts, eos_at in cases:
            got = gpu.Sessions.packed_rows(L, R, H, counts, eos_at, incremental)
            assert got == brute_force(L, R, H, counts, eos_at, incremental), (L, R, H, counts, eos_at)
    # the issue's table: 100 / 30 / 10 ms ticks of a running TDNN-S stream
    for ms, inc, full in ((100, 16, 30), (30, 9, 23), (10, 7, 21)):
        counts = [4000] + [16 * ms] * 3
        assert gpu.Sessions.packed_rows(10, 10, 6, counts, None, True)[-1] == inc
        assert gpu.Sessions.packed_rows(10, 10, 6, counts, None, False)[-1] == full


def test_abi_lists_the_incremental_entries():
    from catears_amd import gpu
    lib = gpu.lib()
    for name in ("ce_gpu_sessions_create_ex", "ce_gpu_sessions_stats"):
        assert name in gpu.ABI and hasattr(lib, name)
    assert gpu.SESSIONS_INCREMENTAL == 1
