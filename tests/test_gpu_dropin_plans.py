"""The drop-in classes on their lanes' reusable plans (tests/native/
pk_fbank_stream.cc): Fbank::Process and CMVN::CMVN rebind the lane's plan
(ce_gpu_plan_assign) where they used to create and destroy a plan per call.

The features keep their bits -- the bars of tests/test_dropin.py against the
oracle and the Kaldi dump, and the bits of one ce_gpu_fbank call over the
whole utterance on a plan of ce_gpu_plan_create -- and the library's
allocation counters (ce_gpu_debug_counters) stand still once a lane is warm:
a stream of 512-sample reads never moves them, a 100 000-sample piece moves
them by the one growth of the lane's plan, and so may a long CMVN."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(ROOT, "catears_amd", "lib", "pk_fbank_stream")
FEAT_TOL = 1e-5


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


def run(*args):
    assert os.path.exists(DRIVER), "pk_fbank_stream not built"
    r = subprocess.run([DRIVER] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args[0], r.returncode, r.stderr[-2000:])
    seen = {}
    for line in r.stdout.splitlines():
        label, allocs, frees = line.split()
        seen[label] = (int(allocs), int(frees))
    assert sorted(seen) == ["first", "last", "start"], r.stdout
    return seen


def load(path):
    raw = open(path, "rb").read()
    rows, cols = struct.unpack("<ii", raw[:8])
    return np.frombuffer(raw[8:], dtype=np.float32).reshape(rows, cols)


def put(tmp_path, name, arr):
    p = tmp_path / name
    np.ascontiguousarray(arr).tofile(p)
    return p


def moved(a, b):
    return (b[0] - a[0], b[1] - a[1])


@pytest.fixture(scope="module")
def one_growth(torch, G):
    """What one model-less reusable plan costs in allocations, and as many
    releases when it goes: the move of one growth."""
    ctx = G.Context(0)
    a = G.debug_counters()
    plan = G.Plan.reusable(ctx, 1, 1 << 20)
    b = G.debug_counters()
    plan.close()
    c = G.debug_counters()
    assert moved(a, b)[1] == 0 and moved(b, c) == (0, moved(a, b)[0])
    return (moved(a, b)[0], moved(a, b)[0])


def whole_utterance_bits(torch, G, wave, samples):
    ctx = G.Context(0)
    plan = G.Plan(ctx, [samples])
    feats = G.fbank(ctx, plan, torch.from_numpy(np.ascontiguousarray(wave[:samples])).cuda())
    torch.cuda.synchronize()
    return feats.cpu().numpy()


def test_a_stream_of_512_sample_reads_allocates_nothing(torch, G, tmp_path, oracle):
    from catears_amd import synth
    wave = synth.pcm(5, 200 * 512 + 300)
    out = tmp_path / "f.bin"
    seen = run("fbank", put(tmp_path, "pcm.f32", wave), 512, 200, out)
    assert seen["start"] == seen["first"] == seen["last"]
    got = load(out)
    want = oracle.Fbank().compute(wave[:200 * 512])
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= FEAT_TOL
    assert np.array_equal(got.view(np.uint32), whole_utterance_bits(torch, G, wave, 200 * 512).view(np.uint32))


@pytest.mark.parametrize("chunk", [777, 160, 100000])
def test_fbank_streaming_keeps_its_bits(torch, G, tmp_path, oracle, one_growth, chunk):
    wave = oracle.read_wav(os.path.join(GOLDEN, "en-us-hello.wav"))
    if chunk == 100000:  # one piece of exactly that many samples
        wave = np.concatenate([wave] * (100000 // len(wave) + 1))[:100000]
    out = tmp_path / "f.bin"
    seen = run("fbank", put(tmp_path, "pcm.f32", wave), chunk, 0, out)
    got = load(out)
    want = oracle.Fbank().compute(wave)
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= FEAT_TOL
    assert np.array_equal(got.view(np.uint32), whole_utterance_bits(torch, G, wave, len(wave)).view(np.uint32))
    # the reference's own bar (test/fbank_test.cc); the frames of the file's
    # first copy when it was repeated
    kaldi = np.loadtxt(os.path.join(GOLDEN, "fbankmat_en-us-hello.wav.txt"), dtype=np.float32).reshape(-1, 40)
    assert np.max(np.abs(got[:len(kaldi)] - kaldi)) <= 1e-4
    if chunk == 100000:
        # beyond the lane plan's first capacity: the one growth, nothing else
        assert moved(seen["start"], seen["last"]) == one_growth
    else:
        assert len(got) == len(kaldi)
        assert seen["start"] == seen["first"] == seen["last"]


def test_cmvn_twice_moves_the_counters_only_by_a_growth(tmp_path, oracle, global_stats, one_growth):
    from catears_amd import synth
    feats = oracle.Fbank().compute(synth.pcm(3, 400 + 160 * 699))
    assert len(feats) == 700
    out_a, out_b = tmp_path / "a.bin", tmp_path / "b.bin"
    seen = run("cmvn", put(tmp_path, "x.f32", feats), 47, 700, os.path.join(GOLDEN, "cmvn_stats.bin"), out_a, out_b)
    for rows, out in ((47, out_a), (700, out_b)):
        want = oracle.cmvn(global_stats, feats[:rows])
        assert np.array_equal(load(out).view(np.uint32), want.view(np.uint32)), rows
    assert seen["start"] == seen["first"]  # 47 frames fit the lane plan as it starts
    assert moved(seen["first"], seen["last"]) in ((0, 0), one_growth)
