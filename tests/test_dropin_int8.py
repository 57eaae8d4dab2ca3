"""Static int8 from a configuration file: the key gpu_int8_ranges = <path>
(a VEC0 of min0 max0 min1 max1 ..., one pair per Linear) in the drop-in
AcousticModel::Read (catears_amd/host/src/am.cc) and in
ce_gpu_model_load_config.  The rows of a static int8 model do not depend on
the batch, so the drop-in's streamed chunks must be, bit for bit, the rows
Model.quantize_static gives through Python on the whole padded utterance.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_dropin import DRIVER, _am_config, _load, _put, _run

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
def ctx(torch, G):
    return G.Context(0)


def dev(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def calibrated(torch, G, ctx, oracle, xs_config, tmp_path_factory):
    """TDNN-XS ranges from Model.calibrate on three utterances, as VEC0 files
    (a good one and one a value short), the features of a fourth utterance and
    their rows from Model.quantize_static through Python (the whole utterance
    padded as AcousticModel pads it, prior subtracted)."""
    from catears_amd import formats, synth
    d = tmp_path_factory.mktemp("int8_ranges")
    m = G.Model(ctx, xs_config)
    waves = [synth.pcm(60 + i, 16000 * 3) for i in range(3)]
    plan = G.Plan(ctx, [len(w) for w in waves], m)
    ranges = m.calibrate(ctx, plan, G.fbank(ctx, plan, dev(torch, np.concatenate(waves))))
    good, bad = d / "ranges.vec0", d / "ranges_short.vec0"
    good.write_bytes(formats.vec_bytes(ranges.reshape(-1)))
    bad.write_bytes(formats.vec_bytes(ranges.reshape(-1)[:-1]))
    feats = oracle.Fbank().compute(synth.pcm(5, 16000 * 3 + 123))
    am = formats.read_am(xs_config)
    block = np.concatenate([np.repeat(feats[:1], am["left"], 0), feats, np.repeat(feats[-1:], am["right"], 0)], 0)
    fp32 = G.nnet_propagate(ctx, m, dev(torch, block), subtract_prior=True).cpu().numpy()
    m.quantize_static(ctx, ranges)
    want = G.nnet_propagate(ctx, m, dev(torch, block), subtract_prior=True).cpu().numpy()
    assert want.shape == fp32.shape == (len(feats), am["num_pdfs"])
    return {"good": good, "bad": bad, "feats": feats, "want": want, "fp32": fp32, "block": block}


@pytest.mark.parametrize("chunk", [7, 50])
def test_am_config_key_gives_the_static_int8_rows(tmp_path, xs_config, calibrated, chunk):
    feats, want = calibrated["feats"], calibrated["want"]
    x = _put(tmp_path, "x.f32", feats)
    out8, out32 = tmp_path / "am8.bin", tmp_path / "am32.bin"
    conf8 = _am_config(tmp_path, xs_config, chunk, extra=f"gpu_int8_ranges = {calibrated['good']}\n")
    _run("am", conf8, x, len(feats), out8)
    got = _load(out8)
    assert got.shape == want.shape
    diff = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert diff.size == 0, f"{diff.size} frames differ, first {diff[0]}"
    # the same config without the key scores fp32: other rows, so the key
    # cannot have been ignored
    _run("am", _am_config(tmp_path, xs_config, chunk), x, len(feats), out32)
    plain = _load(out32)
    assert plain.shape == got.shape and not np.array_equal(bits(plain), bits(got))
    assert np.max(np.abs(plain - calibrated["fp32"])) <= 1e-4


def test_am_read_refuses_a_short_ranges_file(tmp_path, xs_config, calibrated):
    conf = _am_config(tmp_path, xs_config, 50, extra=f"gpu_int8_ranges = {calibrated['bad']}\n")
    x = _put(tmp_path, "x.f32", calibrated["feats"])
    r = subprocess.run([DRIVER, "am", str(conf), str(x), str(len(calibrated["feats"])), str(tmp_path / "o.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert os.path.basename(str(calibrated["bad"])) in r.stdout + r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "o.bin").exists()


def test_load_config_key(torch, G, ctx, tmp_path, xs_config, calibrated):
    """The same good and bad files through ce_gpu_model_load_config."""
    block = dev(torch, calibrated["block"])
    good = _am_config(tmp_path, xs_config, 50, extra=f"gpu_int8_ranges = {calibrated['good']}\n")
    m = G.Model(ctx, str(good))
    assert m.quant_params()[0].size == m.num_linear
    got = G.nnet_propagate(ctx, m, block, subtract_prior=True).cpu().numpy()
    assert np.array_equal(bits(got), bits(calibrated["want"]))
    bad = _am_config(tmp_path, xs_config, 7, extra=f"gpu_int8_ranges = {calibrated['bad']}\n")
    h = ctypes.c_void_p(1)
    rc = G.lib().ce_gpu_model_load_config(ctx.h, str(bad).encode(), ctypes.byref(h))
    assert rc == -2 and not h.value
    msg = G.lib().ce_gpu_last_error().decode()
    assert os.path.basename(str(calibrated["bad"])) in msg and "model_quantize_static" in msg, msg
