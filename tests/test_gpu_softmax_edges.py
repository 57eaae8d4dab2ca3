"""LogSoftmax and Softmax at the edges of expf.

The reference's LogSoftmax is x - log(sum exp x) with no max shift
(oracle.c orc_log_softmax), so a logit of 89 overflows the sum and logits
below -104 underflow it.  The GPU has it in five places -- finalize_vec_kernel
(width 512), finalize_kernel's register form (510) and loop form (4100), the
row-op kernel (ce_gpu_rowwise) and latency mode's fused tail (512 on a latency
context) -- and every other test feeds them logits of a few units.

The logits are injected exactly in every GEMM mode: a one-Linear net whose
input rows are [r, 0, 0, ...], r = 0..8, whose weights are small integers in
row 0 and zero elsewhere and whose bias holds the integer logit pattern:
logit[r, c] = bias[c] + r * w[0, c], netgen's exact-integer argument
(check_exact_budget is asserted).  Nine rows: kernels of four rows per block
end on a ragged block.

Patterns:
  dominant   one logit at 85, the rest <= 0: finite; within LOGLIK_TOL of the
             float64 x - logsumexp(x)
  overflow   two logits >= 89: every output -inf, as the oracle's
  underflow  every logit <= -104: the sum is 0, every output +inf, as the oracle's
  denormal   every logit in [-100, -90]: the reference's sum is a denormal of
             few bits, so its own error against float64 is large; the GPU's
             may be max(LOGLIK_TOL, 2 x the oracle's) -- the form of
             test_split_gemms_are_fp32_accurate, the 2 for another, equally
             valid expf
"""
import functools

import numpy as np
import pytest

import netgen
from test_gpu_parity import LOGLIK_TOL, dev
from test_int8_static import FLT_MIN

pytestmark = pytest.mark.gpu

ROWS, IN_DIM = 9, 40
WIDTHS = {512: "vector", 510: "scalar", 4100: "loop"}   # netgen.finalize_path
PATTERNS = ("dominant", "overflow", "underflow", "denormal")
# Softmax outputs are at most 1: expf and the sum are good to a few ulp
SOFTMAX_TOL = 1e-6


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
    c = {"plain": G.Context(0), "latency": G.Context(0)}
    c["latency"].set_latency(True)
    return c


@functools.lru_cache(maxsize=None)
def case(pattern, n):
    """(layers without the LogSoftmax, x, logits float32): logits[r, c] =
    bias[c] + r * w0[c], exact in every mode."""
    rng = np.random.default_rng(9000 + n + 17 * PATTERNS.index(pattern))
    hot = [n // 3, n - 2]          # one mid-row, one in the last (ragged) chunk
    if pattern in ("dominant", "overflow"):
        bias, w0 = rng.integers(-60, -23, n), rng.integers(-3, 4, n)
        w0[hot] = 0
        if pattern == "dominant":
            bias[hot[0]] = 85
        else:
            bias[hot], w0[hot[1]] = [89, 90], 1
    elif pattern == "underflow":
        bias, w0 = rng.integers(-140, -111, n), rng.integers(-1, 2, n)
        bias[hot], w0[hot] = -104, [0, -1]
    else:
        bias, w0 = rng.integers(-100, -97, n), np.zeros(n, np.int64)
        up = rng.choice(n, 8, replace=False)   # eight logits climb to -90 by the last row
        w0[up], bias[up[0]], bias[up[1]] = 1, -98, -100
    W = np.zeros((IN_DIM, n), np.float32)
    W[0] = w0
    layers = [{"kind": "linear", "W": W, "b": bias.astype(np.float32)}]
    x = np.zeros((ROWS, IN_DIM), np.float32)
    x[:, 0] = np.arange(ROWS)
    netgen.check_exact_budget(layers, x)
    logits = netgen.exact(layers, x)
    assert np.array_equal(logits, bias[None, :] + np.arange(ROWS)[:, None] * w0[None, :])
    lo, hi = logits.min(), logits.max()
    if pattern == "dominant":
        assert hi == 85 and (np.sort(logits, axis=1)[:, -2] <= 0).all()
    elif pattern == "overflow":
        assert ((logits >= 89).sum(axis=1) == 2).all()
    elif pattern == "underflow":
        assert hi == -104 and (logits.max(axis=1) == -104).all()
    else:
        assert lo == -100 and hi == -90
        assert (np.exp(logits.astype(np.float64)).sum(axis=1) < FLT_MIN).all()   # the sum is a denormal
    for a in (x, logits):
        a.setflags(write=False)
    return layers, x, logits


def f64_log_softmax(logits):
    v = logits.astype(np.float64)
    m = v.max(axis=1, keepdims=True)
    return v - (m + np.log(np.exp(v - m).sum(axis=1, keepdims=True)))


def f64_softmax(logits):
    v = logits.astype(np.float64)
    e = np.exp(v - v.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def classes(a):
    return np.isposinf(a), np.isneginf(a), np.isnan(a)


def same_classes(got, want):
    return all(np.array_equal(g, w) for g, w in zip(classes(got), classes(want)))


def judge(pattern, got, oracle_out, want64, tol, what, pairs):
    """The pattern's bar on one result; pairs collects the denormal zone's
    (GPU error, oracle error)."""
    assert got.shape == oracle_out.shape, what
    if pattern == "dominant":
        assert np.isfinite(got).all() and np.isfinite(oracle_out).all(), what
        err = float(np.abs(got - want64).max())
        assert err <= tol, (what, err)
    elif pattern == "denormal":
        gpu_err, ref_err = float(np.abs(got - want64).max()), float(np.abs(oracle_out - want64).max())
        pairs.append((what, gpu_err, ref_err))
        print(f"{what}: GPU vs float64 {gpu_err:.3g}, oracle vs float64 {ref_err:.3g}")
        assert np.isfinite(oracle_out).all() and gpu_err <= max(tol, 2.0 * ref_err), (what, gpu_err, ref_err)
    else:
        assert same_classes(got, oracle_out), what
        fin = np.isfinite(oracle_out)
        assert np.abs(got[fin] - oracle_out[fin]).max(initial=0.0) <= tol, what


def runs(n):
    """(context flavour, gemm mode) pairs a width runs in: 510 is no multiple
    of 4, so its net is the fp32 program in every mode and context."""
    if n % 4:
        return [("plain", "fp32"), ("latency", "fp32")]
    return [("plain", "fp32"), ("plain", "bf16x6"), ("plain", "bf16"), ("latency", "bf16x6")]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", sorted(WIDTHS))
def test_log_softmax_finalize(torch, G, ctxs, oracle, n, pattern):
    linear, x, logits = case(pattern, n)
    layers = linear + [{"kind": "log_softmax"}]
    assert netgen.finalize_path(n) == WIDTHS[n]
    assert netgen.x6_ok(layers) == (n % 4 == 0)
    if n == 512:   # latency mode's fused tail
        assert netgen.kernels(layers, ROWS, "latency")[-1].endswith("+lat_finalize")
    ref = oracle.layer_forward(layers[-1], logits)
    want64 = f64_log_softmax(logits)
    if pattern == "overflow":
        assert np.isneginf(ref).all()
    if pattern == "underflow":
        assert np.isposinf(ref).all()
    prior = netgen.prior(n, 77)
    log_prior = np.log(prior.astype(np.float64))
    pairs = []
    for with_prior in (False, True):
        ref_p = (ref - log_prior.astype(np.float32)[None, :]).astype(np.float32) if with_prior else ref
        want_p = want64 - log_prior[None, :] if with_prior else want64
        for flavour, mode in runs(n):
            ctx = ctxs[flavour]
            model = G.Model(ctx, image=netgen.image(layers), prior=prior if with_prior else None)
            if mode != model.gemm:
                model.set_gemm(mode)
            assert model.gemm == mode
            got = G.nnet_propagate(ctx, model, dev(torch, x.copy()), subtract_prior=with_prior).cpu().numpy()
            judge(pattern, got, ref_p, want_p, LOGLIK_TOL, f"n={n} {flavour}/{mode} prior={with_prior}", pairs)


@pytest.mark.parametrize("op", ["log_softmax", "softmax"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", sorted(WIDTHS))
def test_row_ops(torch, G, ctxs, oracle, n, pattern, op):
    """ce_gpu_rowwise's stand-alone LogSoftmax and Softmax (exp x / sum: NaN
    where the oracle's inf / inf and 0 / 0 are)."""
    _, _, logits = case(pattern, n)
    ref = oracle.layer_forward({"kind": op}, logits)
    if op == "log_softmax":
        want64, tol = f64_log_softmax(logits), LOGLIK_TOL
    else:
        want64, tol = f64_softmax(logits), SOFTMAX_TOL
        if pattern == "overflow":
            assert (np.isnan(ref).sum(axis=1) == 2).all() and (ref[~np.isnan(ref)] == 0).all()
        if pattern == "underflow":
            assert np.isnan(ref).all()
    got = G.rowwise(ctxs["plain"], op, dev(torch, logits.copy())).cpu().numpy()
    judge(pattern, got, ref, want64, tol, f"n={n} rowwise {op}", [])
