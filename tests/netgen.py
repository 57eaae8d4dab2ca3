"""Generated nets for the GEMM shape tests (tests/test_gpu_gemm_shapes.py).

Exact-integer nets.  When every input, weight, bias and BatchNorm parameter
is an integer and, for every Linear, sum_k |a_ik| |w_kj| + |b_j| < 2^24, every
partial sum of every summation order is an integer that float32 represents
exactly: a naive fp32 GEMM, an fp64 GEMM and any correct fp32 GEMM kernel --
whatever its tiles, its split-K order or the MFMA's internal accumulation --
give the same bits.  The bf16x6 kernels drop three of the nine plane products
(a1b2, a2b1, a2b2), f16x3 one of four (a1b1); those are exactly zero when, per
Linear, one operand fits one plane or both fit two.  check_exact_budget
asserts all of it on the actual operands and their planes, so a mismatch on
the GPU is the kernel's, not the recipe's (tests/test_netgen.py runs the
oracle in three orders on every case as the proof).

Which plane products a case makes nonzero, at which Linear, is census()'s
answer; drop_product() is the kernel that skipped one.  The plane recipes
(W3, A3, P11; F1, FX, FW for f16x3) exist so that every product a form keeps
reaches output bits at every position of every kernel family: coverage(),
asserted cell by cell in tests/test_netgen.py.

Real-valued nets: the same geometry with synth.tdnn_layers' variance-
preserving float weights, compared against an fp64 evaluation.
"""
import functools

import numpy as np

from catears_amd import formats, synth

EXACT_LIMIT = float(1 << 24)

# (max |w|, nonzeros per column) per Linear; a third entry is the smallest
# |w| and makes every weight odd (a full-width significand).
# WIDE: small weights (one bf16 plane), activations growing layer by layer.
# The third Linear of a net reads values beyond 2^16, but round-to-nearest
# residuals let h + m cover 17 significant bits and these activations need no
# more: WIDE reaches the products a0b0 and a1b0 only, never a third plane
# (census(); the W3 / A3 / P11 recipes below are there for the rest).
WIDE = [(3, 24), (15, 12), (31, 10), (15, 8)]
# TWO_PLANES: inputs up to 1023 and first-layer weights up to 2047 (two bf16
# planes each), then ternary layers; BatchNorm scales +-1 (a scale of 2 per
# layer would leave the 2^24 budget).
TWO_PLANES = [(2047, 1), (1, 2), (1, 2), (1, 2)]


def _ints(rng, lo, hi, size):
    return rng.integers(lo, hi + 1, size=size).astype(np.float32)


def _splice_layers(idx):
    idx = [int(i) for i in idx]
    if idx == [0]:
        return []
    return [{"kind": "splice", "indices": idx},
            {"kind": "narrow", "left": -min(min(idx), 0), "right": max(max(idx), 0)}]


def _assemble(in_dim, widths, splices, post, linear, batchnorm, log_softmax):
    assert len(widths) == len(splices) == len(post)
    layers = []
    width = in_dim
    for i, (n, idx, ops) in enumerate(zip(widths, splices, post)):
        assert len(ops) <= 4 and sum(op == "batchnorm" for op in ops) <= 1, ops
        layers += _splice_layers(idx)
        layers.append(linear(i, width * len(idx), n))
        for op in ops:
            layers.append({"kind": "relu"} if op == "relu" else batchnorm(n))
            assert op in ("relu", "batchnorm"), op
        width = n
    if log_softmax:
        layers.append({"kind": "log_softmax"})
    return layers


def int_net(in_dim, widths, splices, post, spec, seed, log_softmax=False, bn_scales=(1.0, 2.0, -1.0), bias=64):
    """Layer list (formats.nnet_bytes' vocabulary) of an exact-integer net.
    widths: output width per Linear; splices: index list per Linear ([0]: no
    Splice); post: per Linear a tuple out of "relu" / "batchnorm" (at most 4,
    one BatchNorm: what the loader fuses); spec: per Linear (max |w|, nonzeros
    per column[, min |w|: then every weight is odd]).  Weights are sparse
    integers, biases integers in [-bias, bias], BatchNorm scales out of
    bn_scales with integer offsets in [-8, 8]."""
    rng = np.random.default_rng(seed)

    def linear(i, k, n):
        wmax, nnz = spec[i][:2]
        nnz = min(nnz, k)
        W = np.zeros((k, n), np.float32)
        rows = rng.integers(0, k, size=(nnz, n))
        mag = rng.integers(spec[i][2] if len(spec[i]) > 2 else 1, wmax + 1, size=(nnz, n))
        if len(spec[i]) > 2:
            mag |= 1
        sign = rng.integers(0, 2, size=(nnz, n)) * 2 - 1
        W[rows, np.arange(n)[None, :]] = (mag * sign).astype(np.float32)
        return {"kind": "linear", "W": W, "b": _ints(rng, -bias, bias, n)}

    def batchnorm(n):
        return {"kind": "batchnorm", "scale": np.array(bn_scales, np.float32)[rng.integers(0, len(bn_scales), size=n)],
                "offset": _ints(rng, -8, 8, n)}

    return _assemble(in_dim, widths, splices, post, linear, batchnorm, log_softmax)


def real_net(in_dim, widths, splices, post, seed, log_softmax=True):
    """The same geometry with synth.tdnn_layers' weights: W ~ U(-1, 1) *
    sqrt(3 / K), small biases, BatchNorm scales near 1."""
    tensor = [0]

    def draw(n, lo, hi):
        tensor[0] += 1
        return synth.uniform(seed * 1000003 + tensor[0], n, lo, hi)

    def linear(i, k, n):
        W = (draw(k * n, -1.0, 1.0) * np.sqrt(3.0 / k)).astype(np.float32).reshape(k, n)
        return {"kind": "linear", "W": W, "b": (0.1 * draw(n, -1.0, 1.0)).astype(np.float32)}

    def batchnorm(n):
        return {"kind": "batchnorm", "scale": (1.0 + 0.1 * draw(n, -1.0, 1.0)).astype(np.float32),
                "offset": (0.1 * draw(n, -1.0, 1.0)).astype(np.float32)}

    return _assemble(in_dim, widths, splices, post, linear, batchnorm, log_softmax)


def context(layers):
    """(left, right): the rows the net's Narrow layers drop."""
    return (sum(L["left"] for L in layers if L["kind"] == "narrow"),
            sum(L["right"] for L in layers if L["kind"] == "narrow"))


def image(layers):
    """The NN02 bytes gpu.Model(ctx, image=...) loads."""
    return formats.nnet_bytes(layers, *context(layers))


def in_dim(layers):
    segs = 1
    for L in layers:
        if L["kind"] == "splice":
            segs = len(L["indices"])
        if L["kind"] == "linear":
            return L["W"].shape[0] // segs
    raise ValueError("no Linear layer")


def int_input(layers, rows, seed, amax=7, amin=None):
    """rows + left + right input rows of integers in [-amax, amax]; with amin
    odd integers of magnitude amin .. amax."""
    left, right = context(layers)
    shape = (rows + left + right, in_dim(layers))
    rng = np.random.default_rng(seed)
    if amin is None:
        return _ints(rng, -amax, amax, shape)
    return ((rng.integers(amin, amax + 1, size=shape) | 1) * (rng.integers(0, 2, size=shape) * 2 - 1)).astype(np.float32)


def real_input(layers, rows, seed):
    """rows + left + right input rows ~ N(0, 3)."""
    left, right = context(layers)
    return np.random.default_rng(seed).normal(0.0, 3.0, size=(rows + left + right, in_dim(layers))).astype(np.float32)


def prior(n, seed):
    p = synth.uniform(seed, n, 0.5, 1.5)
    return (p / p.sum()).astype(np.float32)


def binade_shift(layers, x, e):
    """The same net with the input scaled by 2^e and the first Linear's
    weights by 2^-e: every first-layer product is unchanged (a power-of-two
    scaling is exact), so the outputs carry the same bits, while every
    first-layer operand is split into planes |e| binades away."""
    out = [dict(L) for L in layers]
    first = next(L for L in out if L["kind"] == "linear")
    first["W"] = np.ldexp(first["W"], -e).astype(np.float32)
    xs = np.ldexp(np.asarray(x, np.float32), e).astype(np.float32)
    assert np.all(np.isfinite(xs)) and np.all(np.isfinite(first["W"]))
    assert np.array_equal(np.ldexp(xs.astype(np.float64), -e), np.asarray(x, np.float64))
    return out, xs


def _walk(layers, x, visit=None, product=None):
    """fp64 evaluation.  Splice + Narrow together keep the rows whose every
    spliced row exists (the rows the reference's clamped Splice computes and
    its Narrow keeps).  visit(linear_layer, its_input) is called per Linear,
    visit(batchnorm_layer, its_input) per BatchNorm; product(linear_index,
    its_input, W) replaces the fp64 a @ W of a Linear."""
    x = np.asarray(x, np.float64)
    i, n_linear = 0, 0
    while i < len(layers):
        L = layers[i]
        k = L["kind"]
        if k == "splice":
            nar = layers[i + 1]
            assert nar["kind"] == "narrow"
            idx, left, right = L["indices"], nar["left"], nar["right"]
            assert left == -min(min(idx), 0) and right == max(max(idx), 0)
            rows = x.shape[0] - left - right
            assert rows > 0, "input does not cover the context"
            x = np.concatenate([x[left + o:left + o + rows] for o in idx], axis=1)
            i += 1
        elif k == "narrow":
            assert L["left"] == 0 and L["right"] == 0
        elif k == "linear":
            if visit:
                visit(L, x)
            W = L["W"].astype(np.float64)
            x = (product(n_linear, x, W) if product else x @ W) + L["b"].astype(np.float64)
            n_linear += 1
        elif k == "relu":
            x = np.where(x < 0.0, 0.0, x)
        elif k == "batchnorm":
            if visit:
                visit(L, x)
            x = x * L["scale"].astype(np.float64) + L["offset"].astype(np.float64)
        elif k == "log_softmax":
            m = x.max(axis=1, keepdims=True)
            x = x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))
        else:
            raise ValueError(k)
        i += 1
    if visit:
        visit(None, x)
    return x


def eval_f64(layers, x):
    """The net in float64 (every operation, the LogSoftmax included)."""
    return _walk(layers, x)


def exact(layers, x):
    """eval_f64 cast to float32: for a net inside check_exact_budget the
    bits every correct fp32 evaluation must produce."""
    return eval_f64(layers, x).astype(np.float32)


# ------------------------------------------------------------- the planes --
# What the split GEMMs make of an operand, restated from their definitions
# (csrc/bf16_split.h; kernels/gemm_f16x3.hip and the weight scale of
# csrc/weight_images.cc), in numpy and apart from the project's host code.

FORMS = ("bf16x6", "f16x3")
# the plane products (activation plane, weight plane) each form computes
KEPT = {"bf16x6": ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0)), "f16x3": ((0, 0), (0, 1), (1, 0))}
F16_ACT_SHIFT = -8          # activations are stored as x * 2^-8
F16_ACT_LIMIT = 16000000.0  # beyond it a hidden output sets the overflow flag


def _f32(v):
    v64 = np.asarray(v, np.float64)
    v32 = v64.astype(np.float32)
    assert np.all(np.isfinite(v32)) and np.array_equal(v32.astype(np.float64), v64), "not float32 values"
    return v32


def bf16_rne(v):
    """float32 -> the nearest bfloat16 (ties to even), as a float32."""
    u = _f32(v).view(np.uint32)        # finite: the sum below cannot carry out of 32 bits
    return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)).view(np.float32)


def split3_planes(v):
    """(h, m, l), float64: three successive round-to-nearest-even bf16
    roundings of the exact residual (split3 of bf16_split.h: each of its fp32
    subtractions is exact).  Asserts h + m + l == v."""
    v = _f32(v).astype(np.float64)
    h = bf16_rne(v).astype(np.float64)
    m = bf16_rne(v - h).astype(np.float64)
    l = bf16_rne(v - h - m).astype(np.float64)
    assert np.array_equal(h + m + l, v), "three bf16 planes do not hold the value"
    return h, m, l


def f16_weight_shift(W):
    """f16_plane_image's per-layer scale: max |w| * 2^s in [2^14, 2^15)."""
    mx = float(np.abs(W).max())
    e = int(np.frexp(np.float32(mx))[1]) if mx > 0.0 else 0
    return max(-100, min(100, 15 - e))


def split2_raw(v, s):
    """(x0, x1) as float32: u = v * 2^s, x0 = f16(u), x1 = f16((u - x0) *
    2^11), in fp32 arithmetic as split2 of gemm_f16x3.hip and
    f16_plane_image have it."""
    u = np.ldexp(_f32(v), s).astype(np.float32)
    x0 = u.astype(np.float16)
    x1 = ((u - x0.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    assert np.all(np.isfinite(x0)) and np.all(np.isfinite(x1)), "beyond fp16's range"
    return x0.astype(np.float32), x1.astype(np.float32)


def split2_planes(v, s):
    """(p0, p1), float64, in the units of v: p0 = x0 * 2^-s, p1 = x1 * 2^-11
    * 2^-s of split2_raw.  Two planes of 11 bits: the sum need not be v
    (check_exact_budget asserts it where a test relies on it)."""
    x0, x1 = split2_raw(v, s)
    return np.ldexp(x0.astype(np.float64), -s), np.ldexp(x1.astype(np.float64), -s - 11)


def planes(v, form, weights=False):
    """The planes of an operand under `form` (weights: the f16x3 layer scale)."""
    if form == "bf16x6":
        return split3_planes(v)
    assert form == "f16x3", form
    return split2_planes(v, f16_weight_shift(v) if weights else F16_ACT_SHIFT)


def _meet(pa, pw):
    """|pa| @ |pw| is nonzero somewhere: some k has a nonzero in pa's column
    and in pw's row."""
    return bool(((pa != 0.0).any(axis=0) & (pw != 0.0).any(axis=1)).any())


def _per_linear(layers, x, fn):
    out = []
    _walk(layers, x, lambda L, a: out.append(fn(a, L)) if L and L["kind"] == "linear" else None)
    return out


def census(layers, x, form):
    """Per Linear the set of plane pairs (i, j) with |a_i| @ |w_j| nonzero
    somewhere: the plane products that contribute to the net's outputs on x."""
    def pairs(a, L):
        ap, wp = planes(a, form), planes(L["W"], form, weights=True)
        return {(i, j) for i, pa in enumerate(ap) for j, pw in enumerate(wp) if _meet(pa, pw)}
    return _per_linear(layers, x, pairs)


def drop_product(layers, x, linear_index, pair, form):
    """The net's outputs (float32 of the fp64 walk) with the plane product
    `pair` = (i, j) left out of Linear `linear_index`: what a kernel that
    skipped it, or read a zero plane there, would give."""
    def product(n, a, W):
        if n != linear_index:
            return a @ W
        return a @ W - planes(a, form)[pair[0]] @ planes(W, form, weights=True)[pair[1]]
    return _walk(layers, x, product=product).astype(np.float32)


def check_exact_budget(layers, x, form="bf16x6"):
    """Raises AssertionError unless the net on input x is exact in fp32 in
    every summation order and under the split of `form`: integer operands;
    per BatchNorm |x| |scale| + |offset| < 2^24; per Linear, with P(v) the sum
    of |v|'s planes (P(v) = |v| for a one-plane operand), max_ij (sum_k
    P(a_ik) P(w_kj) + |b_j|) < 2^24 -- every partial sum of every plane
    product, in any order and in any number of accumulators, is then an
    integer that float32 holds -- and every plane product the form drops
    (a1b2, a2b1, a2b2; f16x3: a1b1) identically zero.  f16x3 in addition: the
    planes hold every operand exactly (inputs, weights and hidden outputs
    reconstruct from two fp16 planes) and every activation stays below the
    overflow limit of 16 000 000.
    Returns the log2 of each Linear's bound."""
    assert form in FORMS, form
    bounds = []

    def integers(v, what):
        v = np.asarray(v, np.float64)
        assert np.all(np.isfinite(v)) and np.array_equal(v, np.rint(v)), f"{what}: not integers"

    def visit(L, a):
        integers(a, "activations")
        if L is None:
            assert np.abs(a).max() < EXACT_LIMIT, "output beyond 2^24"
            return
        if L["kind"] == "batchnorm":
            integers(L["scale"], "BatchNorm scale")
            integers(L["offset"], "BatchNorm offset")
            bound = (np.abs(a) * np.abs(L["scale"]).astype(np.float64) + np.abs(L["offset"])).max()
            assert bound < EXACT_LIMIT, f"BatchNorm bound 2^{np.log2(bound):.1f}"
            return
        integers(L["W"], "weights")
        integers(L["b"], "bias")
        ap, wp = planes(a, form), planes(L["W"], form, weights=True)
        if form == "f16x3":
            assert np.abs(a).max() < F16_ACT_LIMIT, f"f16x3: max |a| {np.abs(a).max()} sets the overflow flag"
            assert np.array_equal(ap[0] + ap[1], a), "f16x3: two planes do not hold the activations"
            assert np.array_equal(wp[0] + wp[1], L["W"]), "f16x3: two planes do not hold the weights"
        for p in ap + wp:
            integers(p, "planes")
        bound = (sum(np.abs(p) for p in ap) @ sum(np.abs(p) for p in wp) + np.abs(L["b"])).max()
        assert bound < EXACT_LIMIT, f"Linear bound 2^{np.log2(bound):.1f} >= 2^24"
        for i, pa in enumerate(ap):
            for j, pw in enumerate(wp):
                if (i, j) not in KEPT[form]:
                    assert not _meet(pa, pw), \
                        f"{form} would drop a nonzero a{i}b{j}: max |a| {np.abs(a).max()}, max |w| {np.abs(L['W']).max()}"
        bounds.append(float(np.log2(max(bound, 1.0))))

    assert not any(L["kind"] == "log_softmax" for L in layers), "LogSoftmax is not exact"
    _walk(layers, x, visit)
    return bounds


# ------------------------------------------------------------- geometries --

S5 = [-2, -1, 0, 1, 2]
RB, BR, RBR = ("relu", "batchnorm"), ("batchnorm", "relu"), ("relu", "batchnorm", "relu")

# id -> (in_dim, widths, splices, post).  Every PostMode (none, relu,
# batchnorm, relu+batchnorm, batchnorm+relu, generic) is on a hidden layer
# and on a last layer of an x6 geometry with n <= 4096 (lat_finalize) --
# and the generic chain also on F's n > 4096 (lat_reduce + the loop finalize).
GEOMETRIES = {
    "A": (40, [96, 800, 772], [S5, [-1, 0, 2], [0]], [RB, BR, ("relu",)]),
    "B": (40, [32, 64, 36], [[0], [0], [0]], [("relu",), (), ("batchnorm",)]),
    "C": (24, [96, 64, 100], [[-3, -2, -1, 0, 1, 2, 3], [-7, -3, -1, 0, 2, 5, 9, 20], [0]],
          [("batchnorm",), RBR, ()]),
    # 800 wide after the padded first layer, so that a 3000-row block takes
    # the 512 x 128 kernel there (K of 128: 4 tiles) and the second layer has
    # an odd 75 K-tiles
    "D": (13, [800, 256, 1028], [S5, [-1, 0, 1], [0]], [RB, ("relu",), RB]),
    "E": (40, [100, 100, 37], [S5, [-1, 0, 1], [0]], [RBR, (), BR]),
    "F4100": (40, [96, 640, 4100], [S5, [-1, 0, 2], [0]], [RB, BR, RBR]),
    "F4099": (40, [96, 640, 4099], [S5, [-1, 0, 2], [0]], [RB, BR, RBR]),
    "G9": (40, [288, 3456], [S5, [0]], [RB, BR]),
    "G25": (40, [800, 3456], [S5, [0]], [BR, RBR]),
    "G20": (40, [640, 3456], [S5, [0]], [("batchnorm",), RB]),
    # two Linears of B with every operand one fp16 plane: the f16x3 recipe
    "B2": (40, [32, 36], [[0], [0]], [RB, ("batchnorm",)]),
    # a first layer whose segments are whole K-tiles (64 wide): the fp32
    # program hands the caller's own pointer and row stride to the GEMM, the
    # bf16x6 program reads the caller's rows through the splice offsets in the
    # generic direct-weight kernel (no `first` gather form)
    "H": (64, [96, 64, 36], [[-2, 0, 1], [-1, 0, 1], [0]], [RB, BR, ()]),
}

ROWS = (1, 17, 70, 129)
BIG_ROWS = 3000
BIG = ("A", "D", "G9", "G25", "G20")   # reach the 512 x 128 kernel only there
BINADE = ("A", "C")                    # +-60-binade variants
TWO_PLANE_GEOMS = ("A", "B", "C", "D", "H")  # also run with the TWO_PLANES recipe

# The plane recipes: each puts operands of a chosen number of planes at a
# chosen Linear p, so that the plane products WIDE and TWO_PLANES leave zero
# (census() on the committed cases; the table is in DESIGN.md) contribute to
# output bits.  BatchNorm scales +-1 and biases in [-4, 4] keep the 2^24
# budget for the operands.
#   W3@p  one-plane activations (ternary layers before p) times odd weights
#         of 18-19 significant bits at p: a0b0, a0b1, a0b2 there, and the
#         three-plane outputs give a0b0, a1b0, a2b0 behind it
#   A3    odd inputs of 20 bits: a0b0, a1b0, a2b0 at every Linear
#   P11@p a hidden or last Linear with two-plane activations and two-plane
#         weights: all of a0b0, a0b1, a1b0, a1b1 there
# f16x3 (two fp16 planes of 11 bits):
#   F1    every operand fits one plane: a0b0 alone, on every x6 geometry
#   FX    odd inputs of 14 bits: a1b0 at the first and the hidden Linears
#   FW@p  odd weights of 14 bits at p (every p) on one-plane activations: a0b1
PLANE_GEOMS = ("A", "D", "G9", "H")    # the bf16x6 plane recipes run there ...
# ... at BIG_ROWS too on A and G9, the smallest nets that reach the 512 x 128
# kernel, and the first-layer recipes on D, the only net that runs that
# kernel on a first layer
PLANE_BIG = {"A": None, "G9": None, "D": ("W3@0", "A3")}   # None: every recipe
PLANE_BINADE = ("W3@0", "A3")          # +-60-binade forms, on A
F16_GEOMS = ("A", "B", "C", "D", "G9", "G20", "H")   # FX / FW; F1: wherever x6_ok holds
BIAS = 4


def _w3(n, p):
    at = ((1 << 18) - 1, 2, 1 << 17) if p == 0 else ((1 << 19) - 1, 1, 1 << 18)
    return [(1, 2)] * p + [at] + [(1, 1)] * (n - p - 1)


def _p11(n, p):
    return ([(63, 4)] if p == 1 else [(3, 2), (31, 2)]) + [(2047, 2, 1024)] + [(1, 1)] * (n - p - 1)


def _fw(n, p):
    return [(1, 2)] * p + [((1 << 14) - 1, 2, 1 << 13)] + [(1, 1)] * (n - p - 1)


def plane_recipes(n, form="bf16x6"):
    """{name: (spec, input arguments)} for a net of n Linears."""
    if form == "f16x3":
        r = {"F1": ([(3, 4), (3, 4), (3, 2)][:n], dict(amax=7)),
             "FX": ([(1, 2)] + [(1, 1)] * (n - 1), dict(amax=(1 << 14) - 1, amin=1 << 13))}
        for p in range(n):
            r[f"FW@{p}"] = (_fw(n, p), dict(amax=3))
        return r
    r = {f"W3@{p}": (_w3(n, p), dict(amax=3 if p == 0 else 2)) for p in range(n)}
    r["A3"] = ([(1, 2)] + [(1, 1)] * (n - 1), dict(amax=(1 << 20) - 1, amin=1 << 19))
    for p in range(1, n):
        r[f"P11@{p}"] = (_p11(n, p), dict(amax=7))
    return r


def case_rows(geom, name):
    """The row counts the GPU tests score a case at: ROWS, and BIG_ROWS where
    the geometry reaches the 512 x 128 kernel (the plane recipes: on the
    smallest such nets only, the f16x3 ones nowhere)."""
    recipe = name.split("*")[0]
    if recipe in ("wide", "two-planes"):
        big = geom in BIG
    else:
        big = recipe[0] != "F" and geom in PLANE_BIG and (PLANE_BIG[geom] is None or recipe in PLANE_BIG[geom])
    return ROWS + ((BIG_ROWS,) if big else ())


def max_rows(geom, name="wide"):
    return case_rows(geom, name)[-1]


def geom_x6_ok(geom):
    """x6_ok of the geometry's nets (the rule reads widths only)."""
    _, widths, _, _ = GEOMETRIES[geom]
    return all(n % 4 == 0 for n in widths) and all(n % 32 == 0 for n in widths[:-1])


def recipe_names(geom, form="bf16x6"):
    """The plane recipes exact_cases(geom, form) holds."""
    names = list(plane_recipes(len(GEOMETRIES[geom][1]), form))
    if form == "f16x3":
        return [r for r in names if r == "F1" or geom in F16_GEOMS] if geom_x6_ok(geom) else []
    return names if geom in PLANE_GEOMS else []


def exact_cases(geom, form="bf16x6"):
    """[(name, layers, x)] of the exact-integer leg of one geometry.  bf16x6
    (every mode but f16x3 runs these): the WIDE recipe, its binade-shifted
    forms, the TWO_PLANES recipe, the plane recipes W3@p, A3, P11@p with the
    binade-shifted W3@0 and A3.  f16x3: F1, FX, FW@p (and B2's own "wide").
    x has max_rows(geom, name) + left + right rows; the first r + left +
    right of them give the first r output rows."""
    in_d, widths, splices, post = GEOMETRIES[geom]
    seed = 1000 + sorted(GEOMETRIES).index(geom)
    cases = []
    if form == "bf16x6" or geom == "B2":
        layers = int_net(in_d, widths, splices, post, WIDE, seed)
        x = int_input(layers, max_rows(geom), seed + 500)
        cases.append(("wide", layers, x))
    if form == "bf16x6":
        if geom in BINADE:
            for e in (60, -60):
                cases.append((f"wide*2^{e}",) + binade_shift(layers, x, e))
        if geom in TWO_PLANE_GEOMS:
            l2 = int_net(in_d, widths, splices, post, TWO_PLANES, seed + 1, bn_scales=(1.0, -1.0))
            cases.append(("two-planes", l2, int_input(l2, max_rows(geom), seed + 501, amax=1023)))
    names = recipe_names(geom, form)
    for i, name in enumerate(names):
        spec, xargs = plane_recipes(len(widths), form)[name]
        ln = int_net(in_d, widths, splices, post, spec, seed + 10 + i, bn_scales=(1.0, -1.0), bias=BIAS)
        xn = int_input(ln, max_rows(geom, name), seed + 510 + i, **xargs)
        cases.append((name, ln, xn))
        if geom == "A" and name in PLANE_BINADE:
            for e in (60, -60):
                cases.append((f"{name}*2^{e}",) + binade_shift(ln, xn, e))
    return cases


def one_plane_mode_cases(geom):
    """exact_cases(geom) without the plane recipes: the cases of the modes
    that keep one plane per operand (plain bf16: tests/test_gemm_bf16.py,
    tests/test_gpu_gemm_bf16.py), whose bits are defined by one rounding per
    operand and not by plane products."""
    return [c for c in exact_cases(geom) if c[0].split("*")[0] in ("wide", "two-planes")]


# ------------------------------------------------ the dispatch rules, read --
# A restatement of the host-side kernel choice (csrc/model.cc build_program,
# csrc/nnet_programs.cc run_steps_*, kernels/gemm_bf16x6.hip launch_gemm_bf16x6 / gemm_bf16x6_kernels.h x6w_fits,
# kernels/gemm_bf16x6_lat.hip x6_lat_slices, kernels/gemm_f32.hip launch_glds,
# kernels/rowops.hip launch_finalize), so tests/test_netgen.py can assert
# that every geometry reaches the path it is there for.

def linears(layers):
    """Per Linear: dict(din, nseg, off, k, n) as the loader sees it."""
    out, segs = [], [0]
    for L in layers:
        if L["kind"] == "splice":
            segs = list(L["indices"])
        elif L["kind"] == "linear":
            k, n = L["W"].shape
            out.append(dict(din=k // len(segs), nseg=len(segs), off=segs, k=k, n=n))
            segs = [0]
    return out


def x6_ok(layers):
    """build_program's rule for the bf16x6 / f16x3 programs (every post op
    of these nets is fused, so every step is a GEMM)."""
    return all(g["n"] % 4 == 0 and (i == 0 or g["din"] % 32 == 0) for i, g in enumerate(linears(layers)))


def lat_slices(ktiles, n):
    """x6_lat_slices: K-tiles per slice of the latency GEMM, slice by slice."""
    cols = (n + 63) // 64
    slices = max(1, min(ktiles, 256 // cols))
    per = min((ktiles + slices - 1) // slices, 8)
    count = (ktiles + per - 1) // per
    return [min(per, ktiles - s * per) for s in range(count)]


def finalize_path(n):
    """launch_finalize's three row kernels."""
    return "loop" if n > 4096 else ("vector" if n % 4 == 0 else "scalar")


def kernels(layers, out_rows, mode, caller_aligned=True):
    """Per Linear the kernel `mode` runs on a block of out_rows output rows
    (the GEMMs see out_rows + left + right rows); mode: fp32, bf16x6,
    bf16x6p, wide, latency.  A net that is not x6_ok runs the fp32 program
    whatever was asked.  caller_aligned: the caller's rows are float4 rows
    (16-byte aligned base, ld_in % 4 == 0); without it no kernel reads them
    with 16-byte loads: the bf16x6 / latency first layer goes through
    splice_pad (run_steps_x6f's lat_direct) and an fp32 first layer of whole
    K-tiles leaves the LDS-DMA kernel for pipe2 (launch_gemm_f32's a_fast)."""
    left, right = context(layers)
    m = out_rows + left + right
    ok = x6_ok(layers)
    names = []
    for i, g in enumerate(linears(layers)):
        k64 = (g["k"] + 63) // 64 * 64            # the loader pads K to 64
        if mode == "fp32" or not ok:
            # segments that are not whole K-tiles: the spliced block is written
            # once, zero padded, and the same kernel runs on it
            if g["din"] % 32 != 0:
                names.append("splice_pad+f32_glds")
            else:
                names.append("f32_glds" if i > 0 or caller_aligned else "f32_pipe2")
            continue
        ktiles = (k64 if i == 0 else g["k"]) // 32
        if mode == "bf16x6p":
            names.append(("splice_pad_split+" if i == 0 else "") + f"x6q_128x128[kt={ktiles}]")
            continue
        # the loader splices the caller's rows itself (lat_direct)
        gathered = i == 0 and g["din"] % 8 == 0 and caller_aligned
        pad = "splice_pad+" if i == 0 and not gathered else ""
        if mode == "latency":
            sl = lat_slices(ktiles, g["n"])
            last = i + 1 == len(linears(layers))
            tail = "lat_finalize" if last and m <= 1024 and g["n"] <= 4096 else "lat_reduce"
            names.append(f"{pad}lat_gemm<KT={(max(sl) + 1) // 2 * 2}>[{','.join(map(str, sl))}]+{tail}")
            continue
        first = gathered and g["din"] % 32 != 0   # launch_gemm_bf16x6's `first`
        tiles_n, tiles_m = (g["n"] + 511) // 512, (m + 127) // 128
        if mode == "wide" or first:
            names.append(f"{pad}x6d_128x128{'_gather' if first else ''}[kt={ktiles}]")
        elif (g["n"] + 255) // 256 * 256 >= tiles_n * 512 and tiles_n * tiles_m >= 48:
            names.append(f"{pad}x6w_512x128[kt={ktiles}]")
        else:
            names.append(f"{pad}x6d_256x128[kt={ktiles}]")
    return names


def f16x3_kernels(layers):
    """Per Linear the f16x3 program's launch (run_steps_chain16<ChainF16>,
    launch_gemm_f16x3): the first layer reads the block splice_pad_f16 wrote
    (one segment, K padded to 64: K-tiles of 64), a later one gathers its
    segments through the packed splice offsets, with K-tiles of 64 only when
    a segment is whole ones."""
    assert x6_ok(layers)
    return [("splice_pad_f16+x3<BK=64>" if i == 0 else
             f"x3<BK={64 if g['din'] % 64 == 0 else 32}>" + ("[spliced]" if g["nseg"] > 1 else ""))
            for i, g in enumerate(linears(layers))]


# --------------------------------------------------- the coverage matrix --
# family -> (the positions it can run at, its test on a kernels() name).  The
# last Linear of a two-Linear net (it reads the first layer's output) and of
# a three-Linear net (it reads a hidden layer's) are positions of their own.
FIRST, HIDDEN, LAST2, LAST3 = "first", "hidden", "last of two", "last of three"
LATER = (HIDDEN, LAST2, LAST3)
FAMILIES = {
    "bf16x6": {
        "x6d_128x128_gather": ((FIRST,), lambda k: "_gather[" in k),
        "splice_pad+": ((FIRST,), lambda k: k.startswith("splice_pad+")),
        "splice_pad_split+x6q": ((FIRST,), lambda k: k.startswith("splice_pad_split+x6q")),
        "x6q_128x128": (LATER, lambda k: k.startswith("x6q_")),
        # first: H's generic direct first layer (the caller's rows through the splice offsets)
        "x6d_256x128": ((FIRST,) + LATER, lambda k: k.startswith("x6d_256x128[")),
        "x6w_512x128": ((FIRST,) + LATER, lambda k: "x6w_512x128[" in k),
        "wide x6d_128x128": ((FIRST,) + LATER, lambda k: k.startswith("x6d_128x128[")),
        "lat_gemm+lat_reduce": ((FIRST,) + LATER, lambda k: k.startswith("lat_gemm") and k.endswith("+lat_reduce")),
        "lat_gemm+lat_finalize": ((LAST2, LAST3), lambda k: k.startswith("lat_gemm") and k.endswith("+lat_finalize")),
    },
    "f16x3": {
        "splice_pad_f16+x3<BK=64>": ((FIRST,), lambda k: k.startswith("splice_pad_f16+")),
        # no geometry has a middle Linear of 64-wide segments: K-tiles of 64
        # behind the first layer run on last layers only
        # (tests/test_netgen.py asserts it, so a new geometry adds the cell)
        "x3<BK=64>": ((LAST2, LAST3), lambda k: k.startswith("x3<BK=64>")),
        "x3<BK=32>": (LATER, lambda k: k.startswith("x3<BK=32>")),
        "x3 spliced": ((HIDDEN,), lambda k: k.endswith("[spliced]")),
    },
}
X6_MODES = ("bf16x6", "bf16x6p", "wide", "latency")


@functools.lru_cache(maxsize=None)
def _case_census(geom, form):
    """[(name, layers, census of the first ROWS[-1] output rows)]: what is
    nonzero there is nonzero in every larger block."""
    out = []
    for name, layers, x in exact_cases(geom, form):
        if "*2^" not in name and x6_ok(layers):
            out.append((name, layers, census(layers, x[:ROWS[-1] + sum(context(layers))], form)))
    return out


def launches(form):
    """(geom, case, Linear index, position, mode, rows, kernel, the plane
    pairs nonzero there) of every Linear of every exact case (the
    binade-shifted forms apart) in every mode and at every row count the GPU
    test scores the case at."""
    for geom in GEOMETRIES:
        for name, layers, nonzero in _case_census(geom, form):
            n = len(nonzero)
            runs = [("f16x3", r, f16x3_kernels(layers)) for r in case_rows(geom, name)] if form == "f16x3" else \
                   [(mode, r, kernels(layers, r, mode)) for mode in X6_MODES for r in case_rows(geom, name)]
            for mode, r, names in runs:
                for li, k in enumerate(names):
                    pos = FIRST if li == 0 else HIDDEN if li < n - 1 else LAST2 if n == 2 else LAST3
                    yield geom, name, li, pos, mode, r, k, nonzero[li]


def coverage(form, skip=()):
    """{(family, position, plane pair): [(geom, case, Linear index, mode,
    rows)]}: where the exact cases (but those named in `skip`) have the pair
    nonzero at a Linear that runs a kernel of the family, over launches(form).
    A family's cell exists at the positions it can run at; a first-layer-only
    kernel has no hidden cell."""
    cells = {(f, pos, pair): [] for f, (positions, _) in FAMILIES[form].items() for pos in positions
             for pair in KEPT[form]}
    for geom, name, li, pos, mode, r, k, nonzero in launches(form):
        if name in skip:
            continue
        for f, (positions, match) in FAMILIES[form].items():
            if pos in positions and match(k):
                for pair in nonzero & set(KEPT[form]):
                    cells[f, pos, pair].append((geom, name, li, mode, r))
    return cells
