"""Generated nets for the GEMM shape tests (tests/test_gpu_gemm_shapes.py).

Exact-integer nets.  When every input, weight, bias and BatchNorm parameter
is an integer and, for every Linear, sum_k |a_ik| |w_kj| + |b_j| < 2^24, every
partial sum of every summation order is an integer that float32 represents
exactly: a naive fp32 GEMM, an fp64 GEMM and any correct fp32 GEMM kernel --
whatever its tiles, its split-K order or the MFMA's internal accumulation --
give the same bits.  The bf16x6 kernels drop three of the nine plane products
(a1b2, a2b1, a2b2); those are exactly zero when, per Linear, the inputs or the
weights fit one bf16 plane (|v| <= 255) or both fit two (|v| <= 65535).
check_exact_budget asserts all of it on the actual operands, so a mismatch
on the GPU is the kernel's, not the recipe's (tests/test_netgen.py runs the
oracle in three orders on every case as the proof).

Real-valued nets: the same geometry with synth.tdnn_layers' variance-
preserving float weights, compared against an fp64 evaluation.
"""
import numpy as np

from catears_amd import formats, synth

EXACT_LIMIT = float(1 << 24)

# (max |w|, nonzeros per column) per Linear.
# WIDE: small weights (one bf16 plane), activations growing layer by layer:
# the third Linear of a net reads values beyond 2^16, all three planes set.
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


def int_net(in_dim, widths, splices, post, spec, seed, log_softmax=False, bn_scales=(1.0, 2.0, -1.0)):
    """Layer list (formats.nnet_bytes' vocabulary) of an exact-integer net.
    widths: output width per Linear; splices: index list per Linear ([0]: no
    Splice); post: per Linear a tuple out of "relu" / "batchnorm" (at most 4,
    one BatchNorm: what the loader fuses); spec: per Linear (max |w|, nonzeros
    per column).  Weights are sparse integers, biases integers in [-64, 64],
    BatchNorm scales out of bn_scales with integer offsets in [-8, 8]."""
    rng = np.random.default_rng(seed)

    def linear(i, k, n):
        wmax, nnz = spec[i]
        nnz = min(nnz, k)
        W = np.zeros((k, n), np.float32)
        rows = rng.integers(0, k, size=(nnz, n))
        mag = rng.integers(1, wmax + 1, size=(nnz, n))
        sign = rng.integers(0, 2, size=(nnz, n)) * 2 - 1
        W[rows, np.arange(n)[None, :]] = (mag * sign).astype(np.float32)
        return {"kind": "linear", "W": W, "b": _ints(rng, -64, 64, n)}

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


def int_input(layers, rows, seed, amax=7):
    """rows + left + right input rows of integers in [-amax, amax]."""
    left, right = context(layers)
    return _ints(np.random.default_rng(seed), -amax, amax, (rows + left + right, in_dim(layers)))


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


def _walk(layers, x, visit=None):
    """fp64 evaluation.  Splice + Narrow together keep the rows whose every
    spliced row exists (the rows the reference's clamped Splice computes and
    its Narrow keeps).  visit(linear_layer, its_input) is called per Linear,
    visit(batchnorm_layer, its_input) per BatchNorm."""
    x = np.asarray(x, np.float64)
    i = 0
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
            x = x @ L["W"].astype(np.float64) + L["b"].astype(np.float64)
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


def check_exact_budget(layers, x, plane_max=None):
    """Raises AssertionError unless the net on input x is exact in fp32 in
    every summation order and under the bf16x6 split: integer operands; per
    Linear max_ij (sum_k |a_ik| |w_kj| + |b_j|) < 2^24 and (max |a| <= 255 or
    max |w| <= 255 or both <= 65535); per BatchNorm |x| |scale| + |offset| <
    2^24.  plane_max=2047: additionally every Linear's inputs and weights fit
    one fp16 plane (the f16x3 kernels, which drop the a1b1 product).
    Returns the log2 of each Linear's bound."""
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
        bound = (np.abs(a) @ np.abs(L["W"]).astype(np.float64) + np.abs(L["b"])).max()
        assert bound < EXACT_LIMIT, f"Linear bound 2^{np.log2(bound):.1f} >= 2^24"
        amax, wmax = np.abs(a).max(), np.abs(L["W"]).max()
        assert amax <= 255 or wmax <= 255 or (amax <= 65535 and wmax <= 65535), \
            f"bf16x6 would drop nonzero products: max |a| {amax}, max |w| {wmax}"
        if plane_max is not None:
            assert amax <= plane_max and wmax <= plane_max, f"max |a| {amax}, max |w| {wmax} > {plane_max}"
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
TWO_PLANE_GEOMS = ("A", "B", "C", "H") # also run with the TWO_PLANES recipe


def max_rows(geom):
    return BIG_ROWS if geom in BIG else ROWS[-1]


def exact_cases(geom):
    """[(name, layers, x)] of the exact-integer leg of one geometry: the WIDE
    recipe, its binade-shifted forms, the TWO_PLANES recipe.  x has
    max_rows(geom) + left + right rows; the first r + left + right of them
    give the first r output rows."""
    in_d, widths, splices, post = GEOMETRIES[geom]
    seed = 1000 + sorted(GEOMETRIES).index(geom)
    layers = int_net(in_d, widths, splices, post, WIDE, seed)
    x = int_input(layers, max_rows(geom), seed + 500)
    cases = [("wide", layers, x)]
    if geom in BINADE:
        for e in (60, -60):
            cases.append((f"wide*2^{e}",) + binade_shift(layers, x, e))
    if geom in TWO_PLANE_GEOMS:
        l2 = int_net(in_d, widths, splices, post, TWO_PLANES, seed + 1, bn_scales=(1.0, -1.0))
        cases.append(("two-planes", l2, int_input(l2, max_rows(geom), seed + 501, amax=1023)))
    return cases


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
