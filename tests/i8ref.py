"""The int8 nnet path off the TDNN shapes (tests/test_gpu_int8_shapes.py; the
CPU proofs are in tests/test_i8ref.py).

chunk_reference restates dynamic int8 -- LinearLayer as Quantize +
MatMat_U8U8F32 + bias with per-tensor activation parameters -- from
oracle/pyoracle.py's public pieces, over one or more padded blocks that share
the parameters: one block of nnet_propagate, or one packed chunk of
am_forward.  The Narrows are deferred (every block carries all its rows, as
the GPU does, and is cut once at the end), so "the rows the reference chain
holds" at a Linear is a row range of the carried block and the rule that picks
it can be exchanged for a wrong one: rule="all" folds every row, "swapped"
exchanges the left and right contexts.  A wrong rule's parameters are only
reported, never applied -- the activations stay the reference's -- and exist
nowhere but here.

paths restates the host's choices per Linear (csrc/model.cc quantize_weights;
csrc/nnet_programs.cc run_steps_i8, run_steps_i8_static; kernels/nnet_i8.hip launch_i8_quantize,
launch_i8_gemm; kernels/nnet_i8_lat.hip), so the CPU tests can assert that the
geometries reach every class of them.
"""
import functools

import numpy as np

import netgen
from netgen import BR, RB, RBR, S5
from test_int8_static import fold_range

ROWS = (1, 17, 70, 129, 257, 300)
S8 = [-7, -3, -1, 0, 2, 5, 9, 20]
K_ALIGN = 128          # i8_k_align: the int8 GEMM's K-tile, bytes
TILE_M, TILE_N = 256, 128   # gemm_i8_pipe_kernel<256, 128, ...>
LAT_MAX_ROWS = 280     # kI8LatMaxRows

# id -> (in_dim, widths, splices, post) in netgen's vocabulary.
I8_GEOMETRIES = {g: netgen.GEOMETRIES[g] for g in ("A", "C", "D", "E", "F4100", "F4099", "G20", "H")}
I8_GEOMETRIES.update({
    # 8 asymmetric segments of 128: the segment changes on every K-tile
    "I1": (40, [128, 256, 100], [S5, S8, [0]], [RB, BR, ()]),
    # segments of two K-tiles, three full column tiles, then 33 ragged ones on
    # the scalar epilogue
    "I2": (40, [256, 384, 4099], [S5, [-1, 0, 2], [0]], [RB, RBR, ("batchnorm",)]),
    # a hidden width that is no multiple of 4
    "I3": (24, [130, 36], [[-3, -2, -1, 0, 1, 2, 3], [0]], [("relu",), ()]),
    # a first layer gathered in the loader (through row_map in am_forward),
    # asymmetric; one segment of 128; three asymmetric segments of 128; eight
    # asymmetric segments of 256 (16 K-tiles)
    "I4": (128, [128, 128, 256, 100], [[-4, -1, 0, 1], [0], [-1, 0, 2], S8],
           [(), ("relu",), ("batchnorm",), BR]),
    # a second BatchNorm and a ReLU behind the middle Linear run as row ops of
    # their own (ROW_OPS), between two Linears
    "I5": (40, [128, 128, 97], [S5, [0], [-1, 0, 1]], [RB, RB, ()]),
    # odd K-tile counts, widths ragged against the tile with n % 4 == 0
    "I6": (40, [132, 516, 96], [S5, [-2, 0, 1], [0]], [BR, (), ("relu",)]),
})
# geometry -> (Linear index, kinds) of stand-alone row ops behind that Linear
ROW_OPS = {"I5": (1, ("batchnorm", "relu"))}

# what every kept CATEARS_I8_GEMM variant of the experiments library scores
# (tests/test_gpu_i8_variants.py; test_i8ref.py shows what these reach)
VARIANT_GEOMS, VARIANT_ROWS = ("I1", "I3"), (70, 300)

HELD = ("A", "C", "E", "I1", "I3", "I4", "I5")     # the held-row tests' geometries
FINALIZE = ("F4100", "F4099", "I2")                # with a LogSoftmax and a prior


def seed_of(geom):
    # H joined after the others: it takes the seed behind theirs, so none moves
    return 3000 + (sorted(g for g in I8_GEOMETRIES if g != "H") + ["H"]).index(geom)


@functools.lru_cache(maxsize=None)
def net(geom):
    """Real-valued layers of a geometry, no LogSoftmax (a test that wants one
    appends it)."""
    in_d, widths, splices, post = I8_GEOMETRIES[geom]
    layers = netgen.real_net(in_d, widths, splices, post, seed_of(geom), log_softmax=False)
    if geom in ROW_OPS:
        after, kinds = ROW_OPS[geom]
        lin = [i for i, L in enumerate(layers) if L["kind"] == "linear"]
        at = lin[after + 1] if after + 1 < len(lin) else len(layers)
        while layers[at - 1]["kind"] in ("splice", "narrow"):
            at -= 1
        bn = next(L for L in layers[lin[after]:at] if L["kind"] == "batchnorm")
        extra = []
        for kind in kinds:
            extra.append({"kind": "relu"} if kind == "relu" else
                         {"kind": "batchnorm", "scale": (bn["scale"] * np.float32(0.75)).astype(np.float32),
                          "offset": (bn["offset"] - np.float32(0.25)).astype(np.float32)})
        layers = layers[:at] + extra + layers[at:]
    return layers


# ------------------------------------------------------------------ inputs --

def edge_input(layers, rows, seed, left=1.0, right=1.0, nleft=None, nright=None):
    """netgen.real_input with the first nleft rows scaled by `left` and the
    last nright rows by `right` (default: the net's whole left / right
    context): rows that only the early layers hold."""
    x = netgen.real_input(layers, rows, seed)
    L, R = netgen.context(layers)
    nleft, nright = L if nleft is None else nleft, R if nright is None else nright
    if nleft:
        x[:nleft] *= np.float32(left)
    if nright:
        x[len(x) - nright:] *= np.float32(right)
    return x


def held_inputs(geom, rows=70, factor=32.0):
    """[(name, x)] of the held-row tests: per Linear after the first, one
    block whose first in_left rows are scaled and one whose last in_right
    rows are -- the rows that Linear's fold must leave out, and little else."""
    layers = net(geom)
    seed = 5000 + seed_of(geom)
    out, seen = [], set()
    for left, right in contexts(layers)[1:]:
        for side, n in (("L", left), ("R", right)):
            if n and (side, n) not in seen:
                seen.add((side, n))
                kw = dict(left=factor, nleft=n) if side == "L" else dict(right=factor, nright=n)
                out.append((f"{side}{n}", edge_input(layers, rows, seed, **kw)))
    return out


def utterances(layers, lengths, seed, first=1.0, last=1.0, scales=None):
    """Unpadded utterances (frames x in_dim) ~ N(0, 3), utterance u scaled by
    scales[u], its first frame by `first` and its last by `last`: the frames
    am_forward replicates into the context."""
    rng = np.random.default_rng(seed)
    out = []
    for u, t in enumerate(lengths):
        x = rng.normal(0.0, 3.0, size=(t, netgen.in_dim(layers))).astype(np.float32)
        if scales is not None:
            x *= np.float32(scales[u])
        x[0] *= np.float32(first)
        x[-1] *= np.float32(last)   # a 1-frame utterance takes both factors
        out.append(x)
    return out


def padded(layers, utt):
    """The block am_forward forms of one utterance: left copies of the first
    frame, the frames, right copies of the last."""
    L, R = netgen.context(layers)
    return np.concatenate([np.repeat(utt[:1], L, 0), utt, np.repeat(utt[-1:], R, 0)], 0)


def frames_to_samples(frames):
    return 400 + 160 * (frames - 1)


# one packed chunk of am_forward: utterances of 1 and 3 frames (shorter than
# every context here) among longer ones, each at a scale of its own (so the
# chunk's parameters are not any single utterance's), the short ones small
# (all their rows are held rows: large, they would hide the others' edges)
CHUNK_LENGTHS = (1, 3, 70, 33, 150)
CHUNK_SCALES = (0.25, 0.5, 1.0, 4.0, 0.5)
CHUNK = ("A", "C", "E", "I1", "I3", "I4", "I5")
# I4's last splice is so wide (context 12 + 23) that, padded by replication,
# a block's non-held rows are copies of held ones at every Linear: no input
# of am_forward can tell the rules apart there (it is in CHUNK for its first
# layer, gathered through the row map)
CHUNK_SHARP = tuple(g for g in CHUNK if g != "I4")


def chunk_inputs(geom):
    """[(name, utterances)]: first frames scaled, last frames scaled."""
    layers = net(geom)
    return [(f"first*{a}/last*{b}", utterances(layers, CHUNK_LENGTHS, 7000 + seed_of(geom), first=a, last=b,
                                                scales=CHUNK_SCALES)) for a, b in ((32, 1), (1, 32))]


def calib_case():
    """(layers, {name: integer utterances}) for ce_gpu_model_calibrate:
    geometry A (its last Linear's contexts are 3 / 4) as an exact-integer net,
    utterances of 1, 3, 37, 64 and 20 frames in [-7, 7] with the longer ones'
    first (or last) frame times 4 -- every block inside
    netgen.check_exact_budget, which the caller asserts."""
    in_d, widths, splices, post = netgen.GEOMETRIES["A"]
    layers = netgen.int_net(in_d, widths, splices, post, netgen.WIDE, 1000)
    rng = np.random.default_rng(1501)
    base = [rng.integers(-7, 8, size=(t, in_d)).astype(np.float32) for t in (1, 3, 37, 64, 20)]
    cases = {}
    for name, (a, b) in (("first*4", (4, 1)), ("last*4", (1, 4))):
        us = [u.copy() for u in base]
        for u in us[2:]:
            u[0] *= a
            u[-1] *= b
        cases[name] = us
    return layers, cases


# --------------------------------------------------------------- reference --

def f64_gemm_ok(k, z, zw):
    """static_oracle's guard: the float64 GEMM equals the int32 ring while no
    accumulator can wrap and both zero points are bytes."""
    return k * (255 + abs(z)) * (255 + abs(zw)) < 2 ** 31 and 0 <= z <= 255 and 0 <= zw <= 255


def held_rows(n, left, right, rule):
    """Row range of an n-row carried block that the fold reads."""
    if rule == "all":
        return 0, n
    if rule == "swapped":
        left, right = right, left
    assert rule in ("reference", "swapped"), rule
    return left, n - right


def chunk_reference(oracle, layers, blocks, rule="reference", exact_f64=True, log=None):
    """Dynamic int8 over padded blocks sharing per-tensor parameters.
    Returns (outputs per block, (num_linear, 2) ranges, [(scale, zp)]): the
    ranges and parameters under `rule`, the outputs always the reference's.
    log: list that receives per Linear dict(k, z, zw, f64)."""
    xs = [np.ascontiguousarray(b, np.float32) for b in blocks]
    left = right = 0          # rows the Narrows so far would have dropped
    pre = None                # (blocks, left, right) entering the pending Splice
    ranges, params = [], []
    for layer in layers:
        kind = layer["kind"]
        if kind == "splice":
            pre = (xs, left, right)
            xs = [oracle.layer_forward(layer, x) for x in xs]
        elif kind == "narrow":
            left, right = left + layer["left"], right + layer["right"]
        elif kind == "linear":
            src, sl, sr = pre if pre is not None else (xs, left, right)
            pre = None

            def fold(r):
                mn, mx = fold_range(np.concatenate([b[slice(*held_rows(len(b), sl, sr, r))] for b in src]))
                return mn, mx, oracle.quantize(np.float32([mn, mx]))[1:]

            _, _, (s, z) = fold("reference")
            mn, mx, qp = fold(rule)
            ranges.append((mn, mx))
            params.append(qp)
            wq, sw, zw = oracle.quantize(layer["W"])
            f64 = exact_f64 and f64_gemm_ok(layer["W"].shape[0], z, zw)
            if log is not None:
                log.append(dict(k=layer["W"].shape[0], z=z, zw=zw, f64=f64))
            gemm = oracle.gemm_u8u8f32_f64 if f64 else oracle.gemm_u8u8f32
            bias = np.asarray(layer["b"], np.float32)[None, :]
            xs = [(gemm(oracle._quantize_with(x, s, z), s, z, wq, sw, zw) + bias).astype(np.float32) for x in xs]
        else:
            xs = [oracle.layer_forward(layer, x) for x in xs]
    assert pre is None
    return [x[left:len(x) - right] for x in xs], np.array(ranges, np.float32).reshape(-1, 2), params


def fp32_held_ranges(oracle, layers, blocks, rule="reference"):
    """(num_linear, 2): what ce_gpu_model_calibrate measures -- the range of
    every Linear's input over the rows the reference chain holds there, all
    blocks folded together -- in an fp32 forward with the Narrows deferred
    (Linear as a float64 product rounded once: exact for an integer net inside
    netgen.check_exact_budget)."""
    xs = [np.ascontiguousarray(b, np.float32) for b in blocks]
    left = right = 0
    pre = None
    out = []
    for layer in layers:
        kind = layer["kind"]
        if kind == "splice":
            pre = (xs, left, right)
            xs = [oracle.layer_forward(layer, x) for x in xs]
        elif kind == "narrow":
            left, right = left + layer["left"], right + layer["right"]
        elif kind == "linear":
            src, sl, sr = pre if pre is not None else (xs, left, right)
            pre = None
            out.append(fold_range(np.concatenate([b[slice(*held_rows(len(b), sl, sr, rule))] for b in src])))
            W, b = layer["W"].astype(np.float64), layer["b"].astype(np.float64)
            xs = [(x.astype(np.float64) @ W + b).astype(np.float32) for x in xs]
        else:
            xs = [oracle.layer_forward(layer, x) for x in xs]
    return np.array(out, np.float32).reshape(-1, 2)


def block_input(geom, rows):
    """The block of `rows` output rows the one-block tests score."""
    return netgen.real_input(net(geom), rows, seed_of(geom) + 100 + rows)


def calibration_input(geom):
    """The static tests' ranges are test_int8_static.fp32_ranges of this
    block: another input than any they score."""
    return netgen.real_input(net(geom), 300, 9000 + seed_of(geom))


def latency_rows(geom):
    """Output rows whose blocks have kI8LatMaxRows and kI8LatMaxRows + 1 rows:
    the last row count of the split-K pair and the first of the throughput
    kernel."""
    ctx = sum(netgen.context(net(geom)))
    return LAT_MAX_ROWS - ctx, LAT_MAX_ROWS + 1 - ctx


# With the ranges shrunk to their central half every Linear's bytes hold 0,
# 255 and interior values at 129 rows -- but for C's last Linear, whose input
# stays below the top: its block is scored at twice the scale.
CLAMP_ROWS = 129
CLAMP_SCALE = {"C": 2.0}


def clamp_input(geom):
    return (block_input(geom, CLAMP_ROWS) * np.float32(CLAMP_SCALE.get(geom, 1.0))).astype(np.float32)


_REFERENCE = {}


def reference(oracle, geom, rows):
    """(x, dynamic int8 output) of block_input, computed once; the output is
    read-only."""
    if (geom, rows) not in _REFERENCE:
        x = block_input(geom, rows)
        (want,), _, _ = chunk_reference(oracle, net(geom), [x])
        want.setflags(write=False)
        _REFERENCE[geom, rows] = (x, want)
    return _REFERENCE[geom, rows]


def contexts(layers):
    """Per Linear (in_left, in_right): what the Narrows ahead of the block its
    parameters are folded over have dropped (GemmLayer::in_left / in_right)."""
    out, left, right, pend = [], 0, 0, None
    for L in layers:
        if L["kind"] == "splice":
            pend = (left, right)
        elif L["kind"] == "narrow":
            left, right = left + L["left"], right + L["right"]
        elif L["kind"] == "linear":
            out.append(pend if pend is not None else (left, right))
            pend = None
    return out


# --------------------------------------------------- the dispatch, restated --

def post_mode(ops):
    """internal.h post_mode()."""
    return {(): "none", ("relu",): "relu", ("batchnorm",): "bn", RB: "relu+bn", BR: "bn+relu"}.get(tuple(ops), "generic")


def steps(layers):
    """build_program's steps: per Linear dict(din, nseg, off, k, n, post,
    row_ops) -- post the fused ops, row_ops the stand-alone ones behind it."""
    out = netgen.linears(layers)
    cur, open_ = -1, False
    for L in layers:
        kind = L["kind"]
        if kind == "linear":
            cur += 1
            out[cur].update(post=[], row_ops=[])
            open_ = True
        elif kind in ("relu", "batchnorm"):
            g = out[cur]
            if open_ and len(g["post"]) < 4 and not (kind == "batchnorm" and "batchnorm" in g["post"]):
                g["post"].append(kind)
            else:
                g["row_ops"].append(kind)
                open_ = False
        elif kind == "splice":
            open_ = False
    return out


def paths(layers, out_rows, form, row_map=False):
    """Per Linear what the host runs on a block of out_rows output rows (the
    GEMMs see out_rows + left + right rows); form: dynamic, static,
    static-latency.  row_map: the first layer reads the caller's rows through
    a row map (am_forward, calibrate)."""
    from catears_amd import gpu
    assert form in ("dynamic", "static", "static-latency"), form
    left, right = netgen.context(layers)
    m = out_rows + left + right
    st = steps(layers)
    max_width = max(g["n"] for g in st)
    out = []
    cur = 0                   # which half of the fp32 workspace the GEMM writes
    have_bytes = False        # static: the previous epilogue wrote this layer's bytes
    fused_mm = False          # dynamic: the previous epilogue reduced this layer's min / max
    ldx = netgen.in_dim(layers)
    for i, g in enumerate(st):
        kpad = (g["k"] + K_ALIGN - 1) // K_ALIGN * K_ALIGN
        spliced = g["din"] % K_ALIGN != 0
        p = dict(linear=i, n=g["n"], post=post_mode(g["post"]), row_ops=list(g["row_ops"]), ktiles=kpad // K_ALIGN,
                 tiles_n=(g["n"] + TILE_N - 1) // TILE_N, tiles_m=(m + TILE_M - 1) // TILE_M, width=g["din"])
        if spliced:   # the quantize pass writes the spliced operand; the loader reads one segment
            p.update(operand="spliced", nseg=1, off=[0], din=kpad, q_nseg=g["nseg"], q_off=list(g["off"]))
        else:
            p.update(operand="gathered", nseg=g["nseg"], off=list(g["off"]), din=g["din"], q_nseg=1, q_off=[0])
        # launch_i8_gemm's LDS-DMA branch: anything else would be the fallback kernel
        lda = kpad if spliced else g["din"]
        p["fallback_gemm"] = not (kpad % 128 == 0 and p["din"] % 128 == 0 and lda % 16 == 0)
        vec_in = g["din"] % 4 == 0 and ldx % 4 == 0
        if have_bytes:
            p["quantize"] = "none"
        elif p["q_nseg"] == 1 and not (row_map and i == 0) and p["q_off"][0] == 0 and vec_in:
            p["quantize"] = "fast"
        else:
            p["quantize"] = "general-vector" if vec_in else "general-scalar"
        if form == "dynamic":
            p["minmax"] = "fused" if fused_mm else ("vector" if vec_in else "scalar")
        last = i + 1 == len(st)
        nxt = None if last or g["row_ops"] else st[i + 1]
        requant = form != "dynamic" and nxt is not None and g["n"] % 128 == 0
        p["unfused_because"] = []
        if form != "dynamic" and not last and not requant:
            if g["row_ops"]:
                p["unfused_because"].append("row op")
            else:
                p["unfused_because"] += ["n % 128", "next spliced"]   # one condition: the next din is this n
        aligned = cur == 0 or (m * max_width) % 4 == 0
        p["epilogue"] = "requantize" if requant else ("vector" if g["n"] % 4 == 0 and aligned else "scalar")
        p["fused_minmax"] = form == "dynamic" and nxt is not None
        if form == "static-latency":
            p["slices"] = gpu.i8_latency_plan(kpad, g["n"], m)
        if not requant:
            cur ^= 1
        have_bytes, fused_mm = requant, p["fused_minmax"]
        ldx = g["n"]
        out.append(p)
    return out
