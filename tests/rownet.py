"""Nets with row steps of their own -- layers the loader cannot fuse into a
Linear's epilogue -- for tests/test_rownet.py and tests/test_gpu_row_ops.py,
and the row steps' definition restated in numpy float32.

A row step (ce_gpu_model_admit_row_ops, include/catears_gpu.h) is a function
of one fp32 row with rowop_kernel's arithmetic (kernels/rowops.hip): ReLU and
BatchNorm element-wise in the reference's rounding order; Normalize, Softmax
and LogSoftmax with their sum taken as lane l of 64 adding the columns
c = l (mod 64) in ascending order, then wave_sum's xor tree 32 down to 1;
Normalize's scale (float)sqrt((double)(float)dim / (double)s).  lane_sum and
row_op say that; walk evaluates a whole net with it.

Exact cases.  netgen's exact-integer recipe carries over to a net with row
steps as long as every row step keeps the integers (ReLU, BatchNorm with
integer parameters) -- or is a Normalize whose result no later sum can
reorder: on an integer row with sum x^2 < 2^24 the sum is exact in every
order, so the scale and every x * scale are one rounding each; a *selection*
Linear behind it (per column one nonzero weight +-2^e, an integer bias) forms
+-2^e x exactly, in any K order, in the bf16x6 planes (x is the exact sum of
its three planes, and every partial sum of them is a prefix of its mantissa)
and in split-K, and adds the bias with one rounding.  In the plain bf16 mode
the same holds with the Normalize output rounded once by bf16ref.rne_bf16
(every other operand of these nets is an integer of magnitude <= 255, which
bf16 holds).  tests/test_rownet.py proves it with the oracle in three GEMM
orders."""
import functools

import numpy as np

import netgen

ROWS = (1, 23, 70, 129, 300)
PDFS = 36
# small weights and activations: every Linear operand but a Normalize output
# is an integer of magnitude <= 255 (one bf16 plane)
SPEC = [(1, 3), (1, 2), (1, 2)]
BN_SCALES = (1.0, -1.0)


# ------------------------------------------------- the row steps, restated --

def lane_sum(terms):
    """Section-2 order of the sum of each row of `terms` (rows x dim float32):
    64 lane sums over the columns c = l (mod 64) ascending, then the xor tree
    32 .. 1 (v += shfl_xor(v, d): float addition commutes, so after the tree
    every lane holds the same bits).  Columns the kernel never adds are
    padded with +0 here: s + 0 is s for every s but -0, which a sum that
    starts at +0 never is."""
    t = np.ascontiguousarray(terms, np.float32)
    rows, dim = t.shape
    per = -(-dim // 64)
    pad = np.zeros((rows, per * 64), np.float32)
    pad[:, :dim] = t
    s = np.zeros((rows, 64), np.float32)
    for j in range(per):
        s = (s + pad[:, 64 * j:64 * (j + 1)]).astype(np.float32)
    lanes = np.arange(64)
    d = 32
    while d >= 1:
        s = (s + s[:, lanes ^ d]).astype(np.float32)
        d >>= 1
    assert np.array_equal(s.view(np.uint32), np.repeat(s[:, :1], 64, 1).view(np.uint32)) or np.isnan(s).any()
    return s[:, 0].copy()


def row_op(kind, x, scale=None, offset=None):
    """One row step on the rows of x (float32), every column of x a true
    column."""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(all="ignore"):
        if kind == "relu":
            return np.where(x < 0.0, np.float32(0.0), x).astype(np.float32)
        if kind == "batchnorm":
            v = (x * np.asarray(scale, np.float32)).astype(np.float32)
            return (v + np.asarray(offset, np.float32)).astype(np.float32)
        if kind == "normalize":
            s = lane_sum((x * x).astype(np.float32))
            sc = np.sqrt(np.float64(np.float32(x.shape[1])) / s.astype(np.float64)).astype(np.float32)
            return (x * sc[:, None]).astype(np.float32)
        if kind == "softmax":
            e = np.exp(x).astype(np.float32)
            return (e / lane_sum(e)[:, None]).astype(np.float32)
        if kind == "log_softmax":
            ls = np.log(lane_sum(np.exp(x).astype(np.float32))).astype(np.float32)
            return (x - ls[:, None]).astype(np.float32)
    raise ValueError(kind)


def walk(layers, x, rnd=None, acc=np.float64, k_reversed=False):
    """The net in float32 with every Linear's products summed in `acc` (K
    ascending or reversed) and every other layer as row_op has it; rnd (e.g.
    bf16ref.rne_bf16): the plain bf16 mode's definition, every Linear's
    operands rounded by it.  A final LogSoftmax is a row_op like any other."""
    x = np.asarray(x, np.float32)
    i = 0
    while i < len(layers):
        L = layers[i]
        k = L["kind"]
        if k == "splice":
            nar = layers[i + 1]
            idx, left, right = L["indices"], nar["left"], nar["right"]
            assert nar["kind"] == "narrow" and left == -min(min(idx), 0) and right == max(max(idx), 0)
            rows = x.shape[0] - left - right
            assert rows > 0, "input does not cover the context"
            x = np.concatenate([x[left + o:left + o + rows] for o in idx], axis=1)
            i += 1
        elif k == "narrow":
            assert L["left"] == 0 and L["right"] == 0
        elif k == "linear":
            a, w = (x, L["W"]) if rnd is None else (rnd(x), rnd(L["W"]))
            a, w = a.astype(acc), w.astype(acc)
            if k_reversed:
                a, w = np.ascontiguousarray(a[:, ::-1]), np.ascontiguousarray(w[::-1])
            x = ((a @ w).astype(np.float32) + L["b"].astype(np.float32)).astype(np.float32)
        else:
            x = row_op(k, x, L.get("scale"), L.get("offset"))
        i += 1
    return x


def eval_f64(layers, x):
    """Every operation in float64 (netgen.eval_f64 with the row layers)."""
    x = np.asarray(x, np.float64)
    i = 0
    while i < len(layers):
        L = layers[i]
        k = L["kind"]
        if k == "splice":
            idx, left = L["indices"], layers[i + 1]["left"]
            rows = x.shape[0] - left - layers[i + 1]["right"]
            x = np.concatenate([x[left + o:left + o + rows] for o in idx], axis=1)
            i += 1
        elif k == "linear":
            x = x @ L["W"].astype(np.float64) + L["b"].astype(np.float64)
        elif k == "relu":
            x = np.where(x < 0.0, 0.0, x)
        elif k == "batchnorm":
            x = x * L["scale"].astype(np.float64) + L["offset"].astype(np.float64)
        elif k == "normalize":
            x = x * np.sqrt(x.shape[1] / (x * x).sum(axis=1, keepdims=True))
        elif k in ("softmax", "log_softmax"):
            m = x.max(axis=1, keepdims=True)
            x = x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))
            if k == "softmax":
                x = np.exp(x)
        else:
            assert k == "narrow", k
        i += 1
    return x


# ------------------------------------------------------ what the loader does --

def steps(layers):
    """build_program's step list (csrc/model.cc): "gemm" per Linear, the kind
    of every layer that becomes a step of its own.  A ReLU / BatchNorm is
    fused while its Linear's chain is open: fewer than 4 post ops, no second
    BatchNorm, no row step yet.  A final LogSoftmax is the finalize."""
    out, npost, bn, open_ = [], 0, False, False
    for i, L in enumerate(layers):
        k = L["kind"]
        if k == "linear":
            out.append("gemm")
            npost, bn, open_ = 0, False, True
        elif k in ("relu", "batchnorm"):
            if open_ and npost < 4 and not (k == "batchnorm" and bn):
                npost += 1
                bn = bn or k == "batchnorm"
            else:
                out.append(k)
                open_ = False
        elif k in ("normalize", "softmax", "log_softmax"):
            if not (k == "log_softmax" and i + 1 == len(layers)):
                out.append(k)
            open_ = False
        elif k == "splice":
            open_ = False
    return out


def has_row_steps(layers):
    return any(s != "gemm" for s in steps(layers))


# ------------------------------------------------------------- exact cases --

def _int_bn(rng, n):
    return {"kind": "batchnorm", "scale": np.array(BN_SCALES, np.float32)[rng.integers(0, 2, size=n)],
            "offset": rng.integers(-8, 9, size=n).astype(np.float32)}


def _insert_after(layers, which, nth, new):
    """`new` behind the nth layer of kind `which`."""
    at = [i for i, L in enumerate(layers) if L["kind"] == which][nth]
    return layers[:at + 1] + list(new) + layers[at + 1:]


def selection_linear(rng, k, n):
    """Per column one nonzero weight +-2^e (e in -2 .. 3), integer bias."""
    W = np.zeros((k, n), np.float32)
    W[rng.integers(0, k, size=n), np.arange(n)] = (np.ldexp(1.0, rng.integers(-2, 4, size=n)) *
                                                  (rng.integers(0, 2, size=n) * 2 - 1)).astype(np.float32)
    return {"kind": "linear", "W": W, "b": rng.integers(-64, 65, size=n).astype(np.float32)}


def normalize_net(hidden, seed, splice=(-1, 0, 1), pdfs=PDFS, spec=SPEC):
    """integer Linear -> ReLU -> Normalize -> Splice -> selection Linear."""
    rng = np.random.default_rng(seed)
    head = netgen.int_net(40, [hidden], [netgen.S5], [("relu",)], spec, seed, bn_scales=BN_SCALES)
    return (head + [{"kind": "normalize"}] + netgen._splice_layers(list(splice)) +
            [selection_linear(rng, hidden * len(splice), pdfs)])


def _three(post0, seed):
    return netgen.int_net(40, [64, 96, PDFS], [netgen.S5, [-1, 0, 1], [0]], [post0, netgen.RB, ()], SPEC, seed,
                          bn_scales=BN_SCALES)


@functools.lru_cache(maxsize=None)
def exact_cases():
    """{name: (layers, x)}, x of ROWS[-1] + left + right integer rows; hidden
    widths 64 and 96, 36 pdfs."""
    rng = np.random.default_rng(8000)
    cases = {}
    # 1. five posts behind one Linear: ReLU, BN, ReLU, ReLU, ReLU -- the fifth is a row step
    cases["five-posts"] = _insert_after(_three(("relu", "batchnorm", "relu", "relu"), 8001), "relu", 2,
                                        [{"kind": "relu"}])
    # 2. a second BatchNorm behind one Linear (and a ReLU behind it: a row step too)
    cases["second-bn"] = _insert_after(_three(("batchnorm", "relu"), 8002), "relu", 0,
                                       [_int_bn(rng, 64), {"kind": "relu"}])
    # 3. a row step behind the last Linear
    cases["row-last"] = _three(netgen.RB, 8003) + [{"kind": "normalize"}]
    # 4. Normalize made exact, on both hidden widths
    cases["normalize-64"] = normalize_net(64, 8004)
    cases["normalize-96"] = normalize_net(96, 8005)
    out = {}
    for i, (name, layers) in enumerate(cases.items()):
        assert has_row_steps(layers), name
        x = netgen.int_input(layers, ROWS[-1], 8100 + i)
        x.setflags(write=False)
        out[name] = (layers, x)
    return out


@functools.lru_cache(maxsize=None)
def big_case():
    """Case 4 on a hidden width of 1024 at 1024 rows: at this size the bf16
    GEMM takes its 128 x 128 tile (bf16ref.tile) and the bf16x6 GEMM a
    direct-weight tile of the large-block family (netgen.kernels names it),
    each writing the fp32 hidden block a row step then reads."""
    layers = normalize_net(1024, 8006, splice=(0,), spec=[(1, 4)])
    x = netgen.int_input(layers, 1024, 8106)
    x.setflags(write=False)
    return layers, x


def integer_prefix(layers):
    """The layers up to the first Normalize (all of them if there is none):
    the part netgen.check_exact_budget speaks about."""
    at = [i for i, L in enumerate(layers) if L["kind"] == "normalize"]
    return layers[:at[0]] if at else layers


def check_exact(layers, x):
    """Asserts the recipe of the module docstring on input x; returns the
    rows (float32) every correct evaluation must give."""
    head = integer_prefix(layers)
    netgen.check_exact_budget(head, x)
    if len(head) < len(layers):
        rows = netgen.exact(head, x)
        ss = (rows.astype(np.float64) ** 2).sum(axis=1)
        assert ss.min() > 0 and ss.max() < netgen.EXACT_LIMIT, (ss.min(), ss.max())
        tail = [L for L in layers[len(head) + 1:] if L["kind"] == "linear"]
        assert len(tail) <= 1, "one selection Linear at most behind the Normalize"
        for L in tail:
            nz = L["W"] != 0
            assert np.all(nz.sum(axis=0) == 1) and np.all(np.abs(np.log2(np.abs(L["W"][nz]))) % 1 == 0)
            assert np.array_equal(L["b"], np.rint(L["b"]))

    def one_plane(a):  # every Linear operand but a Normalize output fits one bf16 plane
        assert np.abs(a).max() <= 255
    for i, L in enumerate(head):
        if L["kind"] == "linear":
            one_plane(L["W"])
            one_plane(walk(head[:i], x))
    return walk(layers, x)


# --------------------------------------------------------------- real nets --

def renorm_tdnn(hidden, pdfs):
    """synth.tdnn_layers with every BatchNorm replaced by Normalize: the
    relu-renorm TDNN.  (layers, left, right)."""
    from catears_amd import synth
    layers, left, right, _ = synth.tdnn_layers(hidden, pdfs)
    return [{"kind": "normalize"} if L["kind"] == "batchnorm" else L for L in layers], left, right


@functools.lru_cache(maxsize=None)
def pad_cases():
    """{name: (layers, x)}: exact nets of true hidden width 100 and 37 pdfs,
    outside the envelope by their widths and by a row step: padnet's P1 with
    the second BatchNorm of tests/test_gpu_pad_widths.py's refusal test, and
    case 4 on those widths."""
    import padnet
    in_d, widths, splices, post = padnet.GEOMETRIES["P1"]
    p1 = netgen.int_net(in_d, widths, splices, post, SPEC, 8201, bn_scales=BN_SCALES)
    bn = {"kind": "batchnorm", "scale": np.ones(100, np.float32), "offset": np.ones(100, np.float32)}
    cases = {"second-bn": _insert_after(p1, "batchnorm", 0, [bn]), "normalize": normalize_net(100, 8202, pdfs=37)}
    out = {}
    for i, (name, layers) in enumerate(cases.items()):
        assert has_row_steps(layers) and [g["n"] for g in netgen.linears(layers)][-1] == 37
        x = netgen.int_input(layers, ROWS[-1], 8300 + i)
        x.setflags(write=False)
        out[name] = (layers, x)
    return out
