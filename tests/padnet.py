"""ce_gpu_model_pad_widths restated on netgen layer lists (csrc/model.cc), and
the geometries of tests/test_padnet.py / tests/test_gpu_pad_widths.py.

pad_layers moves a net onto padded widths: every hidden Linear's output width
up to the next multiple of 32, the last one's to the next multiple of 4; a
later Linear reads the previous padded width, splice segment s keeping its
true rows of W at s * padded_width with zero rows behind them; a padded unit
has a zero weight column, a zero bias and, under a BatchNorm, scale 1 and
offset 0.  A padded unit's activation is +0 after any post chain and meets
only zero weights, so the padded net's first n output columns are the
original net's -- bit for bit on an exact-integer net, whatever the order of
the sums."""
import numpy as np

import netgen

# id -> (in_dim, widths, splices, post), none of them an x6 program as it is:
# P1 is netgen's E (hidden 100 -> 128, an odd last width, every layer's
#    segments narrower than a K-tile before the padding),
# P2 has C's 7-segment first layer and asymmetric 8-segment second layer on
#    widths that are multiples of 8 but not of 32, and an odd last width,
# P3 has D's shapes off the tile: 13-wide input (splice_pad), 780 -> 800 so
#    that a 3000-row block takes the 512 x 128 kernel, 104 -> 128, 1029 -> 1032,
# P4 is netgen's F4099: only the last width changes, 4099 -> 4100 > 4096.
GEOMETRIES = {
    "P1": netgen.GEOMETRIES["E"],
    "P2": (24, [72, 40, 101], netgen.GEOMETRIES["C"][2], netgen.GEOMETRIES["C"][3]),
    "P3": (13, [780, 104, 1029], [netgen.S5, [-1, 0, 1], [0]], [netgen.RB, ("relu",), netgen.RB]),
    "P4": netgen.GEOMETRIES["F4099"],
}
PADDED_WIDTHS = {"P1": [128, 128, 40], "P2": [96, 64, 104], "P3": [800, 128, 1032], "P4": [96, 640, 4100]}
BIG = ("P3",)  # also at netgen.BIG_ROWS rows
RECIPES = {"wide": (netgen.WIDE, (1.0, 2.0, -1.0), 7), "two-planes": (netgen.TWO_PLANES, (1.0, -1.0), 1023)}


def round_up(v, to):
    return (v + to - 1) // to * to


def max_rows(geom):
    return netgen.BIG_ROWS if geom in BIG else netgen.ROWS[-1]


def exact_cases(geom):
    """[(recipe, layers, x)]: the geometry as an exact-integer net under both
    of netgen's recipes, x of max_rows(geom) + left + right rows."""
    in_d, widths, splices, post = GEOMETRIES[geom]
    seed = 4000 + sorted(GEOMETRIES).index(geom)
    out = []
    for i, (name, (spec, bn_scales, amax)) in enumerate(sorted(RECIPES.items())):
        layers = netgen.int_net(in_d, widths, splices, post, spec, seed + i, bn_scales=bn_scales)
        out.append((name, layers, netgen.int_input(layers, max_rows(geom), seed + 500 + i, amax=amax)))
    return out


def pad_layers(layers):
    """The layer list of the padded net.  A final LogSoftmax runs over the
    true columns in the library, which a layer list cannot say: refused when
    the last width changes."""
    n_linear = sum(L["kind"] == "linear" for L in layers)
    out, segs, li, prev_true, prev_pad, cur_true, cur_pad = [], 1, 0, None, None, None, None
    for L in layers:
        kind = L["kind"]
        if kind == "splice":
            segs = len(L["indices"])
            out.append(L)
        elif kind == "linear":
            k, n = L["W"].shape
            din = k // segs
            assert li == 0 or din == prev_true, "a Linear's input is not the previous Linear's output"
            din_pad = din if li == 0 else prev_pad
            n_pad = round_up(n, 4 if li == n_linear - 1 else 32)
            W = np.zeros((segs * din_pad, n_pad), np.float32)
            for s in range(segs):
                W[s * din_pad:s * din_pad + din, :n] = L["W"][s * din:(s + 1) * din]
            b = np.zeros(n_pad, np.float32)
            b[:n] = L["b"]
            out.append({"kind": "linear", "W": W, "b": b})
            prev_true, prev_pad, cur_true, cur_pad, segs, li = n, n_pad, n, n_pad, 1, li + 1
        elif kind == "batchnorm":
            scale, offset = np.ones(cur_pad, np.float32), np.zeros(cur_pad, np.float32)
            scale[:cur_true], offset[:cur_true] = L["scale"], L["offset"]
            out.append({"kind": "batchnorm", "scale": scale, "offset": offset})
        elif kind == "log_softmax":
            assert cur_pad == cur_true, "LogSoftmax over a padded width"
            out.append(L)
        else:
            assert kind in ("relu", "narrow"), kind
            out.append(L)
    return out


def widths(layers):
    return [g["n"] for g in netgen.linears(layers)]


def pad_columns(layers):
    """Per Linear of the padded net of `layers`: a boolean mask over its
    (spliced) input columns, true at the pad columns."""
    true_n = [None] + widths(layers)[:-1]
    masks = []
    for g, t in zip(netgen.linears(pad_layers(layers)), true_n):
        m = np.zeros(g["k"], bool)
        if t is not None:
            m.reshape(g["nseg"], g["din"])[:, t:] = True
        masks.append(m)
    return masks


def kernels(layers, out_rows, mode):
    """netgen.kernels of the padded net of `layers`, with the one host choice
    that reads the true width: in latency mode the last layer's reduce is
    fused into the finalize only when that layer was not padded
    (run_steps_x6f: the fused kernel writes float4 chunks of rows as wide as
    the partials)."""
    names = netgen.kernels(pad_layers(layers), out_rows, mode)
    if mode == "latency" and widths(layers)[-1] % 4 != 0:
        names[-1] = names[-1].replace("+lat_finalize", "+lat_reduce")
    return names
