"""The row counts at which the nnet kernels change what they do, shared by
tests/test_rowseams.py (the CPU proofs) and tests/test_gpu_row_seams.py.

Every GEMM of a block runs on m = output rows + left + right context rows.
A kernel tiles those rows (FAMILIES: row tile, rows per wave, rows per MFMA
step), masks the last tile, and the host picks the kernel from m: the
512 x 128 rule (x6w_fits), the plain-bf16 tile rule (bf16_small_tile), the
latency mode's frame tiles, 1024-row windows and fused last reduce, the
int8 latency limit.  seam_rows() derives from these constants -- each
restated once below, with the file and symbol it restates;
tests/test_rowseams.py reads them back from the sources -- the counts that
sit on every edge: the residues of m that mask a different part of the last
tile, both sides of every switch, and the first full tile behind a switch.

rows_written() and dispatch() are the models the proofs run on: which rows a
family's tile loop produces, and which kernel the host picks, with a short
list of one-character mistakes (MISTAKES).  Each mistake is visible at some
count of seam_rows and at none the suite presented before (old_rows: netgen's
case_rows and i8ref.ROWS plus the nets' contexts, the row blocks of 70 / 33 /
151 and the int8 latency pair 280 / 281).  Slips those counts already show
are not in the list: a wave or 16-row fragment skipped when it is not full
(row0 + rows > m for row0 >= m: every count off a multiple shows it, m = 8
among them), > for >= in x6w_fits and the m % tile slip on the latency mode's
64-row tile (FAMILY_MISTAKES says why).  One more count existed before and
is left out of old_rows on purpose, as the two window tests are not row
sweeps: B's 65 536-row first window (fp32 and bf16x6: f32_glds, x6d_256x128),
a whole number of every tile.
"""
import numpy as np

import bf16ref
import netgen

# family -> (row tile, rows per wave, rows per residue step), restated from
#   gemm_bf16x6_kernels.h  X6D128 = X6Cfg<128, 128, 2, 4, 2>  (BF 128 over WGF 4 waves)
#                          X6D256 = X6Cfg<kX6DirUnits, 128, 4, 2, 2>, X6W512 = W6Cfg<512, 128, 4, 2>
#   kernels/gemm_bf16x6.hip  Q = X6Cfg<128, 128, 4, 2, 3>
#   kernels/gemm_f32.hip   V2 = Cfg<128, 64, 32, 2, 2> (LDS-DMA), V3 = Cfg<64, 128, 32, 2, 2> (pipe2)
#   kernels/gemm_bf16.hip  B16Cfg<32, 32, 2, 1, 4> / B16Cfg<128, 128, 4, 2, 3>
#   kernels/gemm_f16x3.hip X3Cfg<128, 128, 2, 4, 2, 64> / <128, 128, 2, 4, 3, 32>
#   kernels/nnet_i8.hip    ProductTile = I8Tile<256, 128, 4, 2>
#   kernels/nnet_i8_lat.hip kRT = 6 sub-tiles of 16 rows (kBM = 96), every wave on all of them
# The step is 32 rows on the 64-row waves (two 16-row fragments, the MFMA
# step of the fp32 and int8 kernels) and the 16-row fragment on the small
# tiles.
FAMILIES = {
    "x6d_128x128": (128, 32, 32),
    "x6d_256x128": (128, 64, 32),
    "x6w_512x128": (128, 64, 32),
    "x6q_128x128": (128, 64, 32),
    "f32_glds": (128, 64, 32),
    "f32_pipe2": (64, 32, 32),
    "b16_32x32": (32, 32, 16),
    "b16_128x128": (128, 64, 32),
    "x3_128x128": (128, 32, 32),
    "i8_256x128": (256, 64, 32),
    "i8_lat": (96, 96, 16),
    "lat_gemm": (64, 64, 16),     # beyond LAT_TILE_LIMITS; the tiles below are LAT_TILES
}
X6_WIDE_MIN_TILES = 48            # gemm_bf16x6_kernels.h kX6WideMinTiles
X6_WIDE_UNITS = 512               # X6W512::BW
X6_LAT_WINDOW = 1024              # internal.h kX6LatWindow
LAT_TILE_LIMITS = (32, 80)        # gemm_bf16x6_lat.hip launch_gemm_bf16x6_lat: p.rows <= 32, <= 80
LAT_TILES = (32, 80, 64)          # launch_lat_gemm<2>, <5>, <4>: 16 TF rows
B16_LARGE_MIN_TILES = 64          # internal.h kB16LargeMinTiles
I8_LAT_MAX_ROWS = 280             # internal.h kI8LatMaxRows
ROW_KERNEL_ROWS = 4               # rowops.hip / nnet_i8.hip / quant.hip: dim3((rows + 3) / 4)
CAP = 3100                        # no seam of the committed nets lies beyond it

MODES = ("fp32", "bf16x6", "bf16x6p", "wide", "latency")
OTHER_MODES = ("bf16", "f16x3", "int8", "int8-latency", "int8-dynamic")

assert bf16ref.LARGE_MIN_TILES == B16_LARGE_MIN_TILES


def residues(tile, step):
    """m mod tile at which the last tile is full, one row, one short of full,
    or ends on / one row either side of a step inside it."""
    out = {0, 1, tile - 1}
    for e in range(step, tile, step):
        out |= {e - 1, e, e + 1}
    return sorted(out)


def tile_counts(family, after=0, tiles=2):
    """The counts behind `after` rows (a multiple of the tile: where the
    family takes over) whose residue is in residues(), over `tiles` tiles and
    one row more."""
    tile, _, step = FAMILIES[family]
    assert after % tile == 0
    res = set(residues(tile, step))
    return {m for m in range(after + 1, after + tiles * tile + 2) if m % tile in res}


# ------------------------------------------------------ the dispatch rules --

def x6w_switch(n):
    """The last m on 256 x 128 tiles for an n-wide layer the 512 x 128 kernel
    can run (x6w_fits), or None."""
    tiles_n = (n + X6_WIDE_UNITS - 1) // X6_WIDE_UNITS
    if (n + 255) // 256 * 256 < tiles_n * X6_WIDE_UNITS:
        return None
    tiles_m = (X6_WIDE_MIN_TILES + tiles_n - 1) // tiles_n
    return (tiles_m - 1) * 128


def b16_switch(n):
    """The last m on 32 x 32 tiles (bf16_small_tile)."""
    tiles_n = (n + 127) // 128
    return ((B16_LARGE_MIN_TILES + tiles_n - 1) // tiles_n - 1) * 128


def lat_plan(m, mistake=None):
    """launch_gemm_bf16x6_lat's loop: [(first row, rows, frame tile)] per
    window."""
    out = []
    lo, hi = LAT_TILE_LIMITS
    for r0 in range(0, m, X6_LAT_WINDOW):
        rows = min(X6_LAT_WINDOW, m - r0)
        if mistake == "window_rows_mod" and m - r0 <= X6_LAT_WINDOW:
            rows = (m - r0) % X6_LAT_WINDOW
        small = rows < lo if mistake == "lat_tile_lt" else rows <= lo
        mid = rows < hi if mistake == "lat_tile_lt" else rows <= hi
        out.append((r0, rows, LAT_TILES[0] if small else LAT_TILES[1] if mid else LAT_TILES[2]))
    return out


def lat_fused(m, n, mistake=None):
    """Whether the last layer's reduce runs inside lat_finalize."""
    one_window = m < X6_LAT_WINDOW if mistake == "fused_tail_lt" else m <= X6_LAT_WINDOW
    return one_window and n % 4 == 0 and n <= 4096


def i8_kpad(g):
    return (g["k"] + 127) // 128 * 128


def dispatch(layers, m, mode, mistake=None):
    """Per Linear the kernel `mode` runs on a block of m GEMM rows, by name:
    netgen.kernels / bf16ref.tiles / the int8 latency plan, with what those
    leave out because it does not change a result -- the latency mode's
    windows and frame tiles.  mistake: one of MISTAKES' dispatch slips."""
    c = sum(netgen.context(layers))
    r = m - c
    assert r >= 1, (m, c)
    lin = netgen.linears(layers)
    if mode in MODES:
        names = netgen.kernels(layers, r, mode)
        if not netgen.x6_ok(layers):
            return names
        if mode == "latency":
            plan = ",".join(f"{rows}/{tile}" for _, rows, tile in lat_plan(m, mistake))
            tail = "lat_finalize" if lat_fused(m, lin[-1]["n"], mistake) else "lat_reduce"
            names = [k + f"@[{plan}]" for k in names]
            names[-1] = names[-1].replace("+lat_finalize", "+" + tail).replace("+lat_reduce", "+" + tail)
        return names
    if mode == "bf16":
        out = []
        for shape, kt, n in bf16ref.tiles(layers, r):
            t = b16_switch(n)
            if mistake == "dispatch_gt" and t < m <= t + 128:
                shape = "b16_32x32"
            out.append(f"{shape}[kt={kt}]")
        return out
    if mode == "f16x3":
        return netgen.f16x3_kernels(layers)
    if mode in ("int8", "int8-dynamic"):
        return [f"i8_256x128[tiles_m={(m + 255) // 256}]" for _ in lin]
    assert mode == "int8-latency", mode
    from catears_amd import gpu
    out = []
    for g in lin:
        slices, per = gpu.i8_latency_plan(i8_kpad(g), g["n"], m)
        out.append(f"i8_lat[{slices}x{per}]" if slices else f"i8_256x128[tiles_m={(m + 255) // 256}]")
    return out


def families_at(layers, m, mode):
    """The FAMILIES keys dispatch()'s kernels belong to."""
    out = set()
    for k in dispatch(layers, m, mode):
        if "lat_gemm" in k:
            out.add("lat_gemm")
        elif "f32_" in k:
            out.add("f32_glds" if "f32_glds" in k else "f32_pipe2")
        elif "x3<" in k:
            out.add("x3_128x128")
        else:
            out |= {f for f in FAMILIES if f + "[" in k or f + "_gather[" in k}
    return out


def switches(layers, mode):
    """[(m, m + 1, what)]: the pairs of counts between which some Linear of
    the net changes kernel in `mode`, up to CAP."""
    lin = netgen.linears(layers)
    out = []
    if not netgen.x6_ok(layers) and mode in MODES + ("bf16", "f16x3"):
        return out
    if mode == "bf16x6":
        for i, g in enumerate(lin):
            first = i == 0 and g["din"] % 8 == 0 and g["din"] % 32 != 0
            t = x6w_switch(g["n"])
            if t is not None and not first:
                out.append((t, t + 1, f"Linear {i}: 512 x 128 from {X6_WIDE_MIN_TILES} tiles"))
    elif mode == "bf16":
        for i, g in enumerate(lin):
            out.append((b16_switch(g["n"]), b16_switch(g["n"]) + 1, f"Linear {i}: 128 x 128 tiles"))
    elif mode == "latency":
        for base in (0, X6_LAT_WINDOW):
            out += [(base + t, base + t + 1, f"frame tile beyond {t} rows") for t in LAT_TILE_LIMITS]
        out += [(w, w + 1, f"{w // X6_LAT_WINDOW + 1} windows") for w in (X6_LAT_WINDOW, 2 * X6_LAT_WINDOW)]
    elif mode == "int8-latency":
        out.append((I8_LAT_MAX_ROWS, I8_LAT_MAX_ROWS + 1, "the throughput kernel"))
    return sorted({s for s in out if s[1] <= CAP})


def seam_rows(layers, mode):
    """The sorted GEMM row counts m to present for the net in `mode`: per
    family its Linears run in, the residues over its first two row tiles (a
    family that takes over at a switch: over the tile behind the switch,
    whose last count is that tile exactly full, and one row more); both sides
    of every switch.  m - context is the output row count."""
    c = sum(netgen.context(layers))
    lin = netgen.linears(layers)
    ok = netgen.x6_ok(layers)
    out = set()
    for lo, hi, _ in switches(layers, mode):
        out |= {lo, hi}
    if mode == "fp32" or (mode in MODES and not ok):
        out |= tile_counts("f32_glds")
    elif mode == "bf16x6":
        for i, g in enumerate(lin):
            first = i == 0 and g["din"] % 8 == 0 and g["din"] % 32 != 0
            out |= tile_counts("x6d_128x128" if first else "x6d_256x128")
            t = x6w_switch(g["n"])
            if t is not None and not first and t < CAP:
                out |= tile_counts("x6w_512x128", after=t, tiles=1)
    elif mode == "bf16x6p":
        out |= tile_counts("x6q_128x128")
    elif mode == "wide":
        out |= tile_counts("x6d_128x128")
    elif mode == "latency":
        out |= tile_counts("lat_gemm")
        # the same residues behind each window seam: the short last window
        # runs the small frame tiles again
        for w in (X6_LAT_WINDOW, 2 * X6_LAT_WINDOW):
            out |= {w - 1, w, w + 1}
        out |= {X6_LAT_WINDOW + m for m in tile_counts("lat_gemm", tiles=1)}
    elif mode == "bf16":
        out |= tile_counts("b16_32x32")
        for g in lin:
            if b16_switch(g["n"]) < CAP:
                out |= tile_counts("b16_128x128", after=b16_switch(g["n"]), tiles=1)
    elif mode == "f16x3":
        out |= tile_counts("x3_128x128")
    elif mode == "int8":
        out |= tile_counts("i8_256x128")
    elif mode == "int8-latency":
        out |= tile_counts("i8_lat") | {m for m in tile_counts("i8_256x128") if m > I8_LAT_MAX_ROWS}
    elif mode == "int8-dynamic":
        out |= {t + d for t in (256, 512) for d in (-1, 0, 1)}
    else:
        raise ValueError(mode)
    return sorted(m for m in out if c + 1 <= m <= CAP)


def row_kernel_rows(tile=128):
    """Residues 0 .. 3 mod ROW_KERNEL_ROWS next to the first two row-tile
    seams: the row kernels' last block holds 1, 2, 3 or 4 rows."""
    return sorted({t + d for t in (tile, 2 * tile) for d in range(-2, ROW_KERNEL_ROWS - 2)})


def old_rows(layers, name="wide", geom=None, int8=False):
    """The GEMM row counts the suite presented for a net before the seam
    tests: case_rows (i8ref.ROWS and the latency pair for the int8 nets),
    the blocks of 70 / 33 / 151 rows and the 71-row block, plus context."""
    import i8ref
    c = sum(netgen.context(layers))
    rows = set(i8ref.ROWS if int8 else netgen.case_rows(geom, name) if geom else netgen.ROWS) | {70, 71, 33, 151}
    out = {r + c for r in rows}
    if int8:
        out |= {I8_LAT_MAX_ROWS, I8_LAT_MAX_ROWS + 1}
    return sorted(out)


# --------------------------------------------------------- mutation model --
# name -> (kind, what the slip is).  "rows": rows_written shows it; "dispatch":
# dispatch() names another kernel.
MISTAKES = {
    "tile_tail_mod": ("rows", "the last tile's row count taken as m % tile: nothing when the tile is full"),
    # the 64-row frame tile is not in it: every whole window of the 3007-row
    # blocks of before is a whole number of those
    "lat_small_tail_mod": ("rows", "tile_tail_mod on the 32- and 80-row frame tiles of the latency mode"),
    "window_rows_mod": ("rows", "the last window's rows as (m - r0) % window: nothing when it is whole"),
    "dispatch_gt": ("dispatch", "a tile-count threshold with > for >="),
    "lat_tile_lt": ("dispatch", "the latency frame tiles with rows < 32 / < 80 for <="),
    "fused_tail_lt": ("dispatch", "the fused last reduce with m < window for <="),
}
# the mistakes each family's tile loop or dispatch rule can make
FAMILY_MISTAKES = {f: ["tile_tail_mod"] for f in FAMILIES}
# not the 512 x 128 rule's: with > for >= an 800-wide layer stays on 256 x 128
# tiles up to 3072 rows, and the 3007-row blocks of before sit in between
# (tests/test_netgen.py asserts the kernel they reach)
FAMILY_MISTAKES["b16_32x32"].append("dispatch_gt")
FAMILY_MISTAKES["b16_128x128"].append("dispatch_gt")
FAMILY_MISTAKES["lat_gemm"] = ["lat_small_tail_mod", "window_rows_mod", "lat_tile_lt", "fused_tail_lt"]


def rows_written(m, family, mistake=None, tile=None, wave=None):
    """The output rows a family's tile loop produces on m rows, as a sorted
    array: blocks of `tile` rows, waves of `wave` rows inside a block, every
    row masked against the rows the block holds (lat_gemm: per window, on
    the window's frame tile).  Equals range(m) without a mistake."""
    t0, w0, _ = FAMILIES[family]
    tile, wave = tile or t0, wave or w0
    done = np.zeros(m, bool)

    def block_loop(r0, rows, tile, wave):
        for b0 in range(0, rows, tile):
            held = min(tile, rows - b0)
            small = mistake == "lat_small_tail_mod" and tile != LAT_TILES[2]
            if (mistake == "tile_tail_mod" or small) and b0 + tile >= rows:
                held = rows % tile
            for w in range(0, tile, wave):
                for f in range(w, min(w + wave, held)):
                    done[r0 + b0 + f] = True

    if family == "lat_gemm":
        for r0, rows, ftile in lat_plan(m, mistake):
            block_loop(r0, rows, ftile, ftile)
    else:
        block_loop(0, m, tile, wave)
    return np.flatnonzero(done)


def mistake_shows(layers, m, mode, family, mistake):
    """Whether a run of the net at m rows in `mode` would show `mistake` in
    `family`: rows missing, or another kernel named."""
    if family not in families_at(layers, m, mode):
        return False
    if MISTAKES[mistake][0] == "rows":
        return len(rows_written(m, family, mistake)) != m
    return dispatch(layers, m, mode, mistake) != dispatch(layers, m, mode)


# ------------------------------------------- the cases the GPU test scores --

EXACT_GEOMS = ("A", "D", "H")          # gathered / splice-pad (reaches 512 x 128) / whole-K-tile first layer
EXACT_RECIPES = ("wide", "two-planes")
BF16_GEOMS = ("A", "D")                # both cross bf16_small_tile's switch below CAP
F16_CASES = (("A", "FX"), ("B2", "wide"))
I8_GEOMS = ("I1", "I4", "I3")
FINALIZE_GEOMS = ("G20", "F4100")      # finalize_vec / the loop finalize


def case_modes(geom, recipe):
    """The modes an exact case runs in."""
    if (geom, recipe) in F16_CASES:
        return ("f16x3",)
    return MODES + (("bf16",) if geom in BF16_GEOMS else ())


def exact_ids():
    return [(g, r) for g in EXACT_GEOMS for r in EXACT_RECIPES] + list(F16_CASES)


_CASES = {}


def exact_case(geom, recipe):
    """(layers, x): netgen's net of the case, with an input of its own at the
    largest count of seam_rows over case_modes (read-only, built once)."""
    if (geom, recipe) not in _CASES:
        form = "f16x3" if (geom, recipe) in F16_CASES else "bf16x6"
        layers, = [c[1] for c in netgen.exact_cases(geom, form) if c[0] == recipe]
        xargs = dict(amax=1023) if recipe == "two-planes" else dict(amax=7) if recipe == "wide" else \
            netgen.plane_recipes(len(netgen.linears(layers)), form)[recipe][1]
        m = max(max(seam_rows(layers, mode)) for mode in case_modes(geom, recipe))
        x = netgen.int_input(layers, m - sum(netgen.context(layers)), 7000 + exact_ids().index((geom, recipe)), **xargs)
        x.setflags(write=False)
        _CASES[geom, recipe] = (layers, x)
    return _CASES[geom, recipe]


def finalize_net(geom):
    """The real-valued net of a geometry, ending in LogSoftmax (the one
    tests/test_gpu_gemm_shapes.py's real_case scores)."""
    in_d, widths, splices, post = netgen.GEOMETRIES[geom]
    return netgen.real_net(in_d, widths, splices, post, 2000 + sorted(netgen.GEOMETRIES).index(geom))


def gpu_runs():
    """[(id, layers, mode, old rows)] of every (net, mode) the GPU test sweeps
    over seam_rows."""
    import i8ref
    out = []
    for geom, recipe in exact_ids():
        layers, _ = exact_case(geom, recipe)
        for mode in case_modes(geom, recipe):
            out.append((f"{geom}-{recipe}-{mode}", layers, mode, old_rows(layers, recipe, geom)))
    for geom in FINALIZE_GEOMS:
        layers = finalize_net(geom)
        out += [(f"{geom}-finalize-{mode}", layers, mode, old_rows(layers, geom=geom)) for mode in MODES]
    for geom in I8_GEOMS:
        for mode in ("int8", "int8-latency", "int8-dynamic"):
            out.append((f"{geom}-{mode}", i8ref.net(geom), mode, old_rows(i8ref.net(geom), int8=True)))
    return out
