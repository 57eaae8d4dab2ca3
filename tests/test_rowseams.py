"""CPU proofs for tests/rowseams.py: the restated constants are the sources',
seam_rows sits on both sides of every switch, every named mistake shows at a
seam count and at none of the counts the suite presented before, and the
exact inputs keep the 2^24 budget at their largest count."""
import os
import re

import numpy as np
import pytest

import bf16ref
import i8ref
import netgen
import rowseams
from rowseams import FAMILIES

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "catears_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def ints(pattern, text):
    m = re.search(pattern, text)
    assert m, f"{pattern!r} has moved"
    return tuple(int(g) for g in m.groups())


# ---------------------------------------------------------------- no drift --

def test_constants_are_the_sources():
    h = source("gemm_bf16x6_kernels.h")
    internal = source("internal.h")
    assert ints(r"constexpr int kX6WideMinTiles = (\d+);", h) == (rowseams.X6_WIDE_MIN_TILES,)
    assert ints(r"constexpr int kX6LatWindow = (\d+);", internal) == (rowseams.X6_LAT_WINDOW,)
    assert ints(r"constexpr int kB16LargeMinTiles = (\d+);", internal) == (rowseams.B16_LARGE_MIN_TILES,)
    assert ints(r"constexpr int kI8LatMaxRows = (\d+);", internal) == (rowseams.I8_LAT_MAX_ROWS,)
    assert rowseams.I8_LAT_MAX_ROWS == i8ref.LAT_MAX_ROWS and rowseams.B16_LARGE_MIN_TILES == bf16ref.LARGE_MIN_TILES

    def tile_wave(bf, wgf):
        return bf, bf // wgf

    # X6Cfg / W6Cfg / B16Cfg / X3Cfg <BW, BF, WGW, WGF, ...>: BF frames over WGF waves
    bw, bf, wgw, wgf = ints(r"using X6D128 = X6Cfg<(\d+), (\d+), (\d+), (\d+), \d+>;", h)
    assert tile_wave(bf, wgf) == FAMILIES["x6d_128x128"][:2]
    bf, wgw, wgf = ints(r"using X6D256 = X6Cfg<kX6DirUnits, (\d+), (\d+), (\d+), \d+>;", h)
    assert tile_wave(bf, wgf) == FAMILIES["x6d_256x128"][:2]
    bw, bf, wgw, wgf = ints(r"using X6W512 = W6Cfg<(\d+), (\d+), (\d+), (\d+)>;", h)
    assert tile_wave(bf, wgf) == FAMILIES["x6w_512x128"][:2] and bw == rowseams.X6_WIDE_UNITS
    x6 = source("kernels/gemm_bf16x6.hip")
    bw, bf, wgw, wgf = ints(r"using Q = X6Cfg<(\d+), (\d+), (\d+), (\d+), \d+>;", x6)
    assert tile_wave(bf, wgf) == FAMILIES["x6q_128x128"][:2]
    assert "x6w_fits<X6W512>(p, kX6WideMinTiles)" in x6
    assert "tiles_n * tiles_m >= min_tiles" in h and "(p.m + C::BF - 1) / C::BF" in h

    # gemm_f32 Cfg<BM, BN, BK, WGM, WGN>: BM rows over WGM waves, MFMA steps of 32 rows
    f32 = source("kernels/gemm_f32.hip")
    bm, bn, bk, wgm, wgn = ints(r"using V2 = Cfg<(\d+), (\d+), (\d+), (\d+), (\d+)>;", f32)
    assert (bm, bm // wgm, 32) == FAMILIES["f32_glds"]
    bm, bn, bk, wgm, wgn = ints(r"using V3 = Cfg<(\d+), (\d+), (\d+), (\d+), (\d+)>;", f32)
    assert (bm, bm // wgm, 32) == FAMILIES["f32_pipe2"]
    assert "TI = BM / WGM / 32" in f32
    assert "return launch_glds<V2, 2>(s, p, a_fast, a.b_nmajor, rm);" in f32
    assert "return launch_pipe2<V3>(s, p, a_fast, b_nmajor, rm);" in f32

    b16 = source("kernels/gemm_bf16.hip")
    bw, bf, wgw, wgf = ints(r"if \(bf16_small_tile\(a\.m, a\.n\)\) return "
                            r"launch_b16<B16Cfg<(\d+), (\d+), (\d+), (\d+), \d+>>", b16)
    assert tile_wave(bf, wgf) == FAMILIES["b16_32x32"][:2]
    bw, bf, wgw, wgf = ints(r"\n  return launch_b16<B16Cfg<(\d+), (\d+), (\d+), (\d+), \d+>>", b16)
    assert tile_wave(bf, wgf) == FAMILIES["b16_128x128"][:2]
    assert "((rows + 127) / 128) * ((n + 127) / 128) < kB16LargeMinTiles" in b16

    x3 = source("kernels/gemm_f16x3.hip")
    bf64, wgf64, bf32, wgf32 = ints(r"case 0:\s+return k64 \? "
                                    r"launch_cfg<X3Cfg<\d+, (\d+), \d+, (\d+), \d+, 64>>\(s, p, out16\)\s+"
                                    r": launch_cfg<X3Cfg<\d+, (\d+), \d+, (\d+), \d+, 32>>", x3)
    assert tile_wave(bf64, wgf64) == tile_wave(bf32, wgf32) == FAMILIES["x3_128x128"][:2]

    i8 = source("kernels/nnet_i8.hip")
    bm, bn, wgm, wgn = ints(r"using ProductTile = I8Tile<(\d+), (\d+), (\d+), (\d+)>;", i8)
    assert (bm, bm // wgm, 32) == FAMILIES["i8_256x128"] and (bm, bn) == (i8ref.TILE_M, i8ref.TILE_N)
    assert "TI = BM / WGM / 32" in source("nnet_i8_kernels.h")
    i8l = source("kernels/nnet_i8_lat.hip")
    rt, = ints(r"constexpr int kRT = (\d+);", i8l)
    assert "constexpr int kBM = 16 * kRT;" in i8l and (16 * rt, 16 * rt, 16) == FAMILIES["i8_lat"]
    assert 'CE_KNOB("CATEARS_I8_LAT_MAXROWS", kI8LatMaxRows)' in i8l

    lat = source("kernels/gemm_bf16x6_lat.hip")
    limits = ints(r"if \(p\.rows <= (\d+)\)\s+fixed = launch_lat_gemm<(\d+)>\(s, p\);\s+else if \(p\.rows <= (\d+)\)\s+"
                  r"fixed = launch_lat_gemm<(\d+)>\(s, p\);\s+else\s+fixed = launch_lat_gemm<(\d+)>\(s, p\);", lat)
    assert (limits[0], limits[2]) == rowseams.LAT_TILE_LIMITS
    assert tuple(16 * limits[i] for i in (1, 3, 4)) == rowseams.LAT_TILES
    assert "p.row_tiles = (p.rows + 16 * TF - 1) / (16 * TF);" in lat
    assert FAMILIES["lat_gemm"][0] == rowseams.LAT_TILES[2]
    assert "for (int r0 = 0; r0 < a.m; r0 += kX6LatWindow) {" in lat
    assert "a.tail && a.m <= kX6LatWindow && a.n % 4 == 0 && a.n <= 4096" in lat

    # the row kernels: one block of 256 threads per 4 rows
    per = f"(rows + {rowseams.ROW_KERNEL_ROWS - 1}) / {rowseams.ROW_KERNEL_ROWS}"
    rowops = source("kernels/rowops.hip")
    assert rowops.count(f"dim3 grid({per})") + rowops.count(f"dim3({per})") >= 4
    assert f"dim3({per})" in i8 and f"dim3({per})" in x6 and f"dim3({per})" in x3 and f"dim3({per})" in b16


def test_residues_are_the_issue_s():
    assert rowseams.residues(128, 32) == [0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127]
    assert rowseams.x6w_switch(800) == 2944 and rowseams.x6w_switch(256) is None
    assert rowseams.row_kernel_rows() == [126, 127, 128, 129, 254, 255, 256, 257]


# ------------------------------------------------ both sides of each switch --

RUNS = rowseams.gpu_runs()


@pytest.mark.parametrize("run", RUNS, ids=[r[0] for r in RUNS])
def test_seam_rows_sit_on_both_sides_of_every_switch(run):
    name, layers, mode, _ = run
    rows = rowseams.seam_rows(layers, mode)
    c = sum(netgen.context(layers))
    assert rows == sorted(set(rows)) and rows[0] > c and rows[-1] <= rowseams.CAP
    for lo, hi, what in rowseams.switches(layers, mode):
        assert lo in rows and hi in rows, (name, what)
        a, b = rowseams.dispatch(layers, lo, mode), rowseams.dispatch(layers, hi, mode)
        assert a != b, (name, what, a)
        if mode in rowseams.MODES and "frame tile" not in what and "windows" not in what:
            assert netgen.kernels(layers, lo - c, mode) != netgen.kernels(layers, hi - c, mode), (name, what)
        if mode == "bf16":
            assert bf16ref.tiles(layers, lo - c) != bf16ref.tiles(layers, hi - c), (name, what)
    # a whole number of row tiles, and one row more, for every family the net runs in
    for family in set().union(*(rowseams.families_at(layers, m, mode) for m in rows)):
        tile = FAMILIES[family][0]
        mine = [m for m in rows if family in rowseams.families_at(layers, m, mode)]
        if mode != "int8-latency" or family == "i8_lat":
            assert any(m % tile == 0 for m in mine) and any(m % tile == 1 and m > tile for m in mine), (name, family)


def test_every_switch_kind_is_reached():
    kinds = {}
    for name, layers, mode, _ in RUNS:
        for lo, hi, what in rowseams.switches(layers, mode):
            kinds.setdefault(mode, set()).add(lo)
    assert 2944 in kinds["bf16x6"]                                  # 800 wide: 23 against 24 row tiles
    assert {32, 80, 1024, 1056, 1104, 2048} <= kinds["latency"]
    assert kinds["bf16"] and kinds["int8-latency"] == {280}
    a, _ = rowseams.exact_case("A", "wide")
    assert {2944, 2945, 3072, 3073} <= set(rowseams.seam_rows(a, "bf16x6"))
    assert {32, 33, 80, 81, 1023, 1024, 1025, 2048, 2049} <= set(rowseams.seam_rows(a, "latency"))


# ----------------------------------------------------------- mutation proof --

def test_the_models_are_right_without_a_mistake():
    for family in FAMILIES:
        for m in (1, 31, 32, 33, 96, 128, 129, 1024, 1025, 2048):
            assert np.array_equal(rowseams.rows_written(m, family), np.arange(m)), (family, m)


def test_every_mistake_shows_at_a_seam_count_and_at_no_old_one():
    ran = set()
    shown = {}
    for name, layers, mode, old in RUNS:
        new = rowseams.seam_rows(layers, mode)
        c = sum(netgen.context(layers))
        for family in FAMILIES:
            for mistake in rowseams.FAMILY_MISTAKES[family]:
                at = [m for m in new if rowseams.mistake_shows(layers, m, mode, family, mistake)]
                before = [m for m in old if m > c and rowseams.mistake_shows(layers, m, mode, family, mistake)]
                assert not before, f"{name}: {mistake} in {family} already showed at {before}"
                if at:
                    shown.setdefault((family, mistake), []).append((name, at[:4]))
        ran |= set().union(*(rowseams.families_at(layers, m, mode) for m in new))
    # f32_pipe2 runs on misaligned caller rows only: test_fp32_pipe2_on_misaligned_rows of the GPU test,
    # on the 128-row tile's counts, which hold the 64-row tile's
    assert ran == set(FAMILIES) - {"f32_pipe2"}, ran
    for family in ran:
        assert rowseams.FAMILY_MISTAKES[family], family
        for mistake in rowseams.FAMILY_MISTAKES[family]:
            assert (family, mistake) in shown, f"no seam count shows {mistake} in {family}"
    for (family, mistake), where in sorted(shown.items()):
        print(f"{family:12s} {mistake:16s} {where[0]}")


# -------------------------------------------------------------- exact budget --

@pytest.mark.parametrize("geom,recipe", rowseams.exact_ids())
def test_exact_inputs_keep_the_budget_at_the_largest_count(geom, recipe):
    layers, x = rowseams.exact_case(geom, recipe)
    form = "f16x3" if (geom, recipe) in rowseams.F16_CASES else "bf16x6"
    netgen.check_exact_budget(layers, x, form)
    if "bf16" in rowseams.case_modes(geom, recipe):
        assert max(bf16ref.exact_bounds(layers, x)) < 24.0
    c = sum(netgen.context(layers))
    assert len(x) == max(max(rowseams.seam_rows(layers, m)) for m in rowseams.case_modes(geom, recipe))
    assert len(x) - c >= 1
