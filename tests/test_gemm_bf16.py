"""The plain bf16 GEMM mode on the host (no GPU): the mode's name and number,
ce_gpu_gemm_mode_from_name, and the proof that bf16ref.walk is a valid
zero-tolerance oracle for tests/test_gpu_gemm_bf16.py's exact leg."""
import ctypes

import numpy as np
import pytest

import bf16ref
import netgen

EXACT_GEOMS = ("A", "B", "C", "D", "F4100", "G9", "G20", "G25")
NAMES = {"fp32": 0, "bf16x6": 1, "f16x3": 2, "bf16x6p": 3, "bf16": 4}


def test_mode_is_named_bf16_and_numbered_4():
    from catears_amd import gpu
    assert gpu.GEMM_MODES["bf16"] == 4
    assert gpu.GEMM_MODES == NAMES


def test_gemm_mode_from_name_round_trips_and_rejects():
    from catears_amd import gpu
    for name, mode in NAMES.items():
        assert gpu.gemm_mode_from_name(name) == mode
        assert gpu.gemm_mode_from_name(name.encode()) == mode
    for bad in ("", "bf", "bf16 ", "BF16", "bf16x", "bf16x6pp", "int8", "4", "fp32\n"):
        with pytest.raises(gpu.CatearsError) as e:
            gpu.gemm_mode_from_name(bad)
        assert e.value.code == -2, bad
    with pytest.raises(gpu.CatearsError) as e:
        gpu.gemm_mode_from_name(None)
    assert e.value.code == -2
    # a NULL result pointer
    assert gpu.lib().ce_gpu_gemm_mode_from_name(b"bf16", None) == -2
    v = ctypes.c_int(77)
    assert gpu.lib().ce_gpu_gemm_mode_from_name(b"bogus", ctypes.byref(v)) == -2


def test_rne_bf16_rounds_to_nearest_even():
    f = lambda bits: np.array([bits], np.uint32).view(np.float32)
    bits = lambda v: int(bf16ref.rne_bf16(v).view(np.uint32)[0])
    assert bits(f(0x3f800000)) == 0x3f800000
    assert bits(f(0x3f807fff)) == 0x3f800000          # below the tie: down
    assert bits(f(0x3f808000)) == 0x3f800000          # tie, even below: down
    assert bits(f(0x3f808001)) == 0x3f810000          # above the tie: up
    assert bits(f(0x3f818000)) == 0x3f820000          # tie, odd below: up
    assert bits(f(0xbf818000)) == 0xbf820000
    assert bits(f(0x7f7fffff)) == 0x7f800000          # rounds to infinity, as the hardware does
    assert np.isnan(bf16ref.rne_bf16(f(0x7fc00001))[0])
    assert bits(np.array([257.0], np.float32)) == np.array([256.0], np.float32).view(np.uint32)[0]
    assert bits(np.array([259.0], np.float32)) == np.array([260.0], np.float32).view(np.uint32)[0]


@pytest.mark.parametrize("geom", EXACT_GEOMS)
def test_exact_leg_is_a_valid_oracle(geom):
    """For every exact-integer case: the mode's definition evaluated with an
    fp64 accumulator, an fp32 one and an fp32 one on K reversed gives the same
    bits; per Linear sum |bf16(a)| |bf16(w)| + |b| < 2^24 (so every order of
    every correct kernel does); and the rounding matters -- the result differs
    from the unrounded net's on at least one row, and from truncation's."""
    for name, layers, x in netgen.one_plane_mode_cases(geom):
        ref = bf16ref.walk(layers, x, np.float64)
        assert ref.dtype == np.float32
        assert np.array_equal(ref, bf16ref.walk(layers, x, np.float32)), (geom, name)
        assert np.array_equal(ref, bf16ref.walk(layers, x, np.float32, k_reversed=True)), (geom, name)
        bounds = bf16ref.exact_bounds(layers, x)
        assert len(bounds) == len(netgen.linears(layers)) and max(bounds) < 24.0, (geom, name, bounds)
        changed = int((ref != netgen.exact(layers, x)).any(axis=1).sum())
        print(f"{geom}/{name}: bounds 2^{min(bounds):.1f} .. 2^{max(bounds):.1f}, "
              f"rounding changes {changed} of {ref.shape[0]} rows")
        assert changed >= 1, (geom, name)
        trunc = bf16ref.walk(layers, x, np.float64, rnd=bf16ref.trunc_bf16)
        assert (ref != trunc).any(), (geom, name, "truncation gives the same rows")


def test_b2_rounds_nothing():
    """Geometry B2's operands all fit one bf16 plane: the mode's result is the
    unrounded net's -- the case where bf16 must equal bf16x6 bit for bit."""
    for name, layers, x in netgen.exact_cases("B2"):
        assert np.array_equal(bf16ref.walk(layers, x, np.float64), netgen.exact(layers, x)), name


def test_exact_cases_reach_both_tiles_odd_k_and_ragged_n():
    """The restated tile rule over the GPU exact leg's (geometry, rows): both
    tile shapes, odd K-tile counts on both, and the ragged widths."""
    import test_gpu_gemm_bf16 as t
    seen = set()
    for geom, rows in t.exact_params():
        layers = netgen.exact_cases(geom)[0][1]
        seen.update(bf16ref.tiles(layers, rows))
    shapes = {s for s, _, _ in seen}
    assert shapes == {"b16_32x32", "b16_128x128"}
    for shape in shapes:
        assert any(kt % 2 == 1 for s, kt, _ in seen if s == shape), shape
        assert any(n % 128 != 0 for s, _, n in seen if s == shape), shape
    assert {36, 100, 772, 1028, 4100} <= {n for _, _, n in seen}
    assert {"b16_32x32", "b16_128x128"} <= {s for s, _, n in seen if n == 4100}
    for g in ("A", "D", "F4100", "G9", "G25"):
        assert any(kt % 2 == 1 for _, kt, _ in bf16ref.tiles(netgen.exact_cases(g)[0][1], 17)), g
