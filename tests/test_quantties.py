"""The CPU side of the tie tests (tests/quantties.py): the inputs have teeth,
the emulated division is the oracle's, the reciprocal product as it stood
misses bytes on the tiny-scale window, and with qbyte_rscale's threshold it
equals the division on every range the GPU tests use."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import quantties as qt


@functools.lru_cache(maxsize=None)
def _case(oracle, mn, mx):
    """(x, sensitive, scale, zp, division bytes) of a range, once."""
    x, sens, scale, zp = qt.tie_inputs(oracle, mn, mx)
    div = qt.bytes_of(x, scale, zp)
    div.setflags(write=False)
    return x, sens, scale, zp, div


def _ranges(oracle, *kinds):
    return [r for kind, r in qt.all_ranges(oracle) if kind in kinds]


def test_f32_rounding_is_ieee():
    """qt.f32 against numpy's float64 -> float32 conversion: normals, ties,
    denormals, the overflow threshold."""
    rng = np.random.default_rng(5)
    vals = list(rng.normal(0, 1, 200) * 10.0 ** rng.integers(-44, 38, 200))
    one = 1.0 + 2.0 ** -24            # a tie: to even, down
    vals += [one, 1.0 + 3 * 2.0 ** -24, 2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150, 2.0 ** -126 - 2.0 ** -150,
             float(np.finfo(np.float32).max), 2.0 ** 128 - 2.0 ** 103, 2.0 ** 128 - 2.0 ** 104 - 1e20, 0.0]
    with np.errstate(over="ignore"):
        for v in vals:
            for w in (v, -v):
                got, want = qt.f32(Fraction(w)), float(np.float32(w))
                assert float(got) == want, (w, got, want)


def test_range_list_holds_what_the_issue_names(oracle):
    kinds = [k for k, _ in qt.all_ranges(oracle)]
    assert kinds.count("normal") == 8 and kinds.count("tiny") >= 4 and kinds.count("significand") == 4
    sig = [int(qt.params(oracle, *r)[0].view(np.uint32)) & 0x7FFFFF for r in qt.significand_ranges(oracle)]
    assert sig == [0x7FFFFF, 1, 0x7FFFFF, 1]
    for r in qt.TINY_RANGES:
        s = float(qt.params(oracle, *r)[0])
        assert 2.94e-39 < s < 2e-37 and np.isfinite(np.float32(1) / np.float32(s))
    (above, below) = [qt.params(oracle, *r)[0] for r in qt.THRESHOLD_RANGES]
    assert Fraction(float(above)) == qt.QDIV_MIN_SCALE and below == np.nextafter(above, np.float32(0))


@pytest.mark.parametrize("i", range(18))
def test_tie_inputs_have_teeth(oracle, i):
    """Every range: 1785 tie values and the clamp values, at least 200
    sensitive elements over at least 128 distinct bytes, both clamps reached;
    the emulated division is the oracle's Quantize bit for bit; and moving
    every quotient one float32 up or down changes the expected bytes -- on
    exactly the sensitive elements."""
    ranges = qt.all_ranges(oracle)
    assert len(ranges) == 18
    _, (mn, mx) = ranges[i]
    x, sens, scale, zp, div = _case(oracle, mn, mx)
    assert len(x) == 255 * 7 + 8 and x.dtype == np.float32
    assert int(sens.sum()) >= 200 and len(set(div[sens].tolist())) >= 128, (int(sens.sum()), len(set(div[sens])))
    assert np.array_equal(div, oracle._quantize_with(x, scale, zp))
    assert div[-8:-4].tolist() == [0] * 4 and div[-4:].tolist() == [255] * 4
    up, down = qt.bytes_of(x, scale, zp, perturb=+1), qt.bytes_of(x, scale, zp, perturb=-1)
    assert (up != div).sum() >= 100 and (down != div).sum() >= 100
    assert np.array_equal((up != div) | (down != div), sens)


def test_old_rule_misses_bytes_on_the_tiny_window(oracle):
    """The reciprocal product without the threshold: 10 bytes of [0, 7.6e-37]
    and 6 of [0, 3e-36] are not the division's (every one a sensitive
    element), and quotients differ on every range of the window."""
    wrong = {}
    for mn, mx in qt.TINY_RANGES:
        x, sens, scale, zp, div = _case(oracle, mn, mx)
        old = qt.bytes_of(x, scale, zp, qt.RULE_OLD)
        assert sens[old != div].all()
        wrong[mx] = int((old != div).sum())
        assert qt.quotients_differing(x, scale, qt.RULE_OLD) > 0, (mn, mx)
    print(wrong)
    assert wrong[7.6e-37] == 10 and wrong[3e-36] == 6


def test_fixed_rule_is_the_division_on_every_range(oracle):
    for kind, (mn, mx) in qt.all_ranges(oracle):
        x, _, scale, zp, div = _case(oracle, mn, mx)
        assert qt.quotients_differing(x, scale, qt.RULE_FIXED) == 0, (kind, mn, mx)
        assert np.array_equal(qt.bytes_of(x, scale, zp, qt.RULE_FIXED), div), (kind, mn, mx)


def test_both_rules_agree_off_the_tiny_window(oracle):
    """At and above the threshold, and on every ordinary range, the product
    needs no threshold: the old rule gives the division's quotients too (so
    the threshold moves no bit of an ordinary scale)."""
    for mn, mx in _ranges(oracle, "normal", "significand") + qt.THRESHOLD_RANGES[:1]:
        x, _, scale, zp, div = _case(oracle, mn, mx)
        assert qt.quotients_differing(x, scale, qt.RULE_OLD) == 0, (mn, mx)
        assert np.array_equal(qt.bytes_of(x, scale, zp, qt.RULE_OLD), div), (mn, mx)


def test_threshold_margin(oracle):
    """The derivation in i8_ops.h: with scale >= 2^-100 the remainder of every
    tie input with |q| >= 1/8 is a multiple of 2^-149 (exact in the inner
    fma); one binade below the window's top it is not."""
    def inexact(mn, mx):
        x, _, scale, _ = qt.tie_inputs(oracle, mn, mx)
        s = qt.frac(scale)
        r = qt.f32(1 / s)
        n = 0
        for v in x:
            v = qt.frac(v)
            q0 = qt.f32(v * r)
            if abs(q0) >= Fraction(1, 8):
                rem = v - s * q0
                n += qt.f32(rem) != rem
        return n
    assert inexact(*qt.THRESHOLD_RANGES[0]) == 0
    assert inexact(*qt.TINY_RANGES[0]) > 0
