"""Inputs that sit on the rounding ties of Quantize, and an exact emulation of
the two ways the kernels form its quotient (tests/test_quantties.py proves the
conditions on the CPU; tests/test_gpu_quant_ties.py feeds the inputs to every
quantizer).

The reference computes roundf(clamp(x / scale + zp, 0, 255)).  The int8 nnet
path replaces the division by a corrected reciprocal product (csrc/i8_ops.h
qbyte).  A quotient that is off in its last bit changes the byte only where
q + zp sits on an n + 0.5 tie, and random data never sits there: tie_inputs
places float32 values on and next to every tie of a range and marks the
*sensitive* ones, whose byte changes when the correctly rounded quotient moves
by one ulp.

The emulation is exact rational arithmetic (fractions.Fraction) with one
round-to-nearest-even float32 rounding per IEEE operation, denormals kept.
RULE_OLD is the reciprocal rule as it stood before the scale threshold; it
lives here only, to show that the inputs tell the two apart.
"""
import functools
import math
from fractions import Fraction

import numpy as np

QDIV_MIN_SCALE = Fraction(1, 2 ** 100)   # i8_ops.h kQdivMinScale
RULE_OLD, RULE_FIXED = "old", "fixed"

# the ranges of the issue's CPU survey
NORMAL_RANGES = [(-3.7, 9.1), (0.0, 6.3), (-1.0, 1.0), (-8.25, 0.0), (-0.013, 0.021), (-1234.5, 4321.0), (2.0, 3.0),
                 (-5e-30, 7e-30)]
# scales from 2.98e-39 to 9.4e-38: 1 / scale is finite, the remainder
# x - scale * q0 falls below 2^-149
TINY_RANGES = [(0.0, 7.6e-37), (0.0, 1e-36), (0.0, 3e-36), (0.0, 2.4e-35)]
# scale == 2^-100 exactly (the first that takes the product) and the float
# below it (the last that takes the division)
_TOP = np.float32(255.0 * 2.0 ** -100)
THRESHOLD_RANGES = [(0.0, float(_TOP)), (0.0, float(np.nextafter(_TOP, np.float32(0))))]


# ------------------------------------------------------- exact float32 ops --

def f32(v):
    """Fraction -> the nearest float32 (ties to even, denormals kept), as a
    Fraction; +-inf as a float; None (NaN) stays None."""
    if v is None or isinstance(v, float):
        return v
    if v == 0:
        return Fraction(0)
    p, q = abs(v.numerator), v.denominator
    e = p.bit_length() - q.bit_length()          # 2^(e-1) < p / q < 2^(e+1)
    if (p < q << e) if e >= 0 else (p << -e < q):
        e -= 1                                   # now 2^e <= p / q < 2^(e+1)
    sh = max(e, -126) - 23                       # the float32 spacing there is 2^sh
    num, den = (p, q << sh) if sh >= 0 else (p << -sh, q)
    n, rem = divmod(num, den)
    if rem * 2 > den or (rem * 2 == den and n & 1):
        n += 1
    r = Fraction(n << sh) if sh >= 0 else Fraction(n, 1 << -sh)
    if r >= 1 << 128:
        return math.copysign(math.inf, v)
    return r if v > 0 else -r


def frac(x):
    """A float32 (or float) value as a Fraction; inf / NaN as f32 has them."""
    x = float(x)
    if math.isnan(x):
        return None
    return x if math.isinf(x) else Fraction(x)


def _finite(v):
    return isinstance(v, Fraction)


def quotient_div(x, scale):
    """IEEE x / scale of finite float32 x and scale > 0."""
    return f32(x / scale)


def _fma(a, b, c):
    """fmaf of float32 values: one rounding; NaN / inf as IEEE has them (the
    only non-finite operand here is an overflowed q0)."""
    if not (_finite(a) and _finite(b) and _finite(c)):
        return None if any(v is None for v in (a, b, c)) else math.inf   # class only: the caller falls back
    return f32(a * b + c)


def quotient(x, scale, rule):
    """The kernels' quotient: q = fma(fma(-scale, q0, x), r, q0), q0 = x * r,
    r = 1 / scale correctly rounded; the division when r is not finite, when
    the rule's threshold says so, or when q is not finite."""
    r = f32(1 / scale)
    if not _finite(r) or (rule == RULE_FIXED and scale < QDIV_MIN_SCALE):
        return quotient_div(x, scale)
    assert rule in (RULE_OLD, RULE_FIXED), rule
    q0 = f32(x * r)
    q = _fma(_fma(-scale, q0, x), r, q0)
    return q if _finite(q) else quotient_div(x, scale)


def byte_of(q, zp):
    """roundf(max(0, min(q + zp, 255))) of a float32 quotient: the sum rounded
    to float32, roundf half away from zero."""
    v = q + zp if isinstance(q, float) else f32(q + zp)
    if 255 < v:
        v = Fraction(255)
    if not 0 < v:
        v = Fraction(0)
    return int(math.floor(v + Fraction(1, 2)))


def next_f32(q, up):
    """The float32 neighbour of a finite float32 Fraction."""
    a = np.float32(float(q))
    assert Fraction(float(a)) == q
    return Fraction(float(np.nextafter(a, np.float32(np.inf if up else -np.inf))))


def bytes_of(x, scale, zp, rule=None, perturb=0):
    """uint8 bytes of float32 array x: rule None is the division, otherwise
    the kernels' product under that rule; perturb +-1 moves every quotient one
    float32 up / down first (the teeth test)."""
    s = frac(np.float32(scale))
    out = np.zeros(len(x), np.uint8)
    for i, v in enumerate(np.asarray(x, np.float32)):
        q = quotient_div(frac(v), s) if rule is None else quotient(frac(v), s, rule)
        if perturb:
            q = next_f32(q, perturb > 0)
        out[i] = byte_of(q, zp)
    return out


def quotients_differing(x, scale, rule, min_q=Fraction(1, 8)):
    """How many of the kernels' quotients are not the division's, among the
    elements with |x / scale| >= min_q.  (Below 1/8 no tie is in reach, and a
    denormal x has an inexact remainder at any scale: the clamp values next
    to 0 are such.)"""
    s = frac(np.float32(scale))
    n = 0
    for v in np.asarray(x, np.float32):
        d = quotient_div(frac(v), s)
        n += abs(d) >= min_q and quotient(frac(v), s, rule) != d
    return n


# -------------------------------------------------------------- tie inputs --

def params(oracle, mn, mx):
    """(scale, zp) of the range the way the reference takes them: Quantize's
    parameters of the two-element tensor [mn, mx] (as static_oracle)."""
    _, s, z = oracle.quantize(np.float32([mn, mx]))
    return np.float32(s), int(z)


_TIES = {}


def tie_inputs(oracle, mn, mx):
    """(x, sensitive, scale, zp): for every n in 0..254 the float32 nearest to
    (n + 0.5 - zp) * scale with its three float32 neighbours on each side
    (1785 values), then values up to 3 ulp outside both clamps;
    sensitive[i]: the byte of the correctly rounded quotient x[i] / scale
    differs from the byte of one of its float32 neighbours.  Read-only,
    computed once per range."""
    key = (float(np.float32(mn)), float(np.float32(mx)))
    if key in _TIES:
        return _TIES[key]
    scale, zp = params(oracle, mn, mx)
    s = frac(scale)
    assert s > 0
    xs = []
    for n in range(255):
        c = np.float32(float(f32((Fraction(2 * n + 1, 2) - zp) * s)))
        lo, hi = [c], [c]
        for _ in range(3):
            lo.append(np.nextafter(lo[-1], np.float32(-np.inf)))
            hi.append(np.nextafter(hi[-1], np.float32(np.inf)))
        xs += lo[:0:-1] + [c] + hi[1:]
    for edge, away in ((0, -np.inf), (255, np.inf)):
        v = np.float32(float(f32((Fraction(edge) - zp) * s)))
        for _ in range(4):
            xs.append(v)
            v = np.nextafter(v, np.float32(away))
    x = np.array(xs, np.float32)
    sens = np.zeros(len(x), bool)
    for i, v in enumerate(x):
        q = quotient_div(frac(v), s)
        b = byte_of(q, zp)
        sens[i] = byte_of(next_f32(q, True), zp) != b or byte_of(next_f32(q, False), zp) != b
    x.setflags(write=False)
    sens.setflags(write=False)
    _TIES[key] = (x, sens, scale, zp)
    return _TIES[key]


# ---------------------------------------------------------- the range list --

def _significand(v):
    return int(np.float32(v).view(np.uint32)) & 0x7FFFFF


@functools.lru_cache(maxsize=None)
def _range_with_scale(oracle, target):
    """A range [0, mx] whose scale is the float32 `target`: the scale is
    float((double)mx / 255), about one scale ulp per ulp of mx, so mx is the
    float32 at 255 * target or a neighbour."""
    target = np.float32(target)
    mx = np.float32(255.0 * float(target))
    for step in (0, 1, -1, 2, -2):
        c = mx
        for _ in range(abs(step)):
            c = np.nextafter(c, np.float32(np.inf if step > 0 else -np.inf))
        if params(oracle, 0.0, c)[0] == target:
            return 0.0, float(c)
    raise AssertionError(f"no range [0, mx] has the scale {target!r}")


def significand_ranges(oracle):
    """Scales with an all-ones and a 1 + ulp significand, at two magnitudes:
    the hardest cases of a reciprocal."""
    out = []
    for e in (-7, -65):
        ones = np.nextafter(np.float32(2.0 ** (e + 1)), np.float32(0))
        one_ulp = np.nextafter(np.float32(2.0 ** e), np.float32(np.inf))
        assert _significand(ones) == 0x7FFFFF and _significand(one_ulp) == 1
        out += [_range_with_scale(oracle, float(ones)), _range_with_scale(oracle, float(one_ulp))]
    return out


def all_ranges(oracle):
    """[(name, (mn, mx))]: every range the tie tests use."""
    out = [("normal", r) for r in NORMAL_RANGES]
    out += [("significand", r) for r in significand_ranges(oracle)]
    out += [("tiny", r) for r in TINY_RANGES]
    out += [("threshold", r) for r in THRESHOLD_RANGES]
    return out
