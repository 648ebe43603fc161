"""CPU: the fixed-point form of the complex128 QAM margin certificate (csrc/walk_f64.hpp: walk_qam_fixed4) replayed in exact
arithmetic, against the f64 certificate it stands in front of (csrc/modem.hpp: demod_qam_cert).

The rule, per axis, S = 24, delta = 2, c1 = hs 2^S, c0 = (hl + 1/2) 2^S:
    q = (int) fma(e, c1, c0);  q = med3(q, 2^(S-1), lm1 2^S + 2^(S-1));  k = q >> S;  f = q & (2^S - 1)
    vouched iff delta <= f <= 2^S - 1 - delta   (the kernel tests ((q - delta) << 8) <= ((2^S - 1 - 2 delta) << 8) unsigned: replayed too)
The multiply-add is rounded ONCE (exact rational arithmetic, then one rounding to binary64); the conversion truncates, saturates, and
turns NaN into 0 (v_cvt_i32_f64).  The f64 certificate: t = fl(e hs + hl) (one rounding as compiled, two as written: both replayed),
clamped to [0, lm1], r = rint(t), vouched iff |t - r| <= 1/2 - 2^-30.

Claims held here, on points 2^-k off every half-integer boundary (k = 20 ... 42), on exact half-integers, below 0 and above lm1, and
on +-1e300, +-inf, NaN:
  * every axis the fixed-point test vouches for is vouched for by the f64 certificate, with the same level;
  * every point within 2^-30 of a boundary is NOT vouched (it goes to the f64 form and, there, to the sweep)."""
import math
from fractions import Fraction

import numpy as np
import pytest

S, DELTA = 24, 2
MASK = (1 << S) - 1
LIM = 0.5 - 2.0 ** -30


def _round(fr):
    """one rounding of an exact rational to binary64 (int / int true division is correctly rounded)"""
    try:
        return fr.numerator / fr.denominator
    except OverflowError:
        return math.inf if fr > 0 else -math.inf


def _fma(a, b, c):
    if math.isnan(a) or math.isinf(a):
        return a * b + c
    return _round(Fraction(a) * Fraction(b) + Fraction(c))


def _cvt_i32(x):
    if math.isnan(x):
        return 0
    if x >= 2.0 ** 31:
        return 2 ** 31 - 1
    if x <= -2.0 ** 31:
        return -2 ** 31
    return int(x)                                   # toward zero


def _fixed(e, hs, hl, lm1):
    """(level, vouched) of one axis by the fixed-point rule; the kernel's shifted unsigned test must say the same"""
    c1, c0 = hs * 2.0 ** S, (hl + 0.5) * 2.0 ** S
    assert Fraction(c1) == Fraction(hs) * 2 ** S and Fraction(c0) == (Fraction(hl) + Fraction(1, 2)) * 2 ** S      # exact scalings
    q = _cvt_i32(_fma(e, c1, c0))
    lo, hi = 1 << (S - 1), (lm1 << S) + (1 << (S - 1))
    q = sorted((q, lo, hi))[1]
    k, f = q >> S, q & MASK
    vouched = DELTA <= f <= MASK - DELTA
    shifted = (((q << 8) & 0xFFFFFFFF) + ((-DELTA << 8) & 0xFFFFFFFF)) & 0xFFFFFFFF
    assert (shifted <= ((MASK - 2 * DELTA) << 8)) == vouched
    assert shifted == (((q - DELTA) & MASK) << 8)
    return k, vouched


def _parent(e, hs, hl, lm1, fused):
    """(level, vouched) of one axis by demod_qam_cert"""
    t = _fma(e, hs, hl) if fused else e * hs + hl
    t = min(max(t, 0.0), float(lm1)) if not math.isnan(t) else 0.0          # fmax(NaN, 0) = 0
    r = float(np.rint(t))
    return int(r), abs(t - r) <= LIM


def _axis_points(hs, hl, lm1):
    """estimates e whose level coordinate t = e hs + hl sits at the chosen places (up to the rounding of e itself: the replay
    works from e, whatever t it gives)"""
    ks = sorted(set(range(20, 43)) | {23, 24, 25, 26})
    ts = []
    for b in range(-1, lm1 + 1):                        # every half-integer from -1/2 to lm1 + 1/2
        h = b + 0.5
        ts.append(h)
        for k in ks:
            ts += [h + 2.0 ** -k, h - 2.0 ** -k]
        for k in (22, 23, 24):                          # the new margin itself: delta 2^-S = 2^-23 and its neighbours
            for m in (1, 2, 3, 4, 5):
                ts += [h + m * 2.0 ** -(k + 1), h - m * 2.0 ** -(k + 1)]
    ts += [-0.5 + 2.0 ** -40, -0.5 - 2.0 ** -40, -0.25, -3.0, -1000.0, lm1 + 0.25, lm1 + 0.5 - 2.0 ** -40, lm1 + 0.5 + 2.0 ** -40,
           lm1 + 7.0, lm1 + 1000.0]
    ts += [float(v) for v in range(lm1 + 1)] + list(np.random.RandomState(lm1).uniform(-1.0, lm1 + 1.0, 300))
    es = [(t - hl) / hs for t in ts]
    es += [1e300, -1e300, math.inf, -math.inf, math.nan, 0.0, -0.0, 2.0 ** 40, -2.0 ** 40]
    return es


@pytest.mark.parametrize("L", [4, 8, 16])
@pytest.mark.parametrize("sign", [1, -1], ids=["re", "im"])
def test_fixed_point_vouches_only_where_the_f64_certificate_does(L, sign):
    """sign = -1: the imaginary axis, t = hl - e hs (the multiply-add takes -hs / -c1)"""
    M = L * L
    scale = math.sqrt(2.0 * (M - 1) / 3.0)                # unit-energy square QAM: levels (2 k - lm1) / scale
    lm1, hs, hl = L - 1, sign * 0.5 * scale, 0.5 * (L - 1)
    n_vouched = n_declined = n_near = 0
    for e in _axis_points(abs(hs), hl, lm1):
        e = sign * e if not math.isnan(e) else e
        k, vouched = _fixed(e, hs, hl, lm1)
        if vouched:
            n_vouched += 1
            for fused in (True, False):
                pk, pv = _parent(e, hs, hl, lm1, fused)
                assert pv and pk == k, (e, k, pk, pv, fused)
        else:
            n_declined += 1
        if not (math.isnan(e) or math.isinf(e)):
            te = Fraction(e) * Fraction(hs) + Fraction(hl)
            for b in range(0, lm1):                         # the boundaries between two levels
                if abs(te - (b + Fraction(1, 2))) <= Fraction(1, 2 ** 30):
                    n_near += 1
                    assert not vouched, (e, float(te), k)
    assert n_vouched > 300 and n_declined > 30 * lm1 and n_near > 20 * lm1


@pytest.mark.parametrize("L", [4, 8, 16])
def test_saturating_inputs_land_on_a_vouched_clamped_end(L):
    M = L * L
    scale = math.sqrt(2.0 * (M - 1) / 3.0)
    lm1, hs, hl = L - 1, 0.5 * scale, 0.5 * (L - 1)
    for e, want in ((1e300, lm1), (math.inf, lm1), (-1e300, 0), (-math.inf, 0), (math.nan, 0), (-0.5 / hs - hl / hs, 0)):
        assert _fixed(e, hs, hl, lm1) == (want, True)
        assert _parent(e, hs, hl, lm1, True) == (want, True)
    # the imaginary axis negates: NaN still goes to level 0 on both sides
    assert _fixed(math.nan, -hs, hl, lm1) == (0, True) and _parent(math.nan, -hs, hl, lm1, True) == (0, True)
