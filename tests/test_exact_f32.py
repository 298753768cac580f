"""tests/exact_f32.py against rational arithmetic: fma32(a, b, c) must be the f32 nearest to the
exact a b + c, ties to even (fractions.Fraction and a rounding written out below), bit for bit:
random normals, constructed ties of the f64 sum with a residual on either side (the one case the
helper corrects; their number is asserted), subnormal results, exact cancellation and the sign of
its zero, overflow with the midpoint below 2^128, inf and NaN addends."""
import math
from fractions import Fraction

import numpy as np
import torch

from exact_f32 import chain32, f32, fma32

_MAXF = Fraction(2) ** 128 - Fraction(2) ** 104  # the largest finite f32


def _rn32(x):
    """the f32 nearest to the non-zero rational x, ties to even, as a Python float (or +-inf)"""
    sign, x = (-1.0, -x) if x < 0 else (1.0, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1  # 2^e <= x < 2^(e + 1)
    q = Fraction(2) ** (max(e, -126) - 23)  # the spacing of f32 there (subnormals: 2^-149)
    n = x / q
    lo = n.numerator // n.denominator
    rem = n - lo
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    v = lo * q
    return sign * (float(v) if v <= _MAXF else math.inf)


def _want(a, b, c):
    """fmaf(a, b, c) of three f32 values given as Python floats"""
    if not all(map(math.isfinite, (a, b, c))):
        return a * b + c  # inf and NaN: as any IEEE arithmetic does (no case here has a finite overflow)
    x = Fraction(a) * Fraction(b) + Fraction(c)
    if x == 0:  # an exact zero sum is +0 unless both the product and the addend are -0
        p_neg = math.copysign(1.0, a) * math.copysign(1.0, b) < 0
        both = (Fraction(a) * Fraction(b) == 0 and c == 0 and p_neg and math.copysign(1.0, c) < 0)
        return -0.0 if both else 0.0
    return _rn32(x)


def _is_residual_tie(a, b, c):
    """the f64 sum s of the exact product and c is a midpoint of two neighbouring f32 values (or M)
    while the exact sum is not s: the case fma32 corrects"""
    s = a * b + c  # Python floats: p exact, one f64 rounding
    if not math.isfinite(s) or s == 0:
        return False
    x = Fraction(a) * Fraction(b) + Fraction(c)
    fs = Fraction(s)
    if x == fs:
        return False
    m = abs(fs)
    e = m.numerator.bit_length() - m.denominator.bit_length()
    if Fraction(2) ** e > m:
        e -= 1
    n = m / Fraction(2) ** (max(e, -126) - 23)
    return n.denominator == 2


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


def _check(a, b, c):
    """fma32 over the arrays against _want element by element; returns the number of residual ties"""
    a, b, c = (np.asarray(x, dtype=np.float32) for x in (a, b, c))
    got = fma32(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(c))
    assert got.dtype == torch.float32
    got = got.numpy()
    want = np.array([_want(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    bad = (_bits(got) != _bits(want)) & ~nan
    assert not bad.any(), [(float(a[i]), float(b[i]), float(c[i]), float(got[i]), float(want[i]))
                           for i in np.flatnonzero(bad)[:5]]
    return sum(_is_residual_tie(float(x), float(y), float(z)) for x, y, z in zip(a, b, c))


def test_random_normals_at_three_scales():
    rng = np.random.default_rng(1)
    for scale in (1.0, 1e-20, 3e18):
        a, b, c = (rng.standard_normal(1500).astype(np.float32) for _ in range(3))
        _check(a * np.float32(scale), b * np.float32(scale), c * np.float32(scale) * np.float32(scale))
    # a product far below the addend, and the other way round
    a, b, c = (rng.standard_normal(500).astype(np.float32) for _ in range(3))
    _check(a * np.float32(1e-12), b, c)
    _check(a, b, c * np.float32(1e-12))


def test_constructed_ties_with_a_residual_on_either_side():
    """c = 1 + j 2^-23 and p = +-2^-24 (1 - 2^-36): c + p in f64 is the f32 midpoint c +- 2^-24 and
    the residual -+2^-60 decides; p = +-2^-24 (1 + 2^-17 + 2^-36) is no tie (the control)."""
    j = np.arange(512)
    c = (1.0 + j * 2.0 ** -23).astype(np.float32)
    a = np.full(512, 2.0 ** -12 * (1 + 2.0 ** -18), dtype=np.float32)
    ties = 0
    for sb in (1.0, -1.0):
        for sd in (1.0, -1.0):
            b = np.full(512, sb * 2.0 ** -12 * (1 + sd * 2.0 ** -18), dtype=np.float32)
            n = _check(a, b, c)
            assert n == (0 if sd > 0 else 512 if sb > 0 else 511)  # 1 - 2^-24 is an f32 value: j = 0 is no tie
            ties += n
    # the same around 2^k boundaries (c = 2 - 2^-23 .. and a negative c), where the neighbours' spacing changes
    for c0 in (2.0, -1.0, -2.0, 0.5):
        cc = (c0 * (1.0 + (j - 256) * 2.0 ** -23)).astype(np.float32)
        for sb in (1.0, -1.0):
            b = np.full(512, sb * abs(c0) * 2.0 ** -12 * (1 - 2.0 ** -18), dtype=np.float32)
            ties += _check(a, b, cc)
    print(f"ties of the f64 sum with a non-zero residual: {ties}")
    assert ties >= 1024 + 500  # without them nothing here tests the correction


def test_subnormal_results():
    rng = np.random.default_rng(2)
    a = rng.standard_normal(1500).astype(np.float32) * np.float32(2.0 ** -70)
    b = rng.standard_normal(1500).astype(np.float32) * np.float32(2.0 ** -70)
    c = (rng.integers(-64, 64, 1500) * 2.0 ** -149).astype(np.float32)  # subnormal addends, zeros among them
    _check(a, b, c)
    got = fma32(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(c))
    sub = (got != 0) & (got.abs() < 2.0 ** -126)
    assert int(sub.sum()) > 1000
    # exact ties in the subnormal range: p = (k + 1/2) 2^-149
    k = np.arange(1, 257)
    a2 = ((2 * k + 1) * 2.0 ** -60).astype(np.float32)
    b2 = np.full(256, 2.0 ** -90, dtype=np.float32)
    for c2 in (0.0, -0.0, 2.0 ** -149, -(2.0 ** -149)):
        assert _check(a2, b2, np.full(256, c2, dtype=np.float32)) == 0
    # ... and ties of the f64 sum with a residual: c = (2^22 + j) 2^-149, p = +-2^-150 (1 - 2^-36)
    c3 = ((2 ** 22 + np.arange(256)) * 2.0 ** -149).astype(np.float32)
    a3 = np.full(256, 2.0 ** -75 * (1 + 2.0 ** -18), dtype=np.float32)
    for sb in (1.0, -1.0):
        assert _check(a3, np.full(256, sb * 2.0 ** -75 * (1 - 2.0 ** -18), dtype=np.float32), c3) == 256
    # half the smallest subnormal, and a hair more: +0 and 2^-149
    _check([2.0 ** -75, 2.0 ** -75 * (1 + 2.0 ** -23), -(2.0 ** -75)], [2.0 ** -75, 2.0 ** -75, 2.0 ** -75], [0.0, 0.0, 0.0])


def test_exact_cancellation_and_the_sign_of_zero():
    rng = np.random.default_rng(3)
    a = rng.standard_normal(300).astype(np.float32)
    b = np.float32(2.0) ** rng.integers(-20, 20, 300).astype(np.float32)  # a b is an f32 value
    c = -(a * b)
    _check(a, b, c)
    got = fma32(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(c))
    assert np.array_equal(_bits(got.numpy()), np.zeros(300, np.uint32))  # +0, the sign bit clear
    z = [0.0, -0.0]
    abc = [(x, y, w) for x in z + [1.5, -1.5] for y in z for w in z]
    _check(*zip(*abc))
    got = fma32(torch.tensor([-0.0, 0.0, -0.0]), torch.tensor([1.5, 1.5, -1.5]), torch.tensor([-0.0, -0.0, -0.0]))
    assert _bits(got.numpy()).tolist() == [0x80000000, 0, 0]


def test_results_that_overflow():
    rng = np.random.default_rng(4)
    a = rng.standard_normal(600).astype(np.float32) * np.float32(2e19)
    b = rng.standard_normal(600).astype(np.float32) * np.float32(2e19)
    with np.errstate(over="ignore"):
        c = rng.standard_normal(600).astype(np.float32) * np.float32(3e38)  # inf among them
    _check(a, b, c)
    got = fma32(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(c))
    assert bool((got == math.inf).any()) and bool((got == -math.inf).any()) and bool(torch.isfinite(got).any())
    # around the largest finite f32 F and the midpoint M = 2^128 - 2^103 = 18631 x 1801 x 2^103 above it
    F, t = float(np.finfo(np.float32).max), 2.0 ** -100
    cases = [(18631.0, 1801.0 * 2.0 ** 103, w) for w in (0.0, t, -t, 2.0 ** 80, -(2.0 ** 80))]
    cases += [(-18631.0, 1801.0 * 2.0 ** 103, w) for w in (0.0, t, -t)]
    cases += [(F, 1.0, w) for w in (2.0 ** 102, 2.0 ** 103, 2.0 ** 102 * (1 + 2.0 ** -23), -(2.0 ** 102))]
    _check(*zip(*cases))
    got = fma32(*(torch.tensor(x, dtype=torch.float32) for x in zip(*cases[:3])))
    assert got.tolist() == [math.inf, math.inf, F]  # M itself and above: inf; a hair below: F


def test_inf_and_nan_addends():
    inf, nan = math.inf, math.nan
    cases = [(1.5, 2.0, inf), (1.5, 2.0, -inf), (1.5, 2.0, nan), (inf, 2.0, 1.0), (inf, 2.0, -inf), (inf, 0.0, 1.0),
             (nan, 1.0, 1.0), (-inf, -2.0, inf), (3e38, 3e38, -inf), (3e38, 3e38, inf), (0.0, 1.0, inf)]
    _check(*zip(*cases))
    got = fma32(*(torch.tensor(x, dtype=torch.float32) for x in zip(*cases)))
    assert torch.isnan(got).tolist() == [False, False, True, False, True, True, True, False, False, False, False]


def test_chain32_folds_in_order_from_plus_zero():
    rng = np.random.default_rng(5)
    zs = [torch.from_numpy(rng.standard_normal(200).astype(np.float32)) for _ in range(9)]
    coefs = (rng.standard_normal(9) * 3).tolist()
    got = chain32(coefs, iter(zs)).numpy()
    for i in range(200):
        acc = 0.0
        for c, z in zip(coefs, zs):
            acc = _want(float(f32(c)), float(z[i]), acc)
        assert _bits(got[i]) == _bits(acc)
    assert chain32([], []) is None
    one = chain32([-2.0], [torch.tensor([0.0, -0.0, 1.0])])  # fma(c, z, +0): a -0 product becomes +0
    assert _bits(one.numpy()).tolist() == [0, 0, 0xC0000000]
    big = chain32([1e39], [torch.tensor([1.0, -1.0, 0.0])])  # (float)1e39 is inf
    assert big[0] == math.inf and big[1] == -math.inf and bool(torch.isnan(big[2]))
