"""The doubles on which the device's "%.4f" rounding (csrc/text_digits.hpp) is checked, and the reference for it: the digits
Python's "%.4f" prints, as a signed integer.  Test infrastructure only."""
from decimal import ROUND_HALF_EVEN, Decimal

import numpy as np

# The doubles that csrc/text_digits.hpp rounded one digit off before it decided |p - r| = 0.5 by the sign of the
# product's rounding error: the nearest double to each, found by restating the routine on the CPU.
TIE_NEIGHBOURS = (5e-05, 0.00025, 0.00035, 0.00095, 0.00645)


def ulp_walk(x, n):
    """x and its n neighbours to either side"""
    x = np.asarray(x, dtype=np.float64)
    out = [x]
    lo = hi = x
    for _ in range(n):
        lo = np.nextafter(lo, -np.inf)
        hi = np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


def decimal_ties():
    """every (k + 0.5) / 10^4, k = 0 .. 10000, +- 6 ulps, both signs"""
    v = ulp_walk((np.arange(10001) + 0.5) / 1e4, 6)
    return np.concatenate([v, -v])


def binary_ties():
    """j / 32, j = 1 .. 64: x 10^4 is j x 312.5, a true tie for every odd j (decided to even) -- and 3 ulps around"""
    v = ulp_walk(np.arange(1, 65) / 32.0, 3)
    return np.concatenate([v, -v])


def grid():
    """every k / 10^4 +- 3 ulps (k = 0: the smallest subnormals of either sign)"""
    v = ulp_walk(np.arange(10001) / 1e4, 3)
    return np.concatenate([v, -v])


def edges():
    rng = np.random.default_rng(20250)
    tiny = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072009e-308, 2.2250738585072014e-308, -2.2250738585072014e-308,
                     1e-300, 1e-20, 4.9999999999999996e-05, 1.0, 2.0])
    big = rng.random(20000) * 2e5                                      # up to 2 x 10^5: ten digits before the rounding
    big_ties = ulp_walk((np.floor(big * 1e4) + 0.5) / 1e4, 6)
    top = ulp_walk(np.array([2e5, 199999.99995, 131072.00005, 65536.5, 99999.99995, 12345.67895]), 6)
    v = np.concatenate([tiny, big, big_ties, top])
    return np.concatenate([v, -v])


def random_unit(n=10 ** 6):
    return np.random.default_rng(20251).random(n)


def digits_by_format(v):
    """the digits of "%.4f" % v with its sign: int("-0.0065" without the point) = -65"""
    out = np.empty(len(v), np.int64)
    for i, x in enumerate(v.tolist()):
        s = "%.4f" % x
        out[i] = int(s.replace(".", ""))
    return out


def digits_by_decimal(v):
    """the same by another route: the double's exact decimal expansion quantized half-even"""
    q = Decimal("0.0001")
    return np.array([int(Decimal(x).quantize(q, rounding=ROUND_HALF_EVEN).scaleb(4)) for x in v.tolist()], dtype=np.int64)
