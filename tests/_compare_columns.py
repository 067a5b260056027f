"""The column pairs tests/test_gpu_compare_exact.py gives compare_kernel, built without looking at any result of it
(tests/test_compare_exact_ref.py checks on the CPU that each is what its name says).  Test infrastructure only."""
from fractions import Fraction

import numpy as np

SAMPLE_COUNTS = (2, 3, 257, 8192, 8193, 20000)
THRESHOLD = Fraction(0.009)              # the double the kernel (and the reference program) compares with


# ---- columns: name -> (u, v), the device forms d = fl(u - v) ----
def _two_point(S, c, w):
    """d_i = c + w or c - w in turn (u = 0.5 + d_i, v = 0.5: the subtraction rounds)"""
    d = c + w * np.where(np.arange(S) % 2 == 0, 1.0, -1.0)
    return 0.5 + d, np.full(S, 0.5)


def _width_for(S, c, log_post):
    """w with log(density at 0) = log_post for the two-point column at smoothing 0.3, by bisection in double
    arithmetic on the dominant term (the exact value is checked by the caller): narrower = further from 0"""
    def log_density(w):
        u, v = _two_point(S, c, w)
        d = u - v
        cov = np.var(d, ddof=1) * 0.09
        x = -(d * d) / (2 * cov)
        return float(x.max() + np.log(np.sum(np.exp(x - x.max()))) - np.log(S * np.sqrt(2 * np.pi * cov)))
    lo, hi = 1e-4 * c, 0.9 * c
    assert log_density(lo) < log_post < log_density(hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if log_density(mid) < log_post:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def columns(S, rng):
    col = {}
    col["random psi"] = (rng.random(S), rng.random(S))
    col["close psi"] = (0.4 + 0.2 * rng.random(S), 0.45 + 0.2 * rng.random(S))
    dy = rng.integers(16, 64, S) / 64.0
    col["all 0.25"] = (dy, dy - 0.25)                                  # dyadic: every difference is 0.25 exactly
    one = dy - 0.25
    one[S // 2] = dy[S // 2] - 0.5
    col["all 0.25 but one"] = (dy, one)
    # |d_i| = 0.009 -+ (1, 2, 3) x 2^-40 in turn, signs alternating: the mean is 1e-12 and more off 0.009
    step = (1 + np.arange(S) % 3) * 2.0 ** -40
    sign = np.where(np.arange(S) % 2 == 0, 1.0, -1.0)
    col["mad just under"] = (0.5 + sign * (0.009 - step), np.full(S, 0.5))
    col["mad just over"] = (0.5 + sign * (0.009 + step), np.full(S, 0.5))
    if S > 3:        # (two or three points: the sample variance is not the two-point law's, the target is not met)
        col["density subnormal"] = _two_point(S, 1.0, _width_for(S, 1.0, -315 * np.log(10.0)))
        col["density zero"] = _two_point(S, 1.0, _width_for(S, 1.0, -345 * np.log(10.0)))
        col["just under the cap"] = _two_point(S, 1.0, _width_for(S, 1.0, -12 * np.log(10.0) + 1e-9))
        col["just over the cap"] = _two_point(S, 1.0, _width_for(S, 1.0, -12 * np.log(10.0) - 1e-9))
    v = rng.random(S)
    v[S // 3] = np.nan
    col["nan in one column"] = (rng.random(S), v)
    return col


def exact_mean_abs(d):
    return sum(abs(Fraction(float(x))) for x in d) / len(d)
