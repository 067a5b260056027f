"""CPU: the columns of tests/test_gpu_compare_exact.py are what their names say, by exact arithmetic, and the 50-digit
restatement (_compare_ref.exact_comparison) agrees with the numpy one where double precision suffices."""
from fractions import Fraction

import mpmath
import numpy as np
import pytest

from _compare_columns import SAMPLE_COUNTS, THRESHOLD, columns, exact_mean_abs
from _compare_ref import bayes_factor, density_error_bound, device_mean_abs, exact_comparison, summation_depth


def test_threshold_columns_are_on_their_side_of_0009_by_1e_12():
    """CPU arithmetic only: the exact rational mean|delta| of the threshold columns, and the three statements' branch"""
    for S in SAMPLE_COUNTS:
        col = columns(S, np.random.default_rng(S))
        for name, side in (("mad just under", -1), ("mad just over", 1)):
            u, v = col[name]
            d = u - v
            off = exact_mean_abs(d) - THRESHOLD
            assert off * side >= Fraction(1, 10 ** 12) and abs(off) < Fraction(1, 10 ** 11), (S, name, float(off))
            assert (device_mean_abs(d) <= 0.009) == (side < 0) == (float(np.mean(np.abs(d))) <= 0.009)
            assert bool(exact_comparison(d)["null_peaked"]) == (side < 0)
            assert not np.all(d == d[0])


@pytest.mark.parametrize("S", [257, 8193])
def test_built_cases_are_what_they_claim_by_the_exact_reference(S):
    col = columns(S, np.random.default_rng(S))
    ex = {n: exact_comparison(col[n][0] - col[n][1]) for n in ("density subnormal", "density zero", "just under the cap",
                                                               "just over the cap", "all 0.25", "all 0.25 but one")}
    assert 2.0 ** -1060 < ex["density subnormal"]["post"] < 2.0 ** -1022
    assert ex["density zero"]["post"] < mpmath.mpf(2) ** -1100
    assert 1e12 * (1 - 1e-8) < ex["just under the cap"]["bf"] < 1e12 < ex["just over the cap"]["bf"] < 1e12 * (1 + 1e-8)
    # the cap cases sit further from 1e12 than twice the error bound: the device's side is decided
    for n in ("just under the cap", "just over the cap"):
        rel = 2 * (density_error_bound(S, ex[n]["amplification"]) + 2.0 ** -53)
        assert rel < 1e-11 and abs(float(ex[n]["bf"] / 1e12 - 1)) > 10 * rel
    assert ex["all 0.25"]["all_same"] and ex["all 0.25"]["null_peaked"] and ex["all 0.25"]["mad"] == 0.25
    assert not ex["all 0.25 but one"]["null_peaked"]


def test_exact_restatement_agrees_with_the_numpy_one_and_the_bound_is_what_the_docstring_derives():
    rng = np.random.default_rng(8)
    for S, factor in ((2, 0.3), (3, 0.5), (257, 0.3), (1000, 0.05)):
        u, v = rng.random(S), rng.random(S)
        ebf, edens = bayes_factor(u, v, factor)
        ex = exact_comparison(u - v, factor)
        assert abs(float(ex["post"]) - edens) <= 1e-12 * edens + 1e-300
        assert ex["amplification"] >= 0
    assert summation_depth(2) == 9 and summation_depth(256) == 9 and summation_depth(257) == 10 and summation_depth(20000) == 87
    u = 2.0 ** -53
    D = 10
    assert density_error_bound(257, 3.0) == 3.0 * ((D + 7) * u + 3 * u) + (2 + D) * u + ((D + 7) * u + 2 * u) / 2 + 4 * u
