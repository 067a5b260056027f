"""CPU: the restatement of the quantiles of delta psi from the exact CDF (tests/_exact_delta_ref.py)
against mpmath, on the pair list of the single-end comparison and the case list of the paired-end one, both under both
hyperparameter pairs, at p = 0.025, 0.5 and 0.975.

The criterion brackets the quantile instead of inverting the reference: with H_mp the CDF of psi_1 - psi_2 as the two
comparisons' own mpmath references compute it (tests/test_exact_compare_ref.py mp_H, tests/test_exact_paired_compare_ref.py
mp_H),
    H_mp(q - c) - eps_H <= p <= H_mp(q + c) + eps_H,
c = 5e-5 (half a unit of the fourth printed decimal; the arguments clipped to (-1, 1)) and eps_H the bound those tests assert
for the restated H itself: 5e-6 single-end, 3e-6 paired-end.  No case is left out; the 10^5-pair paired case runs all three
probabilities like the others (the reference's cost depends on its distinct pairs, two).
"""
import mpmath as mp
import numpy as np
import pytest

from _exact_compare_ref import HYPERS, PAIRS, compare, pair_rows
from _exact_delta_ref import PROBS, ROUNDS, paired_cdf, search, single_cdf
from _exact_paired_compare_ref import PairedCompare, cases, paired_stats
from _exact_ref import Posterior
from test_exact_compare_ref import H_TOL as EPS_H_SINGLE
from test_exact_compare_ref import mp_H as mp_H_single
from test_exact_paired_compare_ref import TOL_H as EPS_H_PAIRED
from test_exact_paired_compare_ref import MpSample
from test_exact_paired_compare_ref import mp_H as mp_H_paired

C = 5e-5
INSIDE = 1.0 - 1e-9         # the clip of q -+ c to (-1, 1)
assert EPS_H_SINGLE == 5e-6 and EPS_H_PAIRED == 3e-6 and ROUNDS == 5
COMBOS = [(p, h) for h in HYPERS for p in PAIRS]
COMBO_IDS = ["%s|%s|%s-h%g_%g" % (",".join(map(str, p[0])), ",".join(map(str, p[1])), ",".join(map(str, p[2])), h[0], h[1])
             for p, h in COMBOS]
CASES = cases()
PCOMBOS = [(c, h) for h in HYPERS for c in CASES]
PCOMBO_IDS = ["%s-h%g_%g" % (c[0], h[0], h[1]) for c, h in PCOMBOS]
_cache = {}


@pytest.fixture(scope="module")
def post(orc):
    return Posterior(orc)


@pytest.fixture(scope="module")
def ppost(orc):
    return PairedCompare(orc)


def single_result(post, pair, hyper, swapped=False):
    """(the restatement's [q ..., H0], its CDF) of a pair, made once"""
    key = ("s", pair, hyper, swapped)
    if key not in _cache:
        r1, r2 = pair_rows(pair, hyper)
        H = single_cdf(post, r2, r1) if swapped else single_cdf(post, r1, r2)
        _cache[key] = (search(H, PROBS), H)
    return _cache[key]


def paired_result(ppost, case, hyper, swapped=False):
    key = ("p", case[0], hyper, swapped)
    if key not in _cache:
        ps1, ps2 = paired_stats(case[1], hyper), paired_stats(case[2], hyper)
        H = paired_cdf(ppost, ps2, ps1) if swapped else paired_cdf(ppost, ps1, ps2)
        _cache[key] = (search(H, PROBS), H)
    return _cache[key]


def _bracket_points(q):
    zs = []
    for v in q:
        zs += [min(max(float(v) - C, -INSIDE), INSIDE), min(max(float(v) + C, -INSIDE), INSIDE)]
    return zs


def _assert_bracketed(q, want, eps, what):
    for k, p in enumerate(PROBS):
        below, above = float(want[2 * k]), float(want[2 * k + 1])
        print("%s p %.3f: q %.9f, H_mp(q - c) %.9f, H_mp(q + c) %.9f" % (what, p, q[k], below, above))
        assert below - eps <= p <= above + eps, (what, p, q[k], below, above)


@pytest.mark.parametrize("pair,hyper", COMBOS, ids=COMBO_IDS)
def test_single_end_quantiles_against_mpmath(post, pair, hyper):
    res, H = single_result(post, pair, hyper)
    assert H.evaluations <= 1 + 8 + 32 * len(PROBS)
    rows = pair_rows(pair, hyper)
    want = mp_H_single(rows, list(H.tabs), _bracket_points(res[:3]))
    _assert_bracketed(res[:3], want, EPS_H_SINGLE, (pair, hyper))


@pytest.mark.parametrize("case,hyper", PCOMBOS, ids=PCOMBO_IDS)
def test_paired_end_quantiles_against_mpmath(ppost, case, hyper):
    res, H = paired_result(ppost, case, hyper)
    assert H.evaluations <= 1 + 8 + 32 * len(PROBS)
    m1, m2 = MpSample(case[1], hyper, H.tabs[0]), MpSample(case[2], hyper, H.tabs[1])
    want = mp_H_paired(m1, m2, H.a_is_2, _bracket_points(res[:3]))
    _assert_bracketed(res[:3], want, EPS_H_PAIRED, (case[0], hyper))


def _assert_shape(res, swapped, what):
    q = dict(zip(PROBS, res[:3]))
    qs = dict(zip(PROBS, swapped[:3]))
    assert q[0.025] <= q[0.5] <= q[0.975], what                       # non-decreasing in p
    for p, other in ((0.5, 0.5), (0.025, 0.975), (0.975, 0.025)):      # the swap gives -q(1 - p)
        assert abs(qs[p] + q[other]) <= 2 * C, (what, p, qs[p], q[other])
    assert 0.0 <= res[3] <= 1.0 and abs((1.0 - swapped[3]) - res[3]) <= 1e-5, (what, res[3], swapped[3])


@pytest.mark.parametrize("hyper", HYPERS, ids=lambda h: "h%g_%g" % h)
def test_single_end_monotone_swap_and_cdf_at_zero(post, hyper):
    for pair in PAIRS:
        res, _ = single_result(post, pair, hyper)
        swapped, _ = single_result(post, pair, hyper, swapped=True)
        _assert_shape(res, swapped, pair)
        # H0 is the comparison's own H(0.0), bit for bit
        assert res[3] == compare(post, *pair_rows(pair, hyper), zs=[0.0])[5], pair


@pytest.mark.parametrize("hyper", HYPERS, ids=lambda h: "h%g_%g" % h)
def test_paired_end_monotone_swap_and_cdf_at_zero(ppost, hyper):
    for case in CASES:
        res, _ = paired_result(ppost, case, hyper)
        swapped, _ = paired_result(ppost, case, hyper, swapped=True)
        _assert_shape(res, swapped, case[0])
        got, _ = ppost.compare(paired_stats(case[1], hyper), paired_stats(case[2], hyper), [0.0])
        assert res[3] == got[5], case[0]


def test_search_on_a_known_cdf():
    """the bracket's update and the interpolation on a CDF with a closed form: the uniform law on (-1, 1), where the linear
    interpolation is exact, and a step, where the first point at or above p closes the bracket"""
    q = search(lambda z: (np.float64(z) + 1.0) / 2.0, [0.025, 0.5, 0.975])
    assert np.abs(q[:3] - np.array([-0.95, 0.0, 0.95])).max() <= 1e-15 and q[3] == 0.5
    step = search(lambda z: np.float64(0.0 if z < 0.25 else 1.0), [0.5])
    assert abs(step[0] - 0.25) <= 2.0 / 9 ** ROUNDS and step[1] == 0.0
