"""CPU: the restatements of the exact-posterior family (tests/_exact_ref.py, _exact_paired_ref.py, _exact_compare_ref.py,
_exact_delta_ref.py) over the eligible domain's sweep, against the closed forms of tests/_exact_domain.py (its docstring
carries the derivations), at the project's tolerances: MEAN_TOL, QUANT_TOL at PROBS, C at the two extreme draws
p = 2^-33 and 1 - 2^-33.  The device is held to the same restatements bit for bit, and to the same closed forms directly, in
tests/test_gpu_exact_domain.py.
"""
import numpy as np
import pytest

import _exact_domain as D
from _exact_compare_ref import ZS, compare
from _exact_delta_ref import PROBS as DELTA_PROBS
from _exact_delta_ref import search, single_cdf
from _exact_paired_ref import PairedPosterior, PairedStats
from _exact_ref import Posterior, Stats
from test_exact_compare_ref import H_TOL, mp_H
from test_exact_delta_ref import C, EPS_H_SINGLE, _assert_bracketed, _bracket_points
from test_exact_ref import MEAN_TOL, PROBS, QUANT_TOL

assert (MEAN_TOL, QUANT_TOL, PROBS, C) == (D.MEAN_TOL, D.QUANT_TOL, D.PROBS, D.C_EXTREME)

EQ = D.eq_cases()
EQ_PARTS = 3
C0_PARTS = 2
PAIRS = D.compare_pairs()


@pytest.fixture(scope="module")
def post(orc):
    return Posterior(orc)


@pytest.fixture(scope="module")
def ppost(orc):
    return PairedPosterior(orc)


def restated(post, cases):
    """(means [n, 2], icdf [n, 7, 2]) of single-end cases"""
    means, icdf = [], []
    for c in cases:
        tab = post.tabulate(Stats(*D.row7(c)))
        means.append([tab["mean0"], tab["mean1"]])
        icdf.append(post.icdf(tab, D.ALL_PROBS))
    return np.array(means), np.array(icdf)


def restated_paired(ppost, pcases):
    means, icdf = [], []
    for pc in pcases:
        tab = ppost.tabulate(PairedStats(*pc[1:8]))
        means.append([tab["mean0"], tab["mean1"]])
        icdf.append(ppost.icdf(tab, D.ALL_PROBS))
    return np.array(means), np.array(icdf)


@pytest.mark.parametrize("part", range(EQ_PARTS))
def test_equal_lengths_against_the_beta_law(post, part):
    cases = EQ[part::EQ_PARTS]
    means, icdf = restated(post, cases)
    D.assert_eq("EQ", cases, means, icdf)
    assert np.abs(means.sum(axis=1) - 1.0).max() < 1e-14 and np.abs(icdf.sum(axis=2) - 1.0).max() <= 1e-15


def test_scipy_against_mpmath_where_mpmath_converges(post):
    """the double-precision reference itself, at the restated quantile points of every sweep case small enough for mpmath:
    1e-10 relative keeps its share of a quantile's error below 1e-10 p / pdf, four orders under QUANT_TOL"""
    small = [c for c in EQ + [c for r in D.RATIOS for c in D.c0_cases(r)] if max(c[0] + c[5], c[1] + c[6]) <= D.MP_LIMIT]
    assert len(small) >= 100
    seen, worst, points = set(), (0.0, None), 0
    for c in small:
        a, b = c[0] + c[5], c[1] + c[6]
        if (a, b) in seen:
            continue
        seen.add((a, b))
        eq = (0, 0, 0, 1.0, 1.0, a, b)          # Beta(a, b) itself
        _, icdf = restated(post, [eq])
        d, done = D.mp_cross_check(a, b, icdf[0, :, 0], icdf[0, :, 1], D.ALL_PROBS)
        points += done
        worst = (d, (a, b)) if d > worst[0] else worst
    print("scipy against mpmath: worst relative difference %.3g at (a, b) = %s; %d laws, mpmath converged at %d of %d points"
          % (worst + (len(seen), points, 7 * len(seen))))
    assert worst[0] < 1e-10 and points >= 0.9 * 7 * len(seen)


@pytest.mark.parametrize("part", range(C0_PARTS))
@pytest.mark.parametrize("ratio", D.RATIOS, ids=lambda r: "ratio%.3g" % r)
def test_unequal_lengths_against_the_substituted_beta_law(post, ratio, part):
    cases = D.c0_cases(ratio)[part::C0_PARTS]
    means, icdf = restated(post, cases)
    D.assert_c0("C0 e0/e1 = %g" % ratio, cases, icdf)
    assert np.abs(means.sum(axis=1) - 1.0).max() < 1e-14


def test_unequal_lengths_means(post):
    cases = D.c0_mean_cases()
    means, icdf = restated(post, cases)
    D.assert_c0("C0 mean cases", cases, icdf)
    for c, m in zip(cases, means):
        want = D.c0_mean(c)
        print("C0 mean %s: %.17g, error %.3g" % (D.case_id(c), m[0], m[0] - want))
        assert abs(m[0] - want) < MEAN_TOL and abs(m[1] - (1.0 - want)) < MEAN_TOL, c


@pytest.mark.parametrize("pcase", D.ratio_cases(), ids=lambda pc: pc[0])
def test_paired_ratio_family(post, ppost, pcase):
    """the pairs' factors cancel: the paired restatement against the single-end restatement of the equivalent event (each
    within one tolerance of the truth, so within two of each other) and against mpmath's quadrature of that event"""
    means, icdf = restated_paired(ppost, [pcase])
    smeans, sicdf = restated(post, [pcase[8]])
    assert np.abs(means - smeans).max() < 2 * MEAN_TOL
    assert np.abs(icdf[0, :5] - sicdf[0, :5]).max() < 2 * QUANT_TOL and np.abs(icdf[0, 5:] - sicdf[0, 5:]).max() < 2 * C
    D.assert_ratio(pcase, means[0], icdf[0])


def test_paired_constant_factors_against_the_beta_law(ppost):
    pcases = D.peq_cases()
    means, icdf = restated_paired(ppost, pcases)
    D.assert_eq("PEQ / PMIN", [pc[8] for pc in pcases], means, icdf)


# ---- comparisons ----
_cmp = {}


def compared(post, name):
    if name not in _cmp:
        _, c1, c2 = next(p for p in PAIRS if p[0] == name)
        r1, r2 = D.row7(c1), D.row7(c2)
        H = single_cdf(post, r1, r2)
        _cmp[name] = (compare(post, r1, r2, ZS), search(H, DELTA_PROBS), H, (r1, r2))
    return _cmp[name]


@pytest.mark.parametrize("name", [p[0] for p in PAIRS])
def test_log_density_at_zero_closed_form(post, name):
    got = compared(post, name)[0]
    _, c1, c2 = next(p for p in PAIRS if p[0] == name)
    D.assert_log_d0(name, c1, c2, got[2])
    a1, b1, a2, b2 = c1[0] + c1[5], c1[1] + c1[6], c2[0] + c2[5], c2[1] + c2[6]
    assert abs(got[0] - a1 / (a1 + b1)) < MEAN_TOL and abs(got[1] - a2 / (a2 + b2)) < MEAN_TOL


@pytest.mark.parametrize("name", [p[0] for p in PAIRS])
def test_cdf_of_the_difference_and_its_quantiles(post, name):
    got, q, H, rows = compared(post, name)
    want = mp_H(rows, list(H.tabs), ZS)
    errs = [abs(g - w) for g, w in zip(got[5:], want)]
    print("%s: H %s, errors %s" % (name, ["%.7f" % g for g in got[5:]], ["%.2g" % e for e in errs]))
    assert max(errs) <= H_TOL
    D.assert_pair_shape(name, got[5:][ZS.index(0.0)], q)
    _assert_bracketed(q[:3], mp_H(rows, list(H.tabs), _bracket_points(q[:3])), EPS_H_SINGLE, name)


# ---- beyond the fence (host code: no device is needed) ----

@pytest.mark.parametrize("hyper", [(1.0, 1e20), (1e30, 1.0)], ids=["h1e20", "h1e30"])
def test_the_inputs_that_gave_garbage_are_refused(hyper):
    """(5, 5, 0, 100, 100) under h = (1, 1e20) returned a mean of 9.5e-17 for 6e-20, under h = (1e30, 1) NaN"""
    from miso_amd import InternalError, capi
    el = capi.C.c_int(-1)
    assert capi.lib().miso_exact_eligible(0, 2, capi._p(np.array([100.0, 100.0])), capi._p(np.array(hyper)), capi.C.byref(el)) == 0
    assert el.value == 0
    assert capi.lib().miso_exact_paired_eligible(2, capi._p(np.array([100.0, 100.0])), capi._p(np.array(hyper)), 0, capi.C.byref(el)) == 0
    assert el.value == 0
    with pytest.raises(InternalError, match="not eligible"):
        capi.selftest_exact([[5, 5, 10, 100, 100, hyper[0], hyper[1]]], [0.5])
