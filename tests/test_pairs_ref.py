"""CPU: the two restatements of the all-pairs comparison (tests/_pairs_ref.py) agree with each other, keep the
definition's symmetries, and estimate what they are meant to estimate.  The GPU tests
(tests/test_gpu_compare_pairs.py) hold the kernel to these restatements bit for bit."""
import math

import numpy as np
import pytest

import _pairs_ref as PR

SMALL = [(2, 2, 0.5), (2, 2, 0.95), (3, 5, 0.95), (64, 64, 0.95), (255, 257, 0.9), (256, 256, 0.95), (1000, 450, 0.95),
         (4097, 300, 0.95)]
TAUS = (0.05, 0.2, 0.25, 0.5)


def test_ranks():
    assert PR.ranks(4, 0.5) == (1, 0, 2)
    assert PR.ranks(4, 0.95) == (1, 0, 3)          # floor(0.1 + 0.5) - 1 = -1: the clamp
    assert PR.ranks(1, 0.95) == (0, 0, 0)
    assert PR.ranks(8192 * 8192, 0.95) == ((8192 * 8192 - 1) // 2, 1677721, 65431141)
    assert PR.ranks(25_000_000, 0.95) == (12_499_999, 624_999, 24_374_999)


@pytest.mark.parametrize("kind", PR.KINDS)
@pytest.mark.parametrize("S1,S2,level", SMALL)
def test_bisect_is_brute(kind, S1, S2, level):
    a, b = PR.columns(kind, S1, S2)
    steps = []
    x, y = PR.brute(a, b, level, TAUS), PR.bisect(a, b, level, TAUS, steps_out=steps)
    assert PR.same(x, y), (x, y)
    assert max(steps) <= 64


def test_key_round_trip_and_order():
    v = [-np.inf, -1.0, -1e-300, -5e-324, -0.0, 0.0, 5e-324, 0.1, 1.0, np.inf]
    k = [PR._key(x) for x in v]
    assert k == sorted(k) and len(set(k)) == len(k)
    assert PR.bits([PR._value(x) for x in k]).tolist() == PR.bits(v).tolist()


@pytest.mark.parametrize("kind", PR.KINDS)
def test_swapping_the_samples(kind):
    a, b = PR.columns(kind, 301, 97)
    med, lo, hi, gt, lt, ge, fin, M = PR.brute(a, b, 0.9, TAUS)
    med2, lo2, hi2, gt2, lt2, ge2, fin2, M2 = PR.brute(b, a, 0.9, TAUS)
    # the swapped differences are the negated ones: the order statistic at rank r is minus the one at rank M - 1 - r.  (The
    # summaries' rule puts lo at floor(x + 0.5) - 1 and hi at M - 1 - ceil(x - 0.5), x = M alpha / 2: one rank apart from
    # mirror images of each other unless x - 0.5 is an integer or the clamp acts, as below.)
    d = np.sort(np.subtract.outer(a, b).ravel())
    r_med, r_lo, r_hi = PR.ranks(M, 0.9)
    assert PR.bits([med2, lo2, hi2]).tolist() == PR.bits([-d[M - 1 - r_med] + 0.0, -d[M - 1 - r_lo] + 0.0, -d[M - 1 - r_hi] + 0.0]).tolist()
    assert (gt2, lt2, ge2, M2) == (lt, gt, ge, M)
    # mirrored ranks: the bounds swap and change sign
    a4, b4 = a[:2], b[:2]
    assert PR.ranks(4, 0.95)[1:] == (0, 3)
    x, y = PR.brute(a4, b4, 0.95), PR.brute(b4, a4, 0.95)
    assert PR.bits([y[1], y[2]]).tolist() == PR.bits([-x[2] + 0.0, -x[1] + 0.0]).tolist()
    zeros = M - gt - lt
    assert zeros == int((np.subtract.outer(a, b) == 0).sum())


def test_identical_constant_columns():
    x = PR.brute(np.full(40, 0.3), np.full(33, 0.3), 0.95, (0.1,))
    assert x[:3] == (0.0, 0.0, 0.0) and PR.bits(x[:3]).tolist() == [0, 0, 0]
    assert x[3:] == (0, 0, [0], True, 40 * 33)
    assert PR.same(x, PR.bisect(np.full(40, 0.3), np.full(33, 0.3), 0.95, (0.1,)))


def test_the_decimal_rounding_artefact_is_kept():
    """0.3 - 0.1 is the double below 0.2: such a pair is not counted in |d| >= 0.2; a dyadic threshold is met exactly."""
    assert PR.brute([0.3], [0.1], 0.5, (0.2,))[5] == [0]
    assert PR.bisect([0.3], [0.1], 0.5, (0.2,))[5] == [0]
    assert PR.brute([0.75], [0.5], 0.5, (0.25,))[5] == [1]
    assert PR.brute([0.5], [0.75], 0.5, (0.25,))[5] == [1]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_not_finite(bad):
    a, b = PR.columns("uniform", 9, 7)
    b[3] = bad
    for f in (PR.brute, PR.bisect):
        for x in (f(a, b, 0.9, (0.2,)), f(b, a, 0.9, (0.2,))):
            assert all(math.isnan(v) for v in x[:3]) and x[3:] == (0, 0, [0], False, 63)


def test_refusals():
    assert PR.refusal(8192, 8192, 0.95, (0.1, 0.2, 0.3, 0.4)) is None
    assert "Too many samples" in PR.refusal(8193, 10, 0.95, ())
    assert "Too many samples" in PR.refusal(10, 8193, 0.95, ())
    assert "number of delta psi thresholds" in PR.refusal(10, 10, 0.95, (0.1,) * 5)
    assert "threshold" in PR.refusal(10, 10, 0.95, (1.0,)) and "threshold" in PR.refusal(10, 10, 0.95, (0.0,))
    assert "confidence" in PR.refusal(10, 10, 1.0, ()) and "confidence" in PR.refusal(10, 10, 0.0, ())


# ---- against the truth: two Beta posteriors
def _truth(p1, p2, tau):
    """P(|x - y| >= tau), x ~ Beta(p1), y ~ Beta(p2), by quadrature over x of x's density times y's tail masses"""
    import mpmath as mp
    mp.mp.dps = 25
    (a1, b1), (a2, b2) = p1, p2
    cdf2 = lambda v: mp.betainc(a2, b2, 0, min(max(v, 0), 1), regularized=True)
    pdf1 = lambda x: x ** (a1 - 1) * (1 - x) ** (b1 - 1) / mp.beta(a1, b1)
    f = lambda x: pdf1(x) * (cdf2(x - tau) + 1 - cdf2(x + tau))
    return float(mp.quad(f, [0, tau, 1 - tau, 1]))


BETAS = [((30, 12), (18, 22), 0.2), ((8, 3), (9, 3), 0.1), ((50, 50), (60, 40), 0.2)]


@pytest.fixture(scope="module")
def truths():
    return [_truth(*c) for c in BETAS]


def test_truth_by_two_routes():
    """the quadrature against a closed form: uniform posteriors, P(|x - y| >= tau) = (1 - tau)^2"""
    assert abs(_truth((1, 1), (1, 1), 0.2) - 0.64) < 1e-12


@pytest.mark.parametrize("S1,S2", [(500, 500), (1000, 450), (2000, 2000)])
def test_all_pairs_estimate_within_five_sigma(S1, S2, truths):
    """|n_abs_ge / M - P| <= 5 sqrt((S1 + S2 - 1) / (4 S1 S2)): the variance of a two-sample U-statistic of an indicator
    is at most ((S2 - 1) z10 + (S1 - 1) z01 + z11) / (S1 S2) with every zeta <= 1/4"""
    bound = 5 * math.sqrt((S1 + S2 - 1) / (4.0 * S1 * S2))
    for ci, ((p1, p2, tau), P) in enumerate(zip(BETAS, truths)):
        rng = np.random.default_rng(1000 + ci)
        a, b = rng.beta(*p1, S1), rng.beta(*p2, S2)
        x = PR.bisect(a, b, 0.95, (tau,))
        est = x[5][0] / x[7]
        print("case %d S %d x %d: all pairs %.6f truth %.6f bound %.6f" % (ci, S1, S2, est, P, bound))
        assert abs(est - P) <= bound


def test_all_pairs_beat_the_index_pairing(truths):
    """S = 500, 200 seeds: the all-pairs fraction is closer to the truth than the index-paired one, on average"""
    S = 500
    for ci, ((p1, p2, tau), P) in enumerate(zip(BETAS, truths)):
        e_all, e_idx = [], []
        for seed in range(200):
            rng = np.random.default_rng([seed, ci])
            a, b = rng.beta(*p1, S), rng.beta(*p2, S)
            bs = np.sort(b)
            n = (S * S - PR._count(a, bs, tau, strict=True)) + PR._count(a, bs, -tau)
            e_all.append(abs(n / (S * S) - P))
            e_idx.append(abs(float((np.abs(a - b) >= tau).mean()) - P))
        print("case %d: mean |error| all pairs %.5f, index-paired %.5f" % (ci, np.mean(e_all), np.mean(e_idx)))
        assert np.mean(e_all) < np.mean(e_idx)
