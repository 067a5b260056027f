"""CPU: the exact-posterior mode's numerical scheme (tests/_exact_ref.py, the kernel's restatement) against mpmath at 40
digits, against the checker's counter-mode sampler, and its eligibility rule.

The reference side is kept cheap: equal effective lengths make the posterior a Beta law (mean in closed form, CDF =
the regularised incomplete beta function); otherwise the density is integrated once piece by piece between the
restatement's own quantile points and a few split points around the mode, and the error of a quantile is
(CDF(x) - p) / pdf(x) -- one pass of quadrature per case, no root finding in high precision.
"""
import mpmath as mp
import numpy as np
import pytest

from _exact_ref import CASES, HYPERS, Posterior, Stats, case_stats, eligible
from _libs import OrcLib
from _problems import simulate_se
from miso_amd import capi

PROBS = [0.001, 0.025, 0.5, 0.975, 0.999]
MEAN_TOL = 1e-9      # posterior mean
QUANT_TOL = 1e-6     # inverse CDF, in psi: 1/50 of half a unit of the `.miso` file's fourth decimal


@pytest.fixture(scope="module")
def post(orc):
    return Posterior(orc)


def mp_errors(case, hyper, tab, t_hat):
    """(error of the mean, errors of the quantile points x(t_hat) in psi) of a tabulated posterior against mpmath"""
    mp.mp.dps = 40
    n10, n01, n11, e0, e1 = case
    a, b, n = mp.mpf(n10) + mp.mpf(hyper[0]), mp.mpf(n01) + mp.mpf(hyper[1]), mp.mpf(n10 + n01 + n11)
    e0, e1 = mp.mpf(e0), mp.mpf(e1)
    xs = [1 / (1 + mp.exp(-mp.mpf(float(t)))) for t in t_hat]
    if e0 == e1:
        mean = a / (a + b)
        errs = []
        for p, x in zip(PROBS, xs):
            cdf = mp.betainc(a, b, 0, x, regularized=True)
            pdf = mp.exp((a - 1) * mp.log(x) + (b - 1) * mp.log(1 - x) - mp.log(mp.beta(a, b)))
            errs.append(float((cdf - mp.mpf(p)) / pdf))
        return float(mp.mpf(float(tab["mean0"])) - mean), errs
    gmax = mp.mpf(float(tab["gmax"]))

    def f(t):   # the density in logit space, scaled
        em = mp.exp(-t)
        x, y = 1 / (1 + em), em / (1 + em)
        return mp.exp(a * mp.log(x) + b * mp.log(y) - n * mp.log(x * e0 + y * e1) - gmax)

    def xf(t):
        return f(t) / (1 + mp.exp(-t))
    tm, tL, tR = (mp.mpf(float(tab[k])) for k in ("tm", "tL", "tR"))
    pts = {tm - 300, tL, tm - (tm - tL) / 4, tm - (tm - tL) / 16, tm, tm + (tR - tm) / 16, tm + (tR - tm) / 4, tR, tm + 300}
    pts |= {mp.mpf(float(t)) for t in t_hat}
    pts = sorted(pts)
    cum, Z, M = {pts[0]: mp.mpf(0)}, mp.mpf(0), mp.mpf(0)
    for lo, hi in zip(pts[:-1], pts[1:]):
        Z += mp.quad(f, [lo, hi])
        M += mp.quad(xf, [lo, hi])
        cum[hi] = Z
    errs = []
    for p, t, x in zip(PROBS, t_hat, xs):
        tt = mp.mpf(float(t))
        errs.append(float((cum[tt] / Z - mp.mpf(p)) * Z * x * (1 - x) / f(tt)))
    return float(mp.mpf(float(tab["mean0"])) - M / Z), errs


@pytest.mark.parametrize("hyper", HYPERS[:2], ids=lambda h: "h%g_%g" % h)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_restatement_against_mpmath(post, case, hyper):
    tab = post.tabulate(case_stats(case, hyper))
    t_hat = post.invert(tab, np.array(PROBS) * tab["Z"])
    q = post.icdf(tab, PROBS)
    assert (np.diff(q[:, 0]) > 0).all() and np.allclose(q[:, 0] + q[:, 1], 1.0, rtol=0, atol=1e-15)
    mean_err, q_err = mp_errors(case, hyper, tab, t_hat)
    print("mean error %.3g, quantile errors %s" % (mean_err, ["%.3g" % e for e in q_err]))
    assert abs(mean_err) < MEAN_TOL
    assert max(abs(e) for e in q_err) < QUANT_TOL
    assert abs((tab["mean0"] + tab["mean1"]) - 1.0) < 1e-14


def test_restated_mean_against_counter_mode_sampler(orc, post):
    """the event of test_statistics.py::test_k2_stream_counter_and_quadrature_agree, its rule: 4 se + 2e-3"""
    exons, isoforms, g, pos, cig = simulate_se(orc, 2, 1000, seed=42)
    probe = orc.miso(g, pos, cig, 36, iters=20, burn=2, lag=1, chains=1)
    counts = {tuple(int(v) for v in t): int(c) for t, c in zip(probe.class_templates, probe.class_counts)}
    eff = [int(n) - 36 + 1 for n in orc.isolength(g)]
    n10, n01, n11 = counts.get((1, 0), 0), counts.get((0, 1), 0), counts.get((1, 1), 0)
    tab = post.tabulate(Stats(n10, n01, n10 + n01 + n11, eff[0], eff[1], 1.0, 1.0))
    means = np.array([orc.miso(g, pos, cig, 36, iters=4000, burn=1000, lag=1, chains=1, mode=OrcLib.COUNTER,
                               seed=500 + s, event_id=s).samples[:, 0].mean() for s in range(8)])
    se = np.sqrt(means.var(ddof=1) / 8)
    assert abs(means.mean() - tab["mean0"]) < 4 * se + 2e-3, (means.mean(), tab["mean0"], se)


@pytest.mark.parametrize("paired,K,eff,hyper,want", [
    (False, 2, (100.0, 60.0), (1.0, 1.0), True),
    (False, 2, (100.0, 60.0), (2.0, 5.0), True),
    (False, 2, (1.0, 1.0), (1.0, 1e6), True),
    (False, 2, (100.0, 60.0), (0.5, 0.5), False),      # an unbounded density
    (False, 2, (100.0, 60.0), (1.0, 0.999), False),
    (False, 2, (0.0, 60.0), (1.0, 1.0), False),        # quirk C4
    (False, 2, (100.0, 0.0), (1.0, 1.0), False),
    (False, 3, (100.0, 60.0, 50.0), (1.0, 1.0, 1.0), False),
    (True, 2, (100.0, 60.0), (1.0, 1.0), False),
    # the fence: just inside and just beyond each bound, and what is not finite
    (False, 2, (100.0, 60.0), (1.0, 2.0 ** 20), True),
    (False, 2, (100.0, 60.0), (2.0 ** 20, 1.0), True),
    (False, 2, (100.0, 60.0), (1.0, 2.0 ** 20 + 1.0), False),
    (False, 2, (100.0, 60.0), (2.0 ** 20 + 1.0, 1.0), False),
    (False, 2, (100.0, 60.0), (1.0, 1e20), False),
    (False, 2, (100.0, 60.0), (1e30, 1.0), False),
    (False, 2, (100.0, 60.0), (1.0, float("inf")), False),
    (False, 2, (100.0, 60.0), (float("nan"), 1.0), False),
    (False, 2, (2.0 ** 40, 2.0 ** 20), (1.0, 1.0), True),
    (False, 2, (2.0 ** 40 * (1 + 2.0 ** -52), 2.0 ** 21), (1.0, 1.0), False),
    (False, 2, (2.0 ** -20, 2.0 ** -40), (1.0, 1.0), True),
    (False, 2, (2.0 ** -21, 2.0 ** -40 * (1 - 2.0 ** -53)), (1.0, 1.0), False),
    (False, 2, (1.0, 2.0 ** 20), (1.0, 1.0), True),
    (False, 2, (2.0 ** 20, 1.0), (1.0, 1.0), True),
    (False, 2, (1.0, 2.0 ** 20 + 1.0), (1.0, 1.0), False),
    (False, 2, (2.0 ** 20 + 1.0, 1.0), (1.0, 1.0), False),
    (False, 2, (float("inf"), 60.0), (1.0, 1.0), False),
    (False, 2, (float("inf"), float("inf")), (1.0, 1.0), False),
    (False, 2, (100.0, float("nan")), (1.0, 1.0), False),
])
def test_eligibility_table(paired, K, eff, hyper, want):
    assert eligible(paired, K, eff, hyper) == want
    el = capi.C.c_int(-1)       # ... and the library's own rule (host code: no device is needed)
    assert capi.lib().miso_exact_eligible(int(paired), K, capi._p(np.array(eff)), capi._p(np.array(hyper)), capi.C.byref(el)) == 0
    assert el.value == int(want)
