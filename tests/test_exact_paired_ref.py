"""CPU: the paired-end exact-posterior mode's numerical scheme (tests/_exact_paired_ref.py, the restatement of
csrc/kernels_exact_paired.hip) against mpmath at 40 digits, against the checker's counter-mode paired sampler, and its
eligibility rule.

The mpmath side integrates the density piece by piece between the window's ends, sixteen inner split points and the
restatement's own quantile points (equal pairs collapsed into classes with a count: the same function); the error of a
quantile is (CDF(x) - p) / pdf(x).
"""
import mpmath as mp
import numpy as np
import pytest

from _exact_paired_ref import (PairedPosterior, PairedStats, eligible, simulated_case, synthetic_cases)
from _exact_ref import Posterior, Stats
from _libs import OrcLib
from miso_amd import capi

PROBS = [0.001, 0.025, 0.5, 0.975, 0.999]
MEAN_TOL = 1e-9      # posterior mean (tests/test_exact_ref.py)
QUANT_TOL = 1e-6     # inverse CDF, in psi
HYPERS = [(1.0, 1.0), (2.0, 5.0)]
SYNTH = synthetic_cases()
SIMULATED = [400, 60, 1000]      # simulate_pe(orc, 2, n) at mean 250, variance 900


@pytest.fixture(scope="module")
def post(orc):
    return PairedPosterior(orc)


@pytest.fixture(scope="module")
def sims(orc):
    return {n: simulated_case(orc, n) for n in SIMULATED}


def mp_g(ps_args, hyper):
    """the log density in logit space at 40 digits: t -> g(t), from (n10, n01, A0, A1, pairs)"""
    n10, n01, A0, A1, pairs = ps_args
    pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 2)
    cls = {}
    for m0, m1 in pairs:
        cls[(float(m0), float(m1))] = cls.get((float(m0), float(m1)), 0) + 1
    cls = [(mp.mpf(k[0]), mp.mpf(k[1]), c) for k, c in cls.items()]
    a, b = mp.mpf(n10) + mp.mpf(hyper[0]), mp.mpf(n01) + mp.mpf(hyper[1])
    n = mp.mpf(n10 + n01 + len(pairs))
    A0, A1 = mp.mpf(float(A0)), mp.mpf(float(A1))

    def g(t):
        em = mp.exp(-t)
        x, y = 1 / (1 + em), em / (1 + em)
        v = a * mp.log(x) + b * mp.log(y) - n * mp.log(x * A0 + y * A1)
        for m0, m1, c in cls:
            v += c * mp.log(x * m0 + y * m1)
        return v
    return g


def mp_errors(ps_args, hyper, tab, t_hat):
    mp.mp.dps = 40
    g = mp_g(ps_args, hyper)
    gref = mp.mpf(float(tab["gmax"]))
    memo = {}

    def f(t):
        if t not in memo:
            memo[t] = mp.exp(g(t) - gref)
        return memo[t]

    def xf(t):
        return f(t) / (1 + mp.exp(-t))
    tL, tR = mp.mpf(float(tab["tL"])), mp.mpf(float(tab["tR"]))
    pts = {tL - 300, tL, tR, tR + 300} | {tL + (tR - tL) * k / 16 for k in range(1, 16)} | {mp.mpf(float(t)) for t in t_hat}
    pts = sorted(pts)
    cum, Z, M = {pts[0]: mp.mpf(0)}, mp.mpf(0), mp.mpf(0)
    for lo, hi in zip(pts[:-1], pts[1:]):
        Z += mp.quad(f, [lo, hi])
        M += mp.quad(xf, [lo, hi])
        cum[hi] = Z
    errs = []
    for p, t in zip(PROBS, t_hat):
        tt = mp.mpf(float(t))
        x = 1 / (1 + mp.exp(-tt))
        errs.append(float((cum[tt] / Z - mp.mpf(p)) * Z * x * (1 - x) / f(tt)))
    return float(mp.mpf(float(tab["mean0"])) - M / Z), errs, g


def check_against_mpmath(post, ps_args, hyper):
    n10, n01, A0, A1, pairs = ps_args
    tab = post.tabulate(PairedStats(n10, n01, A0, A1, hyper[0], hyper[1], pairs))
    t_hat = post.invert(tab, np.array(PROBS) * tab["Z"])
    q = post.icdf(tab, PROBS)
    assert (np.diff(q[:, 0]) > 0).all() and np.allclose(q[:, 0] + q[:, 1], 1.0, rtol=0, atol=1e-15)
    mean_err, q_err, g = mp_errors(ps_args, hyper, tab, t_hat)
    print("window [%.4f, %.4f], mean error %.3g, quantile errors %s" % (tab["tL"], tab["tR"], mean_err, ["%.3g" % e for e in q_err]))
    assert abs(mean_err) < MEAN_TOL
    assert max(abs(e) for e in q_err) < QUANT_TOL
    assert abs((tab["mean0"] + tab["mean1"]) - 1.0) < 1e-14
    return tab, g


@pytest.mark.parametrize("hyper", HYPERS, ids=lambda h: "h%g_%g" % h)
@pytest.mark.parametrize("case", SYNTH, ids=lambda c: c[0])
def test_restatement_against_mpmath(orc, post, case, hyper):
    name, args = case[0], case[1:]
    tab, g = check_against_mpmath(post, args, hyper)
    if name.startswith("two-mode") and hyper == (1.0, 1.0):
        # the issue's two maxima (mirrored: their negatives) lie inside the window, each a local maximum of g at 40 digits
        sign = -1.0 if name.endswith("mirrored") else 1.0
        for tm in (-7.22, -0.11):
            tm = sign * tm
            assert tab["tL"] < tm < tab["tR"], (tab["tL"], tab["tR"], tm)
            assert g(mp.mpf(tm)) > max(g(mp.mpf(tm - 0.3)), g(mp.mpf(tm + 0.3)))
        assert g(mp.mpf(sign * -3.17)) < min(g(mp.mpf(sign * -7.22)), g(mp.mpf(sign * -0.11))) - 0.8
    if not len(args[4]):
        # no drawing pair: the single-end density with e = A -- the other scheme's table agrees
        n10, n01, A0, A1, _ = args
        other = Posterior(orc).tabulate(Stats(n10, n01, n10 + n01, A0, A1, hyper[0], hyper[1]))
        assert abs(other["mean0"] - tab["mean0"]) < MEAN_TOL
        qa, qb = post.icdf(tab, PROBS), Posterior(orc).icdf(other, PROBS)
        assert np.abs(qa - qb).max() < QUANT_TOL


@pytest.mark.parametrize("hyper", HYPERS, ids=lambda h: "h%g_%g" % h)
@pytest.mark.parametrize("n_pairs", SIMULATED)
def test_simulated_events_against_mpmath(post, sims, n_pairs, hyper):
    c = sims[n_pairs]
    print("%d pairs: n10 %d, n01 %d, drawing %d in %d classes" % (n_pairs, c["n10"], c["n01"], len(c["pairs"]),
                                                                 len({tuple(p) for p in c["pairs"]})))
    check_against_mpmath(post, (c["n10"], c["n01"], c["A"][0], c["A"][1], c["pairs"]), hyper)


@pytest.mark.parametrize("n_pairs", SIMULATED)
def test_restated_mean_against_counter_mode_paired_sampler(orc, post, sims, n_pairs):
    """test_statistics.py's rule, 4 se + 2e-3, over 8 event ids"""
    c = sims[n_pairs]
    tab = post.tabulate(PairedStats(c["n10"], c["n01"], c["A"][0], c["A"][1], 1.0, 1.0, c["pairs"]))
    means = np.array([orc.miso_paired(c["g"], c["pos"], c["cig"], 36, 250.0, 900.0, iters=4000, burn=1000, lag=1, chains=1,
                                      mode=OrcLib.COUNTER, seed=500 + s, event_id=s).samples.reshape(-1, 2)[:, 0].mean()
                      for s in range(8)])
    se = np.sqrt(means.var(ddof=1) / 8)
    print("exact %.6f, counter-mode sampler %.6f +- %.6f" % (tab["mean0"], means.mean(), se))
    assert abs(means.mean() - tab["mean0"]) < 4 * se + 2e-3, (means.mean(), tab["mean0"], se)


@pytest.mark.parametrize("K,A,hyper,any_bad,want", [
    (2, (60000.0, 43000.0), (1.0, 1.0), False, True),
    (2, (60000.0, 43000.0), (2.0, 5.0), False, True),
    (2, (1.0, 1.0), (1.0, 1e6), False, True),
    (2, (60000.0, 43000.0), (0.5, 0.5), False, False),     # an unbounded density
    (2, (60000.0, 43000.0), (1.0, 0.999), False, False),
    (2, (0.0, 43000.0), (1.0, 1.0), False, False),         # an isoform no fragment fits
    (2, (60000.0, 0.0), (1.0, 1.0), False, False),
    (2, (60000.0, 43000.0), (1.0, 1.0), True, False),      # a pair on a non-finite score entry
    (3, (60000.0, 43000.0, 100.0), (1.0, 1.0, 1.0), False, False),
    # the fence (DESIGN.md sections 15, 17): just inside and just beyond each bound, and what is not finite
    (2, (60000.0, 43000.0), (2.0 ** 20, 2.0 ** 20), False, True),
    (2, (60000.0, 43000.0), (1.0, 2.0 ** 20 + 1.0), False, False),
    (2, (60000.0, 43000.0), (2.0 ** 20 + 1.0, 1.0), False, False),
    (2, (60000.0, 43000.0), (1.0, 1e20), False, False),
    (2, (60000.0, 43000.0), (float("inf"), 1.0), False, False),
    (2, (60000.0, 43000.0), (1.0, float("nan")), False, False),
    (2, (2.0 ** 40, 2.0 ** 20), (1.0, 1.0), False, True),
    (2, (2.0 ** 21, 2.0 ** 40 * (1 + 2.0 ** -52)), (1.0, 1.0), False, False),
    (2, (2.0 ** -40, 2.0 ** -20), (1.0, 1.0), False, True),
    (2, (2.0 ** -40 * (1 - 2.0 ** -53), 2.0 ** -21), (1.0, 1.0), False, False),
    (2, (1.0, 2.0 ** 20), (1.0, 1.0), False, True),
    (2, (2.0 ** 20 + 1.0, 1.0), (1.0, 1.0), False, False),
    (2, (1.0, 2.0 ** 20 + 1.0), (1.0, 1.0), False, False),
    (2, (float("inf"), 43000.0), (1.0, 1.0), False, False),
    (2, (60000.0, float("nan")), (1.0, 1.0), False, False),
])
def test_eligibility_table(K, A, hyper, any_bad, want):
    assert eligible(K, A, hyper, any_bad) == want
    el = capi.C.c_int(-1)       # ... and the library's own rule (host code: no device is needed)
    assert capi.lib().miso_exact_paired_eligible(K, capi._p(np.array(A)), capi._p(np.array(hyper)), int(any_bad), capi.C.byref(el)) == 0
    assert el.value == int(want)
