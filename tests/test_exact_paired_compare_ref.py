"""The restatement of the paired-end exact comparison (tests/_exact_paired_compare_ref.py) against
mpmath.

log_d0 = log Z12 - log Z1 - log Z2 at 40 digits: each Z the integral over logit space of exp(g), g written out from the
model (exponents, the pairs' factors with their multiplicities, the denominator), the pooled one as
exp(g1 + g2 - log x - log y).  H(z) at 20 digits (the nested integral; stated lower precision): 32 panels of 8-point
Gauss-Legendre over the narrower posterior's window, the other posterior's CDF from its density integrated between the
sorted arguments (five-point Gauss-Legendre between close neighbours, mp.quad otherwise).

Worst errors observed over the case list x the two hyperparameter pairs (printed by the tests):
    log_d0  4.5e-11   (50000+50000/3, h = (2, 5))
    H(z)    1.11e-6   (3-0-A50-1/no-pairs, h = (1, 1): the flat posterior's kink at the ends of (0, 1))
asserted at twice that, rounded up to one digit, and never beyond the scheme's caps, 1e-5 for log_d0 and 5e-5 for H.
"""
import mpmath as mp
import numpy as np
import pytest

from _exact_compare_ref import compare as compare16
from _exact_ref import Posterior
from _exact_paired_compare_ref import HYPERS, ZS, PairedCompare, cases, paired_stats

TOL_LOG_D0 = 9e-11       # twice the worst observed, rounded up; the cap is 1e-5
TOL_H = 3e-6             # twice the worst observed, rounded up; the cap is 5e-5
assert TOL_LOG_D0 <= 1e-5 and TOL_H <= 5e-5
CASES = cases()
TAIL = 12                # logit-space units beyond the restatement's window that the reference integrates over


@pytest.fixture(scope="module")
def post(orc):
    return PairedCompare(orc)


@pytest.fixture(scope="module")
def results(post):
    """every case's restated result and tables, made once"""
    out = {}
    for name, s1, s2 in CASES:
        for hyper in HYPERS:
            ps1, ps2 = paired_stats(s1, hyper), paired_stats(s2, hyper)
            res, a2 = post.compare(ps1, ps2, ZS)
            out[name, hyper] = (res, a2, post.tabulate(ps1), post.tabulate(ps2))
    return out


class MpSample:
    """one sample's density in logit space, from the model"""

    def __init__(self, sample, hyper, tab):
        n10, n01, A0, A1, pairs = sample
        m = np.asarray(pairs, np.float64).reshape(-1, 2)
        uniq, cnt = np.unique(m, axis=0, return_counts=True) if len(m) else (m, [])
        self.pairs = [(mp.mpf(float(a)), mp.mpf(float(b)), int(c)) for (a, b), c in zip(uniq, cnt)]
        self.a, self.b = mp.mpf(n10) + mp.mpf(hyper[0]), mp.mpf(n01) + mp.mpf(hyper[1])
        self.n = n10 + n01 + len(m)
        self.A0, self.A1 = mp.mpf(A0), mp.mpf(A1)
        self.gmax, self.tL, self.tR = mp.mpf(float(tab["gmax"])), mp.mpf(float(tab["tL"])), mp.mpf(float(tab["tR"]))

    def g(self, t):
        x, y = 1 / (1 + mp.exp(-t)), 1 / (1 + mp.exp(t))
        v = self.a * mp.log(x) + self.b * mp.log(y) - self.n * mp.log(x * self.A0 + y * self.A1)
        for m0, m1, c in self.pairs:
            v += c * mp.log(x * m0 + y * m1)
        return v

    def f(self, t):
        return mp.exp(self.g(t) - self.gmax)

    def knots(self, panels=8):
        return [self.tL - TAIL] + list(mp.linspace(self.tL, self.tR, panels + 1)) + [self.tR + TAIL]

    def log_z(self):
        k = self.knots()
        return self.gmax + mp.log(sum(mp.quad(self.f, [lo, hi]) for lo, hi in zip(k[:-1], k[1:])))


def mp_log_d0(m1, m2, tab12):
    g12, tL, tR = mp.mpf(float(tab12["gmax"])), mp.mpf(float(tab12["tL"])), mp.mpf(float(tab12["tR"]))

    def f12(t):
        return mp.exp(m1.g(t) + m2.g(t) + mp.log(1 + mp.exp(-t)) + mp.log(1 + mp.exp(t)) - g12)
    k = [tL - TAIL] + list(mp.linspace(tL, tR, 9)) + [tR + TAIL]
    lz12 = g12 + mp.log(sum(mp.quad(f12, [lo, hi]) for lo, hi in zip(k[:-1], k[1:])))
    return lz12 - m1.log_z() - m2.log_z()


def _gauss_legendre(n):
    """nodes and weights on [-1, 1] at the working precision: numpy's nodes refined by Newton steps"""
    out = []
    for v in np.polynomial.legendre.leggauss(n)[0]:
        x = mp.mpf(float(v))
        for _ in range(4):
            dp = n * (x * mp.legendre(n, x) - mp.legendre(n - 1, x)) / (x * x - 1)
            x = x - mp.legendre(n, x) / dp
        dp = n * (x * mp.legendre(n, x) - mp.legendre(n - 1, x)) / (x * x - 1)
        out.append((x, 2 / ((1 - x * x) * dp * dp)))
    assert abs(sum(w for _, w in out) - 2) < mp.mpf(10) ** (-mp.mp.dps + 3)
    return out


def mp_cdf(B, ts):
    """the CDF of B (normalised) at the logit-space points ts (None: below the support, mp.inf: above)"""
    gl5 = _gauss_legendre(5)
    lo0, hi0 = B.tL - TAIL, B.tR + TAIL
    close = (B.tR - B.tL) / 64
    knots = B.knots()
    z = sum(mp.quad(B.f, [a, b]) for a, b in zip(knots[:-1], knots[1:]))
    order = sorted(range(len(ts)), key=lambda i: ts[i])
    out = [None] * len(ts)
    acc, at = mp.mpf(0), lo0
    for i in order:
        t = min(max(ts[i], lo0), hi0)
        if t > at:
            if t - at <= close:
                half, mid = (t - at) / 2, (t + at) / 2
                acc += half * sum(w * B.f(mid + half * v) for v, w in gl5)
            else:
                brk = [at] + [k for k in knots if at < k < t] + [t]
                acc += sum(mp.quad(B.f, [a, b]) for a, b in zip(brk[:-1], brk[1:]))
            at = t
        out[i] = acc / z
    return out


def mp_H(m1, m2, a_is_2, zs, panels=32, order=8):
    mp.mp.dps = 20
    A, B = (m2, m1) if a_is_2 else (m1, m2)
    gl = _gauss_legendre(order)
    # (the other posterior's CDF has a kink where the shifted argument leaves (0, 1): those points end panels)
    kinks = [k for z in zs for k in ((-z, 1 - z) if a_is_2 else (z, 1 + z)) if 0 < k < 1]
    kinks = [mp.log(mp.mpf(k)) - mp.log(1 - mp.mpf(k)) for k in kinks]
    edges = sorted(list(mp.linspace(A.tL, A.tR, panels + 1)) + [k for k in kinks if A.tL < k < A.tR])
    nodes, wts = [], []
    for lo, hi in zip(edges[:-1], edges[1:]):
        half, mid = (hi - lo) / 2, (hi + lo) / 2
        for v, w in gl:
            t = mid + half * v
            nodes.append(t)
            wts.append(half * w * A.f(t))
    total = sum(wts)
    xs = [1 / (1 + mp.exp(-t)) for t in nodes]
    args, where = [], []
    for z in zs:
        for x in xs:
            u = x + mp.mpf(z) if a_is_2 else x - mp.mpf(z)
            where.append(0 if u <= 0 else (1 if u >= 1 else None))
            args.append(mp.log(u) - mp.log(1 - u) if where[-1] is None else mp.mpf(0))
    cdf = mp_cdf(B, [a for a, w in zip(args, where) if w is None])
    it = iter(cdf)
    vals = [next(it) if w is None else mp.mpf(w) for w in where]
    out = []
    for k in range(len(zs)):
        s = sum(w * v for w, v in zip(wts, vals[k * len(xs):(k + 1) * len(xs)])) / total
        out.append(s if a_is_2 else 1 - s)
    return out


WORST = {"log_d0": 0.0, "H": 0.0}


@pytest.mark.parametrize("hyper", HYPERS, ids=["h11", "h25"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_log_density_at_zero_against_mpmath(post, results, case, hyper):
    name, s1, s2 = case
    res, _, tab1, tab2 = results[name, hyper]
    mp.mp.dps = 40
    from _exact_paired_compare_ref import PooledStats
    tab12 = post.tabulate(PooledStats(tab1["ps"], tab2["ps"]))
    want = mp_log_d0(MpSample(s1, hyper, tab1), MpSample(s2, hyper, tab2), tab12)
    err = abs(float(mp.mpf(float(res[2])) - want))
    WORST["log_d0"] = max(WORST["log_d0"], err)
    print("%s %s: log_d0 %.12g, error %.3g (worst so far %.3g)" % (name, hyper, res[2], err, WORST["log_d0"]))
    assert err <= TOL_LOG_D0, (name, hyper, res[2], want)


@pytest.mark.parametrize("hyper", HYPERS, ids=["h11", "h25"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_cdf_of_the_difference_against_mpmath(results, case, hyper):
    name, s1, s2 = case
    res, a2, tab1, tab2 = results[name, hyper]
    want = mp_H(MpSample(s1, hyper, tab1), MpSample(s2, hyper, tab2), a2, ZS)
    errs = [abs(float(mp.mpf(float(h)) - w)) for h, w in zip(res[5:], want)]
    WORST["H"] = max(WORST["H"], max(errs))
    print("%s %s: H %s, worst error %.3g (worst so far %.3g)" % (name, hyper, np.round(res[5:], 6), max(errs), WORST["H"]))
    assert max(errs) <= TOL_H, (name, hyper, res[5:], want)


@pytest.mark.parametrize("hyper", HYPERS, ids=["h11", "h25"])
def test_monotone_and_symmetric_under_the_swap(post, results, hyper):
    for name, s1, s2 in CASES:
        res = results[name, hyper][0]
        assert (np.diff(res[5:]) >= 0).all(), name
        swapped, _ = post.compare(paired_stats(s2, hyper), paired_stats(s1, hyper), [-z for z in ZS])
        # swapping the samples gives 1 - H(-z); log_d0 is symmetric.  The swap changes the order of the pooled sums and which
        # sample's A stands first, so equality holds to rounding, not bit for bit: a few hundred ulps of the sums' terms
        assert np.abs((1.0 - swapped[5:]) - res[5:]).max() <= 1e-12, (name, res[5:], swapped[5:])
        assert abs(swapped[2] - res[2]) <= 1e-9 * max(1.0, abs(res[2])), (name, res[2], swapped[2])
        assert swapped[0] == res[1] and swapped[1] == res[0]


@pytest.mark.parametrize("hyper", HYPERS, ids=["h11", "h25"])
def test_no_pairs_and_equal_A_agree_with_the_single_end_scheme(orc, results, hyper):
    """both samples without drawing pairs and with the same A: section 16's family, e = A.  The two schemes differ in their
    windows and cell rules; they agree to section 16's accuracy (2.2e-6 in H, asserted 5e-6 there) and to 1e-8 in log_d0"""
    p16 = Posterior(orc)
    n = 0
    for name, s1, s2 in CASES:
        if len(s1[4]) or len(s2[4]) or s1[2:4] != s2[2:4]:
            continue
        n += 1
        rows = [[float(s[0]), float(s[1]), float(s[0] + s[1]), s[2], s[3], hyper[0], hyper[1]] for s in (s1, s2)]
        want = compare16(p16, rows[0], rows[1], ZS)
        res = results[name, hyper][0]
        assert np.abs(res[:2] - want[:2]).max() <= 1e-9, name
        assert abs(res[2] - want[2]) <= 1e-8, (name, res[2], want[2])
        assert np.abs(res[5:] - want[5:]).max() <= 5e-6, (name, res[5:], want[5:])
    assert n == 3
