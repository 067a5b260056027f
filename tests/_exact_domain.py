"""The eligible domain of the exact-posterior family (DESIGN.md sections 15 - 20b) as a sweep, and references for it that owe
nothing to the numerical scheme.  Test infrastructure only: nothing under miso_amd/ imports this module.

The sweep is deterministic -- structured products of the axes below plus a part drawn from np.random.default_rng(SEED) -- and
no case is skipped or filtered when a test runs.

Single-end.  The density of psi = x of an event (n10, n01, n11, e0, e1) under hyperparameters (h0, h1) is
    p(x) ~ x^(a-1) (1-x)^(b-1) / D(x)^n,   a = n10 + h0, b = n01 + h1, n = n10 + n01 + n11, D(x) = x e0 + (1-x) e1.

  EQ   e0 = e1 = e.  D = e is a constant, so x ~ Beta(a, b) whatever n11 and e are: mean a / (a + b), CDF the regularised
       incomplete beta function I_x(a, b).
  C0   n11 = h0 + h1, that is n = a + b (c = a + b - n = 0), any e0 != e1.  Substitute w = x e0 / D(x).  Then
       1 - w = (1-x) e1 / D, dw/dx = e0 e1 / D^2, x = w D / e0, 1 - x = (1-w) D / e1, and
           p(x) dx ~ (w D / e0)^(a-1) ((1-w) D / e1)^(b-1) D^-n  D^2 / (e0 e1) dw ~ w^(a-1) (1-w)^(b-1) D^(a+b-n) dw,
       so for n = a + b the power of D vanishes and w ~ Beta(a, b) EXACTLY, at every ratio e0 / e1.  w is increasing in x, so
       P(x <= q) = I_w(q)(a, b); the density of x is Beta's at w times dw/dx; the quantiles follow from
       x = w e1 / (w e1 + (1-w) e0).  The mean of x has no closed form; mp.quad of x(w) against Beta's density gives it on the
       few cases where it is checked (c0_mean).

Paired-end.  The density is x^(a-1) (1-x)^(b-1) / (x A0 + (1-x) A1)^n  prod_i (x m0_i + (1-x) m1_i), n = n10 + n01 + pairs.

  RATIO  every drawing pair has m0_i = 2 m1_i exactly, and A0 = 2 A1.  Then x m0_i + (1-x) m1_i = m1_i (1 + x) and
         x A0 + (1-x) A1 = A1 (1 + x): the pairs' factors cancel against as many factors of the denominator and leave
         x^(a-1) (1-x)^(b-1) / (1 + x)^(n10 + n01) -- the single-end event (n10, n01, n11 = 0, e0 = A0, e1 = A1), whatever
         the pairs are.  A dropped or doubled pair leaves a factor (1 + x)^-+1 behind, which m0 = m1 (a constant factor) would
         not.  Its reference is mpmath's quadrature of that density (mp_single_end); the counts are small.
  PEQ    m0_i = m1_i and A0 = A1: every factor is a constant, x ~ Beta(a, b).
  PMIN   PEQ with sixteen and seventeen pairs at exactly 2^-63, the smallest admitted probability: a block's product is 2^-1008.

Comparisons (EQ only: Beta laws on both sides).  The density of psi_1 - psi_2 at 0 is int p_1 p_2 dx, so
    log_d0 = lnB(a1 + a2 - 1, b1 + b2 - 1) - lnB(a1, b1) - lnB(a2, b2).

How the references are evaluated: scipy.special.betainc / betaln in double precision, the complementary side
I_(1-x)(b, a) above the median (the device's own 1 - x goes in, not a rounded difference); mpmath's betainc at 40 digits stops
converging near a = 40001, b = 30001 ("Hypergeometric series converges too slowly"), so it serves as the cross-check of scipy
on every case with max(a, b) <= MP_LIMIT (mp_cross_check).  The error of a quantile point x^ is the project's own form,
(CDF(x^) - p) / pdf(x^), in psi.
"""
import itertools

import mpmath as mp
import numpy as np
from scipy import special

SEED = 20240915
INT_MAX = 2 ** 31 - 1

# ---- tolerances: tests/test_exact_ref.py (MEAN_TOL, QUANT_TOL, PROBS), tests/test_exact_delta_ref.py (C) ----
MEAN_TOL = 1e-9
QUANT_TOL = 1e-6
PROBS = [0.001, 0.025, 0.5, 0.975, 0.999]
P_EXTREME = 2.0 ** -33                        # a sample row inverts u Z, u in [2^-33, 1 - 2^-33] (exact_uniform)
EXTREMES = [P_EXTREME, 1.0 - P_EXTREME]
ALL_PROBS = PROBS + EXTREMES
C_EXTREME = 5e-5                              # half a unit of the fourth printed decimal
MP_LIMIT = 30000                              # mpmath's betainc converges, and quickly, up to here

# ---- the fence (csrc/batch.hpp exact_fence) ----
HYPER_MAX = 2.0 ** 20
LEN_MAX, LEN_MIN = 2.0 ** 40, 2.0 ** -40
RATIO_MAX = 2.0 ** 20

# ---- the axes ----
COUNTS = [0, 1, 7, 10 ** 3, 10 ** 6, 10 ** 7, INT_MAX]
N11S = [0, 5, 10 ** 6]
LENGTHS = [1.0, 150.0, 1e5]
RATIOS = [2.0 ** -20, 1e-5, 2.0 / 3.0, 3.0, 1e5]
HYPERS = [(1.0, 1.0), (2.0, 5.0), (1.0, 1e6), (1e3, 1.0)]
PAIR_COUNTS = [1, 15, 16, 17, 63, 64, 65, 79, 80, 81, 127, 128, 129, 1000]


def _rng(stream):
    return np.random.default_rng([SEED, stream])


def _log_uniform_int(rng, hi):
    return int(np.floor(np.exp(rng.uniform(0.0, np.log(hi + 1.0))))) - 1


def eq_cases():
    """[(n10, n01, n11, e0, e1, h0, h1)] with e0 == e1: counts x counts x hyperparameters, n11 and e taken in turn; the
    fence's corners; sixty random cases"""
    out = []
    for i, ((n10, n01), h) in enumerate(itertools.product(itertools.product(COUNTS, COUNTS), HYPERS)):
        e = LENGTHS[i % 3]
        out.append((n10, n01, N11S[(i // 3) % 3], e, e, h[0], h[1]))
    for e in (LEN_MIN, LEN_MAX):                  # h at its bound, no reads on that side, all reads on the other; and mirrored
        out += [(0, INT_MAX, 0, e, e, HYPER_MAX, 1.0), (INT_MAX, 0, 5, e, e, 1.0, HYPER_MAX),
                (0, 0, INT_MAX, e, e, HYPER_MAX, HYPER_MAX), (INT_MAX, INT_MAX, INT_MAX, e, e, HYPER_MAX, HYPER_MAX),
                (0, INT_MAX, INT_MAX, e, e, 1.0, HYPER_MAX), (INT_MAX, 0, INT_MAX, e, e, HYPER_MAX, 1.0)]
    rng = _rng(1)
    for _ in range(60):
        e = float(np.exp(rng.uniform(np.log(LEN_MIN), np.log(LEN_MAX))))
        h = [float(np.exp(rng.uniform(0.0, np.log(HYPER_MAX)))) for _ in range(2)]
        out.append((_log_uniform_int(rng, INT_MAX), _log_uniform_int(rng, INT_MAX), _log_uniform_int(rng, INT_MAX), e, e, h[0], h[1]))
    return out


def c0_cases(ratio):
    """[(n10, n01, n11 = h0 + h1, e0 = e ratio, e1 = e, h0, h1)] of one ratio of the effective lengths: counts x counts x
    hyperparameters, e taken in turn; with the two extreme ratios, the fence's corners (the ratio at its bound with the
    lengths at theirs, h at its bound) and ten random cases of that sign"""
    out = []
    for i, ((n10, n01), h) in enumerate(itertools.product(itertools.product(COUNTS, COUNTS), HYPERS)):
        e = LENGTHS[i % 3]
        out.append((n10, n01, int(h[0] + h[1]), e * ratio, e, h[0], h[1]))
    if ratio in (RATIOS[0], RATIOS[-1]):
        up = ratio > 1.0
        bound = RATIO_MAX if up else 1.0 / RATIO_MAX
        for big in (LEN_MAX, LEN_MIN * RATIO_MAX):    # the larger length of the two
            e0, e1 = (big, big / RATIO_MAX) if up else (big / RATIO_MAX, big)
            assert e0 / e1 == bound
            for n10, n01, h0, h1 in [(0, INT_MAX, 1.0, 1.0), (INT_MAX, 0, 1.0, 1.0), (0, INT_MAX, HYPER_MAX, 1.0),
                                     (INT_MAX, 0, 1.0, HYPER_MAX), (0, INT_MAX, 1.0, HYPER_MAX), (INT_MAX, 0, HYPER_MAX, 1.0),
                                     (0, 0, HYPER_MAX, HYPER_MAX), (INT_MAX, INT_MAX, 1.0, 1.0), (0, 0, 1.0, 1.0)]:
                out.append((n10, n01, int(h0 + h1), e0, e1, h0, h1))
        rng = _rng(2 if up else 3)
        for _ in range(10):
            r = float(np.exp(rng.uniform(0.0, np.log(RATIO_MAX))))
            e = float(np.exp(rng.uniform(np.log(LEN_MIN * RATIO_MAX), np.log(LEN_MAX / RATIO_MAX))))
            h = [float(np.floor(np.exp(rng.uniform(0.0, np.log(HYPER_MAX))))) for _ in range(2)]
            out.append((_log_uniform_int(rng, INT_MAX), _log_uniform_int(rng, INT_MAX), int(h[0] + h[1]),
                        e * r if up else e / r, e, h[0], h[1]))
    return out


def c0_mean_cases():
    """the handful of C0 cases whose mean is checked (one quadrature each)"""
    return [(0, 0, 2, 2.0 ** -20, 1.0, 1.0, 1.0), (0, 0, 2, 1e5, 1.0, 1.0, 1.0), (7, 1, 7, 100.0, 150.0, 2.0, 5.0),
            (1000, 7, 1001, 450.0, 150.0, 1e3, 1.0), (0, 1000, 2, 1.0, 1e5, 1.0, 1.0), (1, 0, 1000001, 1e5 * 2.0 ** -20, 1e5, 1.0, 1e6),
            (10 ** 6, 10 ** 3, 7, 1e-5, 1.0, 2.0, 5.0), (7, 10 ** 6, 2, 3e5, 1e5, 1.0, 1.0)]


def swap_labels(case):
    n10, n01, n11, e0, e1, h0, h1 = case
    return (n01, n10, n11, e1, e0, h1, h0)


def row7(case):
    """the statistics of a case in miso_selftest_exact's layout: (n10, n01, n, e0, e1, h0, h1)"""
    n10, n01, n11, e0, e1, h0, h1 = case
    return [float(n10), float(n01), float(n10 + n01 + n11), float(e0), float(e1), float(h0), float(h1)]


def case_id(case):
    return "-".join("%g" % v for v in case)


# ---- the Beta law in double precision ----

def beta_quantile_errors(a, b, u, v, probs, jac=1.0):
    """(CDF(u) - p) / (pdf(u) jac) of Beta(a, b) at the points u with v = 1 - u given on its own; a, b: arrays [n];
    u, v, jac: [n, len(probs)].  Above the median the complementary side, whose target 1 - p is exact for the probabilities
    used here up to an ulp of p."""
    a, b = np.asarray(a, np.float64)[:, None], np.asarray(b, np.float64)[:, None]
    p = np.asarray(probs, np.float64)[None, :]
    low = special.betainc(a, b, u) - p
    high = (1.0 - p) - special.betainc(b, a, v)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pdf = np.exp((a - 1.0) * np.log(u) + (b - 1.0) * np.log(v) - special.betaln(a, b))
        return np.where(p <= 0.5, low, high) / (pdf * jac)


def eq_reference(cases, icdf):
    """(means [n, 2], quantile errors in psi [n, len(probs)]) of EQ cases at the points icdf [n, len(probs), 2] = (x, 1 - x)"""
    a = np.array([c[0] + c[5] for c in cases], np.float64)
    b = np.array([c[1] + c[6] for c in cases], np.float64)
    means = np.stack([a / (a + b), b / (a + b)], axis=1)
    probs = ALL_PROBS[:icdf.shape[1]]
    return means, beta_quantile_errors(a, b, icdf[:, :, 0], icdf[:, :, 1], probs)


def c0_reference(cases, icdf):
    """quantile errors in psi [n, len(probs)] of C0 cases at the points icdf = (x, 1 - x): w = x e0 / D, 1 - w = (1 - x) e1 / D,
    each from its own factor; the density of x is Beta's at w times dw/dx = e0 e1 / D^2"""
    a = np.array([c[0] + c[5] for c in cases], np.float64)
    b = np.array([c[1] + c[6] for c in cases], np.float64)
    for c in cases:
        assert c[2] == c[5] + c[6] and c[3] != c[4]
    e0 = np.array([c[3] for c in cases], np.float64)[:, None]
    e1 = np.array([c[4] for c in cases], np.float64)[:, None]
    x, y = icdf[:, :, 0], icdf[:, :, 1]
    D = x * e0 + y * e1
    probs = ALL_PROBS[:icdf.shape[1]]
    return beta_quantile_errors(a, b, x * e0 / D, y * e1 / D, probs, jac=(e0 / D) * (e1 / D))


def c0_mean(case):
    """E x of a C0 case: x(w) = w e1 / (w e1 + (1 - w) e0) against Beta(a, b)'s density, mpmath at 30 digits, split at Beta's mean"""
    mp.mp.dps = 30
    a, b = mp.mpf(case[0]) + mp.mpf(case[5]), mp.mpf(case[1]) + mp.mpf(case[6])
    e0, e1 = mp.mpf(case[3]), mp.mpf(case[4])
    lnB = mp.loggamma(a) + mp.loggamma(b) - mp.loggamma(a + b)

    def f(w):
        if w <= 0 or w >= 1:
            return mp.mpf(0)
        return w * e1 / (w * e1 + (1 - w) * e0) * mp.exp((a - 1) * mp.log(w) + (b - 1) * mp.log1p(-w) - lnB)
    m, sd = a / (a + b), mp.sqrt(a * b / ((a + b) ** 2 * (a + b + 1)))
    pts = sorted({mp.mpf(0), mp.mpf(1)} | {min(max(m + k * sd, mp.mpf(0)), mp.mpf(1)) for k in (-40, -10, -3, 0, 3, 10, 40)})
    return float(sum(mp.quad(f, [lo, hi]) for lo, hi in zip(pts[:-1], pts[1:])))


def mp_cross_check(a, b, u, v, probs):
    """(the largest relative difference between scipy's and mpmath's (40 digits) incomplete beta function on the side
    beta_quantile_errors takes, the number of points at which mpmath converged) at the points of one law; max(a, b) <= MP_LIMIT"""
    assert max(a, b) <= MP_LIMIT
    mp.mp.dps = 40
    worst, done = 0.0, 0
    for p, uu, vv in zip(probs, u, v):
        aa, bb, xx = (a, b, uu) if p <= 0.5 else (b, a, vv)
        try:
            want = mp.betainc(mp.mpf(aa), mp.mpf(bb), 0, mp.mpf(float(xx)), regularized=True)
        except (ValueError, ZeroDivisionError):     # "hypsum() failed to converge", "pole in hypergeometric series"
            continue
        done += 1
        worst = max(worst, abs(float((mp.mpf(float(special.betainc(aa, bb, xx))) - want) / want)))
    return worst, done


# ---- any single-end density by quadrature (small counts): RATIO's reference ----

def mp_single_end(case, xs, ys):
    """(E x, [CDF at x for x in xs]) of a single-end case, mpmath at 30 digits: the density in logit space integrated piece by
    piece between the sorted points and a few landmarks.  xs ascending; ys = 1 - xs given on their own."""
    mp.mp.dps = 30
    n10, n01, n11, e0, e1, h0, h1 = case
    a, b, n = mp.mpf(n10) + mp.mpf(h0), mp.mpf(n01) + mp.mpf(h1), mp.mpf(n10 + n01 + n11)
    e0, e1 = mp.mpf(e0), mp.mpf(e1)

    def lg(t):
        if t >= 0:
            em = mp.exp(-t)
            return -b * t - (a + b - n) * mp.log1p(em) - n * mp.log(e0 + em * e1)
        ep = mp.exp(t)
        return a * t - (a + b - n) * mp.log1p(ep) - n * mp.log(ep * e0 + e1)
    tm = mp.findroot(lambda t: mp.diff(lg, t), mp.log(a / b), tol=1e-15, verify=False)
    top = lg(tm)
    ts = [mp.log(mp.mpf(float(x))) - mp.log(mp.mpf(float(y))) for x, y in zip(xs, ys)]
    pts = sorted({tm + k for k in (-400, -60, -20, -6, -2, 0, 2, 6, 20, 60, 400)} | set(ts))
    cum, Z, M = {pts[0]: mp.mpf(0)}, mp.mpf(0), mp.mpf(0)
    for lo, hi in zip(pts[:-1], pts[1:]):
        Z += mp.quad(lambda t: mp.exp(lg(t) - top), [lo, hi])
        M += mp.quad(lambda t: mp.exp(lg(t) - top) / (1 + mp.exp(-t)), [lo, hi])
        cum[hi] = Z
    pdf = [mp.exp(lg(t) - top) / (Z * mp.mpf(float(x)) * mp.mpf(float(y))) for t, x, y in zip(ts, xs, ys)]
    return float(M / Z), [cum[t] / Z for t in ts], pdf


# ---- the paired-end cases: (name, n10, n01, A0, A1, h0, h1, pairs, the equivalent single-end case) ----

def _min_prob_pairs(rng, n, ratio):
    """m1 log-uniform in [2^-63, 0.0133 / ratio], m0 = ratio m1 (exact for a power of two)"""
    m1 = np.exp(rng.uniform(np.log(2.0 ** -63), np.log(0.0133 / ratio), size=n))
    m1[0] = 2.0 ** -63
    return np.stack([ratio * m1, m1], axis=1)


def ratio_cases():
    """one RATIO case per pair count, every EXP_BLOCK (16) and EXP_CHUNK (64) boundary of exact_pair_logsum among them"""
    rng = _rng(4)
    counts = [(3, 4), (0, 0), (11, 5), (0, 9), (40, 30), (7, 0), (1, 1), (5, 12)]
    hypers = [(1.0, 1.0), (2.0, 5.0)]
    out = []
    for i, npairs in enumerate(PAIR_COUNTS):
        n10, n01 = counts[i % len(counts)]
        h = hypers[i % 2]
        A1 = [43000.0, 1.0, 2.0 ** 39][i % 3]
        out.append(("ratio-%d" % npairs, n10, n01, 2.0 * A1, A1, h[0], h[1], _min_prob_pairs(rng, npairs, 2.0),
                    (n10, n01, 0, 2.0 * A1, A1, h[0], h[1])))
    return out


def peq_cases():
    """PEQ and PMIN: Beta(a, b)"""
    rng = _rng(5)
    out = []
    for i, (npairs, n10, n01, h) in enumerate([(0, 11, 5, (1.0, 1.0)), (1, 0, 0, (1.0, 1.0)), (17, 0, 1000, (2.0, 5.0)),
                                               (65, 10 ** 6, 7, (1.0, 1e6)), (200, INT_MAX, 0, (1.0, 1.0)),
                                               (81, 0, INT_MAX, (HYPER_MAX, 1.0)), (129, 10 ** 7, 10 ** 7, (1e3, 1.0))]):
        m = np.exp(rng.uniform(np.log(2.0 ** -63), np.log(0.0133), size=npairs))
        A = [60000.0, LEN_MIN, LEN_MAX][i % 3]
        out.append(("peq-%d" % npairs, n10, n01, A, A, h[0], h[1], np.stack([m, m], axis=1).reshape(-1, 2), (n10, n01, npairs, A, A, h[0], h[1])))
    for npairs in (16, 17):
        out.append(("pmin-%d" % npairs, 3, 0, 50.0, 50.0, 1.0, 1.0, np.full((npairs, 2), 2.0 ** -63), (3, 0, npairs, 50.0, 50.0, 1.0, 1.0)))
    return out


def stats6(pcase):
    return [float(v) for v in pcase[1:7]]


# ---- pairs to compare (EQ on both sides): what the fixed pair list lacks ----

def compare_pairs():
    """[(name, case 1, case 2)], both cases with the same e0 == e1"""
    def c(n10, n01, n11=0, e=150.0, h=(1.0, 1.0)):
        return (n10, n01, n11, e, e, h[0], h[1])
    return [
        ("wide/1000-times-narrower", c(5, 5), c(5 * 10 ** 6, 5 * 10 ** 6)),
        ("1000-times-narrower/wide", c(5 * 10 ** 6, 5 * 10 ** 6, 5), c(5, 5, 5)),
        ("sharp-ten-reads-apart", c(200000, 200000), c(200010, 199990)),
        ("both-at-1e-6", c(0, 10 ** 6, 0, 1e5), c(1, 10 ** 6, 0, 1e5)),
        ("both-at-1e-6-h2_5", c(0, 10 ** 6, 5, 1.0, (2.0, 5.0)), c(3, 2 * 10 ** 6, 0, 1.0, (2.0, 5.0))),
        ("opposite-ends", c(0, 1000), c(1000, 0)),
        ("opposite-ends-sharp", c(0, 10 ** 7, 10 ** 6), c(10 ** 7, 0)),
        ("self", c(11, 5, 17), c(11, 5, 17)),
        ("self-sharp", c(40000, 30000), c(40000, 30000)),
    ]


def log_d0_reference(c1, c2):
    """(log_d0, the bound on its error: log_d0_bound);
    mpmath's loggamma at 40 digits -- a double-precision lnB(2, 10^6) is a difference of numbers near 10^7 and good to 1e-9
    only, more than that bound at the pairs whose mass sits at 1e-6"""
    mp.mp.dps = 40

    def lnB(a, b):
        return mp.loggamma(a) + mp.loggamma(b) - mp.loggamma(a + b)
    a1, b1, a2, b2 = (mp.mpf(v) for v in (c1[0] + c1[5], c1[1] + c1[6], c2[0] + c2[5], c2[1] + c2[6]))
    l12, l1, l2 = lnB(a1 + a2 - 1, b1 + b2 - 1), lnB(a1, b1), lnB(a2, b2)
    n1, n2, le = sum(c1[:3]), sum(c2[:3]), mp.log(mp.mpf(c1[3]))
    sizes = abs(l12 - (n1 + n2) * le) + abs(l1 - n1 * le) + abs(l2 - n2 * le)
    return float(l12 - l1 - l2), log_d0_bound(float(sizes), float(2 * (n1 + n2 + a1 + b1 + a2 + b2)))


def log_d0_bound(sizes, weights):
    """The bound on log_d0's error.  tests/test_exact_compare_ref.py has sixteen ulps of `sizes`, the sum of the three |log Z|,
    plus 1e-12.  That is the rounding of the sums; it leaves out the rounding INSIDE a density: 1 + E and the denominator
    e0 + E e1 are each rounded to 2^-53 of a number near its larger term, so their logs carry an absolute error of 2^-53, which
    the density multiplies by |c| and n.  Each log Z therefore carries up to (n + a + b) 2^-53 more; `weights` is that sum
    over the two posteriors and their product.  On the fixed pair list the term is below the first; with 10^6 reads at
    psi = 1e-6 (log Z near -30) it is the larger one."""
    return 16 * 2.0 ** -53 * sizes + 2.0 ** -53 * weights + 1e-12


# ---- the assertions both the restatement's and the device's tests make ----

def _report(what, name, err, cases, tol):
    i, j = np.unravel_index(int(np.nanargmax(np.abs(err))), err.shape)
    print("%s: worst %s %.3g (bound %.3g) at %s, column %d" % (what, name, abs(err[i, j]), tol, case_id(cases[i]), j))
    bad = ~(np.abs(err) < tol)
    assert not bad.any(), (what, name, [(case_id(cases[k]), err[k].tolist()) for k in np.nonzero(bad.any(axis=1))[0][:5]])


def assert_quantiles(what, cases, err):
    """err [n, 7]: the quantile errors in psi at ALL_PROBS"""
    assert err.shape == (len(cases), len(ALL_PROBS))
    _report(what, "quantile error at PROBS", err[:, :len(PROBS)], cases, QUANT_TOL)
    _report(what, "quantile error at the extreme draws", err[:, len(PROBS):], cases, C_EXTREME)


def assert_eq(what, cases, means, icdf):
    """EQ cases: the means [n, 2] and the points icdf [n, 7, 2] of the tabulated posteriors against Beta(a, b)"""
    want, err = eq_reference(cases, icdf)
    _report(what, "mean error", np.asarray(means) - want, cases, MEAN_TOL)
    assert_quantiles(what, cases, err)
    assert (np.diff(icdf[:, :5, 0], axis=1) >= 0).all() and (np.diff(icdf[:, [5, 0, 4, 6], 0], axis=1) >= 0).all(), what


def assert_c0(what, cases, icdf):
    assert_quantiles(what, cases, c0_reference(cases, icdf))


def assert_ratio(pcase, means, icdf):
    """a RATIO case's means [2] and points icdf [7, 2] against mpmath's quadrature of the equivalent single-end event"""
    order = np.argsort(icdf[:, 0], kind="stable")
    mean, cdf, pdf = mp_single_end(pcase[8], icdf[order, 0], icdf[order, 1])
    err = np.zeros(len(ALL_PROBS))
    for k, F, f in zip(order, cdf, pdf):
        err[k] = float((F - mp.mpf(ALL_PROBS[k])) / f)
    print("%s: mean error %.3g, quantile errors %s" % (pcase[0], means[0] - mean, ["%.3g" % e for e in err]))
    assert abs(means[0] - mean) < MEAN_TOL and abs(means[1] - (1.0 - mean)) < MEAN_TOL, pcase[0]
    assert np.abs(err[:len(PROBS)]).max() < QUANT_TOL and np.abs(err[len(PROBS):]).max() < C_EXTREME, (pcase[0], err)


def assert_log_d0(name, c1, c2, got):
    want, bound = log_d0_reference(c1, c2)
    print("%s: log_d0 %.17g, error %.3g, bound %.3g" % (name, got, got - want, bound))
    assert abs(got - want) <= bound, (name, got, want, bound)


H_TOL = 5e-6        # tests/test_exact_compare_ref.py


def assert_pair_shape(name, H0, q):
    """what a pair's name promises of H(0) and of the quantiles q = [median, q(0.025), q(0.975)]"""
    assert q[1] <= q[0] <= q[2], (name, q)
    if name.startswith("self"):
        assert abs(H0 - 0.5) <= H_TOL and abs(q[0]) <= C_EXTREME, (name, H0, q)
    if name.startswith("opposite-ends"):
        assert abs(H0 - 1.0) <= H_TOL and q[2] < -0.99, (name, H0, q)
