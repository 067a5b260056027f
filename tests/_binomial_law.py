"""What tests/test_binomial_law.py (CPU) and tests/test_gpu_binomial_law.py share: the cases, the exact law and the bound.

A draw of include/miso_binomial.h is a function of 32-bit words, so the law its draws follow can be COUNTED: one BTRS trial
reads two words -- the first, U, fixes the candidate k, and the trial accepts for an initial segment [0, V*] of the second --,
the inversion reads one.  hist[k] = the sum over the enumerated U with k(U) = k of V* + 1 (BTRS) or of 1 (inversion);
hist / total is the induced law, exact up to the 2^-32 grain of the words when every U is enumerated and up to stride 2^-32
when every stride-th one is (oracle/miso_oracle.h orc_binomial_law, include/miso_amd.h miso_selftest_binomial_law).

The bound on |hist[k] / total - pmf(k)| is derived, not tuned:

    (2 stride + 2) 2^-32 / accept + restarts / enumerated + 1e-12

* k's words U form an interval (k(U) does not decrease: counted in info["not_monotone"], asserted 0); each of its two ends is
  known to one enumerated word: 2 stride words of 2^-32 each.
* V* is off by at most one word at either end of its own grain: 2 words.  (A probe around V* that contradicts the initial
  segment, info["segment_bad_near"], would widen this by the probes' reach, 3 words; far probes must all agree.)
* accept = total / (enumerated 2^32), the probability that a BTRS trial accepts: the law is the accepted mass renormalised
  (1 for the inversion).
* a restarted inversion search draws from another word: its whole weight, restarts / enumerated, is given away.
* 1e-12: the log-factorial table (~1e-13 relative, tests/test_detmath.py) and the reference pmf.

Cumulative sums are held to twice that: a drift too small for any single bin shows there.

The exact pmf is scipy.stats.binom.pmf in float64 (boost's ibeta_derivative), which `exact_pmf` checks against mpmath at 50
digits -- at 0, n, the mode and on both flanks, for the very double r -- to 1e-13 absolute on every call.  The law of p > 1/2 is
r = fl(1 - p)'s reflected, and 1 - p is exact for p in [1/2, 1]."""
import functools

import mpmath
import numpy as np
from scipy import stats

INV, BTRS = 0, 1
TWO32 = 2.0 ** 32

# (n, p, the routine miso_binomial takes: asserted from info, not computed here)
CASES = [
    (688, 0.31, BTRS), (20, 0.5, BTRS), (21, 0.5, BTRS), (1000, 0.0101, BTRS), (1000, 0.0099, INV), (100000, 0.4, BTRS),
    (60000, 0.97, BTRS), (100000, 0.00011, BTRS), (100000, 0.000099, INV), (40, 0.25, BTRS), (3, 0.5, INV),
    # n r AT the switch: fl(20 * 0.5) = 10 exactly, and fl(1000 * fl(0.01)) = fl(10.0000000000000002...) = 10: not below 10, BTRS
    (1000, 0.01, BTRS),
    (19, 0.5, INV),                   # the largest inversion at p = 1/2
    (1, 0.7, INV), (2, 0.5, INV),
    (50, 0.999, INV),                 # reflected
    (100000, 0.5, BTRS),              # the table is read at lf[n] when k is 0
    (100000, 1e-12, INV),
    (1000, 1 - 2.0 ** -53, INV), (1000, 1e-310, INV),   # q rounds to 1: every draw is 0 (n after reflection)
    (30, 1 / 3, BTRS), (64, 0.2, BTRS),                 # small-n BTRS, where the hat is tightest
    (200, 0.05, BTRS),                # fl(200 * fl(0.05)) = fl(10.0000000000000005...) = 10 as well
    (200, 0.0501, BTRS),
]
DEGENERATE = [(1000, 1 - 2.0 ** -53), (1000, 1e-310)]


def case_id(c):
    return "n%d-p%r" % (c[0], c[1])


def reduced(p):
    return 1.0 - p if p > 0.5 else p


def _mp_pmf(n, r, k):
    with mpmath.workdps(50):
        r = mpmath.mpf(r)
        return float(mpmath.binomial(n, k) * r ** k * (1 - r) ** (n - k))


@functools.lru_cache(maxsize=None)
def exact_pmf(n, p):
    """pmf of Binomial(n, p) at 0 .. n in float64 (see the module's text), read-only"""
    r = reduced(p)
    pm = stats.binom.pmf(np.arange(n + 1), n, r)
    sd = np.sqrt(n * r * (1 - r))
    mode = int((n + 1) * r)
    ks = {0, 1, n - 1, n, mode, min(mode + 1, n)}
    for z in (0.5, 1, 2, 3, 4, 5, 6, 8):
        ks |= {int(mode - z * sd), int(mode + z * sd) + 1}
    for k in sorted(k for k in ks if 0 <= k <= n):
        assert abs(pm[k] - _mp_pmf(n, r, k)) <= 1e-13, (n, p, k, pm[k], _mp_pmf(n, r, k))
    if p > 0.5:
        pm = pm[::-1].copy()
    pm.setflags(write=False)
    return pm


_checker_laws = {}


def checker_law(orc, n, p, stride):
    """the checker's enumeration (hist, info), made once per run of the suite and left unchanged"""
    key = (n, p, stride)
    if key not in _checker_laws:
        hist, info = orc.binomial_law(n, p, stride)
        hist.setflags(write=False)
        _checker_laws[key] = (hist, info)
    return _checker_laws[key]


def accept(info):
    return info["total"] / (info["enumerated"] * TWO32) if info["regime"] == BTRS else 1.0


def bound(info, stride):
    """the module's bound for one enumeration; the assumptions it rests on are asserted here, where they are used"""
    assert info["not_monotone"] == 0, info                     # k's words are an interval
    assert info["segment_bad_far"] == 0, info                  # the accepted V are [0, V*] ...
    words = 2 * stride + 2 + (3 if info["segment_bad_near"] else 0)   # ... to the word, or within the near probes' reach
    if info["regime"] == BTRS:
        assert info["segment_checked"] >= 0.9 * (info["enumerated"] // 256), info   # (words with k out of range are not probed)
    return words / TWO32 / accept(info) + info["restarts"] / info["enumerated"] + 1e-12


def errors(hist, info, n, p):
    """(worst |hist[k] / total - pmf(k)|, its k, worst |cumulative sum - CDF|, its k), bins reflected for p > 1/2"""
    assert int(hist.sum()) == info["total"] and len(hist) == n + 1
    h = hist[::-1] if p > 0.5 else hist
    d = h.astype(np.longdouble) / np.longdouble(info["total"]) - exact_pmf(n, p).astype(np.longdouble)
    c = np.cumsum(d)
    kd, kc = int(np.abs(d).argmax()), int(np.abs(c).argmax())
    return float(abs(d[kd])), kd, float(abs(c[kc])), kc


def check_law(hist, info, n, p, stride, regime):
    """every assertion that the CPU and the GPU test make of one enumeration; returns what they print"""
    assert info["regime"] == regime, (n, p, info)
    assert info["enumerated"] == 2 ** 32 // stride
    assert info["restarts"] == 0, (n, p, info)                 # the rule for these cases (the bound accounts for any)
    if regime == BTRS:
        assert accept(info) >= 0.70, (n, p, accept(info))
    else:
        assert info["total"] == info["enumerated"] and info["out_of_range"] == 0
    b = bound(info, stride)
    e, ke, c, kc = errors(hist, info, n, p)
    line = "n=%d p=%r %s stride=%d accept=%.4f bin err %.3g at k=%d (bound %.3g), cdf err %.3g at k=%d (bound %.3g)" % (
        n, p, "BTRS" if regime == BTRS else "INV", stride, accept(info), e, ke, b, c, kc, 2 * b)
    print(line)
    assert e <= b, line
    assert c <= 2 * b, line
    if (n, p) in DEGENERATE:
        assert int(hist[0]) == info["total"], (n, p, hist[:4])
    return line
