"""A fixed-order restatement of the exact comparison of two paired-end exact-mode posteriors
(miso_amd/csrc/kernels_exact_paired_compare.hip with exact_paired.hpp's ExactSecondSegment), built on
_exact_paired_ref.PairedPosterior and _exact_compare_ref's table_cdf / lane_sum / log_prior0: every operation is one
IEEE-754 double operation in the kernel's order, so the device's results can be compared with these bit for bit
(tests/test_gpu_exact_paired_compare.py) and these with mpmath (tests/test_exact_paired_compare_ref.py).
Test infrastructure only: nothing under miso_amd/ imports it.
"""
import numpy as np

from _exact_ref import G, Stats
from _exact_compare_ref import BF_CAP, LN10, lane_sum, table_cdf
from _exact_compare_ref import log_prior0 as _log_prior0_7
from _exact_paired_ref import PairedPosterior, PairedStats, _ratio_pairs

HYPERS = [(1.0, 1.0), (2.0, 5.0)]
ZS = [-0.2, -0.05, 0.0, 0.05, 0.1, 0.2]


class PooledStats:
    """the product of two samples' densities as the kernel holds it: `base` has the pooled exponents, hyperparameters
    h1 + h2 - 1 and c = (a + b) - (n1 + n2), but n, e0, e1 of sample 1; sample 2's n, A and pairs are the second segment"""

    def __init__(self, ps1, ps2):
        f = np.float64
        b1, b2 = ps1.base, ps2.base
        h0p = ((b1.hm0 + f(1.0)) + (b2.hm0 + f(1.0))) - f(1.0)     # (hm + 1 is the hyperparameter again, exactly, for h >= 1)
        h1p = ((b1.hm1 + f(1.0)) + (b2.hm1 + f(1.0))) - f(1.0)
        n12 = b1.n + b2.n
        self.base = Stats(b1.n10 + b2.n10, b1.n01 + b2.n01, n12, b1.e0, b1.e1, h0p, h1p)
        self.base.n = b1.n
        self.c8 = (n12 + ((self.base.hm0 + 1.0) + (self.base.hm1 + 1.0))) * f(0.03125)
        self.n2, self.e20, self.e21 = b2.n, b2.e0, b2.e1
        self.ps1, self.ps2 = ps1, ps2
        self.nd = ps1.nd + ps2.nd


class PairedCompare(PairedPosterior):
    def eval(self, ps, t):
        if not isinstance(ps, PooledStats):
            return super().eval(ps, t)
        t = np.asarray(t, np.float64)
        g, _, x, y, _, _, at = self.point(ps.base, t)
        E = self.exp(-at)
        Ee0, Ee1 = E * ps.e20, E * ps.e21
        den = np.where(t >= 0, ps.e20 + Ee1, Ee0 + ps.e21)
        g = g - ps.n2 * self.log(den)
        P = self.pair_logsum(ps.ps1, x, y) + self.pair_logsum(ps.ps2, x, y)
        return g + P, x, y

    def compare(self, ps1, ps2, zs=()):
        """what exact_paired_compare reports of one pair: [mean1, mean2, log_d0, bayes_factor, log10_bf, H(z) ...]; also
        returns whether A was sample 2"""
        f64 = np.float64
        tabs = [self.tabulate(ps1), self.tabulate(ps2), self.tabulate(PooledStats(ps1, ps2))]
        w1, w2 = (self.point(tb["st"], tb["tR"])[2] - self.point(tb["st"], tb["tL"])[2] for tb in tabs[:2])
        a_is_2 = bool(w2 < w1)      # A: the narrower window in psi, a tie goes to sample 1
        for tb in tabs:
            tb["post"] = self
        lz = [tb["gmax"] + self.log(tb["Z"]) for tb in tabs]
        log_d0 = (lz[2] - lz[0]) - lz[1]
        log_bf = log_prior0(ps1, ps2) - log_d0
        bf = self.exp(log_bf)
        bf = BF_CAP if bf > BF_CAP else bf
        out = [tabs[0]["mean0"], tabs[1]["mean0"], log_d0, bf, log_bf / LN10]
        A, B = (tabs[1], tabs[0]) if a_is_2 else (tabs[0], tabs[1])
        if len(zs):
            t = A["tL"] + A["h"] * np.arange(G + 1, dtype=np.float64)
            _, _, x, y, _, _, _ = self.point(A["st"], t)
            wgt = np.ones(G + 1)
            wgt[0] = wgt[G] = 0.5
            wf = wgt * A["f"]                     # A's own f, kept from its table
            sf = lane_sum(wf)
            for z in zs:
                z = f64(z)
                if a_is_2:      # H = sum w F_1(y + z) / Z_1
                    val = table_cdf(B, x + z, y - z)
                else:           # H = 1 - sum w F_2(x - z) / Z_2
                    val = table_cdf(B, x - z, y + z)
                s = lane_sum(wf * (val / B["Z"])) / sf
                out.append(s if a_is_2 else f64(1.0) - s)
        return np.array(out, dtype=np.float64), a_is_2


def _row7(ps):
    b = ps.base
    return [b.n10, b.n01, b.n, b.e0, b.e1, b.hm0 + np.float64(1.0), b.hm1 + np.float64(1.0)]


def log_prior0(ps1, ps2):
    """log of the prior density of psi_1 - psi_2 at 0, the host's arithmetic"""
    return _log_prior0_7(_row7(ps1), _row7(ps2))


def stats6(ps):
    b = ps.base
    return [b.n10, b.n01, b.e0, b.e1, b.hm0 + np.float64(1.0), b.hm1 + np.float64(1.0)]


# ---- the case list: (name, sample 1, sample 2), a sample = (n10, n01, A0, A1, pairs) ----

def _rnd(seed, n):
    return np.random.default_rng(seed).uniform(1e-5, 0.0133, size=(n, 2))


A = (60000.0, 43000.0)
A10 = (66000.0, 39000.0)        # about 10 % from A, in opposite directions
TWO_MODE = (0, 0, float(np.exp(6.0)), 1.0, _ratio_pairs(6, 4.5))
TWO_MODE_MIRRORED = (0, 0, 1.0, float(np.exp(6.0)), _ratio_pairs(6, -4.5))


def cases():
    return [
        ("no-pairs/no-pairs", (11, 5, A[0], A[1], []), (3, 9, A[0], A[1], [])),
        ("no-pairs-big/no-pairs", (400, 300, A[0], A[1], []), (410, 290, A[0], A[1], [])),
        ("3-0-A50-1/no-pairs", (3, 0, 50.0, 1.0, []), (0, 0, 50.0, 1.0, [])),
        ("15/1", (2, 1, 52000.0, 61000.0, _rnd(1, 15)), (3, 4, 52000.0, 61000.0, [(0.011, 0.0004)])),
        ("16/1", (2, 1, 52000.0, 61000.0, _rnd(2, 16)), (3, 4, 52000.0, 61000.0, [(0.011, 0.0004)])),
        ("17/1", (2, 1, 52000.0, 61000.0, _rnd(3, 17)), (3, 4, 52000.0, 61000.0, [(0.011, 0.0004)])),
        ("two-mode/narrow", TWO_MODE, (40, 30, A[0], A[1], _rnd(4, 40))),
        ("narrow/two-mode-mirrored", (40, 30, A[0], A[1], _rnd(4, 40)), TWO_MODE_MIRRORED),
        ("A-10-percent-apart", (11, 5, A[0], A[1], _rnd(5, 30)), (9, 8, A10[0], A10[1], _rnd(6, 25))),
        ("few-hundred", (60, 45, A[0], A[1], _rnd(7, 300)), (50, 50, A10[0], A10[1], _rnd(8, 20))),
        ("50000+50000/3", (30000, 20000, A[0], A[1], [(0.012, 0.004)] * 30000 + [(0.003, 0.011)] * 20000),
         (2, 1, A[0], A[1], _rnd(9, 3))),
    ]


def paired_stats(sample, hyper):
    n10, n01, A0, A1, pairs = sample
    return PairedStats(n10, n01, A0, A1, hyper[0], hyper[1], pairs)
