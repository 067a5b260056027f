"""A fixed-order restatement of the quantiles of delta psi between two groups of replicates from the exact posteriors
(miso_amd/csrc/kernels_exact_delta_groups.hip), built on the restatement of the pairwise quantiles: the
mixture's CDF is the a-major mean of the pairwise CDFs (tests/_exact_delta_ref.py single_cdf), summed from 0.0 and divided once
by float(n1 n2), and the search is _exact_delta_ref.search on it.  Every operation is one IEEE-754 double operation in the
kernels' order, so the device's results can be compared with these bit for bit (tests/test_gpu_exact_delta_groups.py) and
these with mpmath (tests/test_exact_delta_groups_ref.py).  Test infrastructure only: nothing under miso_amd/ imports it.
"""
import numpy as np

from _exact_delta_ref import PROBS, search, single_cdf
from _exact_ref import eligible

# the issue's three cases: counts (n10, n01, n11) of group 1's replicates, of group 2's; effective lengths (179, 140)
EFF = (179, 140)
GROUP_CASES = {
    "disagreeing": (((20, 80, 30), (80, 20, 30), (85, 18, 25)), ((22, 75, 40),)),
    "sharp+wide": (((1, 100000, 0), (3, 9, 20)), ((0, 60000, 20000), (11, 5, 17), (0, 0, 0))),
    "3x3agreeing": (((400, 300, 300), (410, 290, 310), (395, 305, 290)), ((300, 400, 300), (290, 410, 310), (305, 395, 290))),
}


def rows_of(counts, hyper, eff=EFF):
    """a group's replicates in miso_selftest_exact's layout: (n10, n01, n, e0, e1, h0, h1) each"""
    return [[float(c[0]), float(c[1]), float(sum(c)), float(eff[0]), float(eff[1]), float(hyper[0]), float(hyper[1])] for c in counts]


def case_rows(name, hyper):
    g1, g2 = GROUP_CASES[name]
    return rows_of(g1, hyper), rows_of(g2, hyper)


def comparable(rows1, rows2):
    """every row eligible for the exact mode, and all with bit-equal (e0, e1)"""
    rows = [np.asarray(r, np.float64) for r in list(rows1) + list(rows2)]
    return all(eligible(False, 2, r[3:5], r[5:7]) and r[3:5].tobytes() == rows[0][3:5].tobytes() for r in rows)


class MixtureCdf:
    """H(z) = (sum_a sum_b H_ab(z)) / float(n1 n2): from 0.0, a outer and b inner, divided once.  A pair of rows that occurs
    more than once is tabulated once (cache: shared between mixtures of one test run if the caller passes one in)."""

    def __init__(self, post, rows1, rows2, cache=None):
        cache = {} if cache is None else cache
        self.pairs = []
        for r1 in rows1:
            for r2 in rows2:
                key = (np.asarray(r1, np.float64).tobytes(), np.asarray(r2, np.float64).tobytes())
                if key not in cache:
                    cache[key] = single_cdf(post, r1, r2)
                self.pairs.append(cache[key])
        self.n1, self.n2 = len(rows1), len(rows2)

    def __call__(self, z):
        s = np.float64(0.0)
        for H in self.pairs:
            s = s + H(z)
        return s / np.float64(self.n1 * self.n2)

    def means(self):
        """(m1, m2): the replicates' posterior means of psi (the tables' own mean0) added in replicate order, divided once"""
        m1, m2 = np.float64(0.0), np.float64(0.0)
        for a in range(self.n1):
            m1 = m1 + self.pairs[a * self.n2].tabs[0]["mean0"]
        for b in range(self.n2):
            m2 = m2 + self.pairs[b].tabs[1]["mean0"]
        return m1 / np.float64(self.n1), m2 / np.float64(self.n2)


def group_delta(post, rows1, rows2, probs=PROBS, zs=(), cache=None):
    """the output row of one comparable event: [m1, m2, q(p) ..., H(0.0), H(z) ...]; None when the event is not comparable"""
    if not comparable(rows1, rows2):
        return None
    H = MixtureCdf(post, rows1, rows2, cache)
    res = search(H, probs)
    m1, m2 = H.means()
    return np.array([m1, m2] + list(res) + [H(np.float64(z)) for z in zs], dtype=np.float64)
