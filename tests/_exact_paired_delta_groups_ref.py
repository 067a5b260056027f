"""A fixed-order restatement of the quantiles of delta psi between two groups of PAIRED-END replicates from the exact posteriors
(miso_amd/csrc/kernels_exact_paired_delta_groups.hip), built on the restatement of the pairwise
quantiles: the mixture's CDF is the a-major mean of the pairwise CDFs (tests/_exact_delta_ref.py paired_cdf), summed from 0.0
and divided once by float(n1 n2), and the search is _exact_delta_ref.search on it.  It holds no arithmetic of its own beyond
that sum, so the device's results can be compared with these bit for bit (tests/test_gpu_exact_paired_delta_groups.py) and
these with mpmath (tests/test_exact_paired_delta_groups_ref.py).  Test infrastructure only: nothing under miso_amd/ imports it.
"""
import numpy as np

from _exact_delta_ref import PROBS, paired_cdf, search
from _exact_paired_compare_ref import A, A10, TWO_MODE, _rnd, paired_stats
from _exact_paired_ref import eligible

# the issue's two cases: group 1's samples, group 2's; a sample = (n10, n01, A0, A1, pairs)
GROUP_CASES = {
    "disagreeing": (((20, 80, A[0], A[1], _rnd(21, 30)), (80, 20, A[0], A[1], _rnd(22, 17)), (85, 18, A10[0], A10[1], _rnd(23, 64))),
                    ((22, 75, A[0], A[1], _rnd(24, 40)),)),
    "two-mode": ((TWO_MODE, (40, 30, A[0], A[1], _rnd(4, 40))),
                 ((2, 1, A[0], A[1], _rnd(9, 3)), (3, 9, A[0], A[1], []), (80, 20, A[0], A[1], _rnd(22, 17)))),
}


def case_stats(name, hyper):
    """(group 1's PairedStats, group 2's) of a case"""
    g1, g2 = GROUP_CASES[name]
    return [paired_stats(s, hyper) for s in g1], [paired_stats(s, hyper) for s in g2]


def replicate(sample, hyper):
    """one event of one replicate as capi.exact_paired_delta_groups takes it: (stats6 row, pairs)"""
    n10, n01, A0, A1, pairs = sample
    return [float(n10), float(n01), float(A0), float(A1), float(hyper[0]), float(hyper[1])], np.asarray(pairs, np.float64).reshape(-1, 2)


class _TablesOnce:
    """a PairedCompare whose tabulate() keeps what it made of a PairedStats object: a replicate takes part in several pairs and
    is tabulated once, as on the device; everything else is the posterior's own"""

    def __init__(self, pc):
        self._pc, self._tabs, self._cdfs = pc, {}, {}

    def __getattr__(self, name):
        return getattr(self._pc, name)

    def cdf(self, ps1, ps2):
        """paired_cdf of a pair of PairedStats objects, made once (a DeltaCdf keeps the values it has computed)"""
        key = (id(ps1), id(ps2))
        if key not in self._cdfs:
            self._cdfs[key] = (ps1, ps2, paired_cdf(self, ps1, ps2))
        return self._cdfs[key][2]

    def tabulate(self, ps):
        if id(ps) not in self._tabs:
            self._tabs[id(ps)] = (ps, self._pc.tabulate(ps))
        return dict(self._tabs[id(ps)][1])


class PairedMixtureCdf:
    """H(z) = (sum_a sum_b H_ab(z)) / float(n1 n2): from 0.0, a outer and b inner, divided once"""

    def __init__(self, pc, stats1, stats2):
        once = pc if isinstance(pc, _TablesOnce) else _TablesOnce(pc)
        self.pairs = [once.cdf(p1, p2) for p1 in stats1 for p2 in stats2]
        self.n1, self.n2 = len(stats1), len(stats2)

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


def comparable(stats1, stats2):
    """every replicate eligible for the paired exact mode"""
    return all(eligible(2, (ps.base.e0, ps.base.e1), (ps.base.hm0 + 1.0, ps.base.hm1 + 1.0)) for ps in list(stats1) + list(stats2))


def group_delta(pc, stats1, stats2, probs=PROBS, zs=()):
    """the output row of one comparable event: [m1, m2, q(p) ..., H(0.0), H(z) ...]; None when the event is not comparable"""
    if not comparable(stats1, stats2):
        return None
    H = PairedMixtureCdf(pc, stats1, stats2)
    res = search(H, probs)
    m1, m2 = H.means()
    return np.array([m1, m2] + list(res) + [H(np.float64(z)) for z in zs], dtype=np.float64)
