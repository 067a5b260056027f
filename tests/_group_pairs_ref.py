"""CPU restatement of the pooled all-pairs comparison of two groups of replicates (miso_batch_compare_pairs_groups,
miso_amd/csrc/kernels_compare_pairs_groups.hip): tests/_pairs_ref.py's restatements on the concatenated
columns.  A = the group-1 samples' columns taken together, B the group-2 ones, D the multiset of the IEEE doubles a - b.

* ``brute`` / ``bisect``   _pairs_ref's, over np.concatenate of each group's columns.
* ``refusal``              the message with which the pass refuses a call, or None: _pairs_ref's with the group limit.
* ``group_columns``        the columns the tests use: n1 + n2 columns of one _pairs_ref kind, another seed per replicate.
* ``disagreeing``          one group-1 replicate near psi = 0.2, two near 0.8, one group-2 replicate near 0.2.
"""
import numpy as np

import _pairs_ref as PR

MAX_GROUP_DRAWS, MAX_TAU = 16384, PR.MAX_TAU


def pooled(cols):
    return np.concatenate([np.asarray(c, np.float64) for c in cols])


def brute(cols1, cols2, level=0.95, taus=()):
    return PR.brute(pooled(cols1), pooled(cols2), level, taus)


def bisect(cols1, cols2, level=0.95, taus=()):
    return PR.bisect(pooled(cols1), pooled(cols2), level, taus)


def refusal(n1, n2, S, level, taus):
    msg = PR.refusal(1, 1, level, taus)
    if msg is not None:
        return msg
    for g, n in ((1, n1), (2, n2)):
        if n * S > MAX_GROUP_DRAWS:
            return "group %d: Too many samples for the pooled all-pairs comparison" % g
    return None


def group_columns(kind, n1, n2, S, seed=0):
    """([n1 columns of S], [n2 columns of S]): replicate r of either group is _pairs_ref.columns(kind, S, S, seed + r)'s"""
    g1 = [PR.columns(kind, S, S, seed=seed + 10 * r)[0] for r in range(n1)]
    g2 = [PR.columns(kind, S, S, seed=seed + 10 * r + 5)[1] for r in range(n2)]
    return g1, g2


def disagreeing(S=200):
    """replicates that disagree: the pooled law is bimodal, its quantiles no function of the pairwise ones"""
    rng = np.random.default_rng(7)
    g1 = [np.round(rng.beta(20, 80, S), 4), np.round(rng.beta(80, 20, S), 4), np.round(rng.beta(80, 20, S), 4)]
    g2 = [np.round(rng.beta(20, 80, S), 4)]
    return g1, g2
