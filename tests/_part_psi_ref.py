"""CPU restatement of the isoform-group passes (miso_batch_summarize_isoform_groups, miso_batch_compare_pairs_isoform_groups;
miso_amd/csrc/kernels_groups.hip).  Test infrastructure only.

A group is (event, mask); its draw of row s is ((0.0 + psi[s, k1]) + psi[s, k2]) + ... over the mask's isoforms ascending,
then + 0.0.  as_text: every member first as "%.4f" prints it and float() reads it back.

* ``group_column``  the column, one explicit add per member.
* ``summarize``     (mean, ci_low, ci_high): the device's strided-then-folded mean (_summary_ref.tree_mean), the order
                    statistics of the sorted column at the strict ranks; three NaN when a draw is not finite.
* ``compare``       the all-pairs statistics of two columns with all M differences formed outright (_pairs_ref.brute).
"""
import numpy as np

import _pairs_ref as PR
from _summary_ref import py2_round, tree_mean


def mask_of(isoforms):
    m = 0
    for k in isoforms:
        m |= 1 << int(k)
    return m


def members(mask):
    return [k for k in range(64) if (mask >> k) & 1]


def as_read(x):
    """what float() makes of "%.4f" % v, element by element"""
    x = np.asarray(x, np.float64)
    return np.array([float("%.4f" % v) for v in x.ravel().tolist()]).reshape(x.shape)


def group_column(samples, mask, as_text=False):
    """samples [S, K] -> v [S]"""
    x = np.asarray(samples, np.float64)
    v = np.zeros(x.shape[0])
    with np.errstate(invalid="ignore"):
        for k in members(mask):
            assert k < x.shape[1]
            c = as_read(x[:, k]) if as_text else x[:, k]
            v = v + c
        return v + 0.0


def strict_ranks(S, level):
    alpha = 1 - level
    lo, hi = py2_round((alpha / 2) * S) - 1, py2_round((1 - alpha / 2) * S) - 1
    assert lo > 0 and hi > 0 and hi < S
    return lo, hi


def summarize(samples, mask, level=0.95, as_text=False):
    v = group_column(samples, mask, as_text)
    if not np.isfinite(v).all():
        return (float("nan"),) * 3
    lo, hi = strict_ranks(len(v), level)
    s = np.sort(v)
    return float(tree_mean(v)), float(s[lo]), float(s[hi])


def compare(samples1, samples2, mask, level=0.95, taus=(), as_text=False):
    """_pairs_ref.brute's tuple for the group's two columns"""
    return PR.brute(group_column(samples1, mask, as_text), group_column(samples2, mask, as_text), level, taus)


def same3(x, y):
    """two (mean, ci_low, ci_high) agree bit for bit (every NaN the same)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return all((a != a and b != b) or PR.bits(a) == PR.bits(b) for a, b in zip(x, y))
