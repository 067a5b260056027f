"""The exact comparison of two paired-end exact-mode batches on the device (csrc/kernels_exact_paired_compare.hip,
miso_batch_compare_exact_paired).

Bit for bit against its restatement (tests/_exact_paired_compare_ref.py, itself checked against mpmath in
tests/test_exact_paired_compare_ref.py): caller-given elements (miso_selftest_exact_paired_compare) on the case list and on
the drawing-pair counts around the block of 16 and the chunk of 64, and whole batches.  Then the contract: the KDE
comparison is untouched, the errors, and H(z) against the mode's own draws.
"""
import numpy as np
import pytest

import miso_amd
from miso_amd import capi
from _exact_paired_ref import PairedStats, ass_sums, fragment_dist
from _exact_paired_compare_ref import HYPERS, ZS, PairedCompare, cases, paired_stats, stats6
from _problems import simulate_pe

pytestmark = pytest.mark.gpu

READ_LEN = 36
MEAN = 250.0
ISOLEN, NOEXONS = [1500, 1000], [3, 2]
Z8 = [-0.3, -0.2, -0.05, 0.0, 0.05, 0.1, 0.2, 0.3]
AA = (60000.0, 43000.0)


@pytest.fixture(scope="module")
def post(orc):
    return PairedCompare(orc)


def _rnd(seed, n):
    return np.random.default_rng(seed).uniform(1e-5, 0.0133, size=(n, 2))


def _check(post, pairs, zs):
    """pairs: [(PairedStats of sample 1, of sample 2)] -> one launch, every element against the restatement; returns which
    elements had A = sample 2"""
    out = capi.selftest_exact_paired_compare([stats6(a) for a, _ in pairs], [a.m for a, _ in pairs],
                                             [stats6(b) for _, b in pairs], [b.m for _, b in pairs], zs)
    assert out.shape == (len(pairs), 5 + len(zs))
    a2 = []
    for j, (a, b) in enumerate(pairs):
        want, a_is_2 = post.compare(a, b, zs)
        assert np.array_equal(out[j], want), (j, a.nd, b.nd, out[j], want)
        a2.append(a_is_2)
    return a2


@pytest.mark.parametrize("hyper", HYPERS, ids=["h11", "h25"])
def test_case_list_bit_exact(post, hyper):
    pairs = [(paired_stats(s1, hyper), paired_stats(s2, hyper)) for _, s1, s2 in cases()]
    a2 = _check(post, pairs, ZS)
    assert any(a2) and not all(a2)           # both outcomes of "A = sample 2"


@pytest.mark.parametrize("counts", [(0, 1, 15, 16), (17, 63, 64), (65, 129)], ids=lambda c: "-".join(map(str, c)))
def test_block_and_chunk_edges_bit_exact(post, counts):
    """nd drawing pairs in sample 1 against nd + 1 in sample 2, and swapped"""
    pairs = []
    for nd in counts:
        a = PairedStats(5, 3, AA[0], AA[1], 1.0, 1.0, _rnd(100 + nd, nd))
        b = PairedStats(2, 6, 52000.0, 61000.0, 2.0, 5.0, _rnd(200 + nd, nd + 1))
        pairs += [(a, b), (b, a)]
    _check(post, pairs, ZS)


def test_asymmetric_counts_a_tie_and_nz(post):
    none1 = PairedStats(9, 4, AA[0], AA[1], 1.0, 1.0, [])
    none2 = PairedStats(3, 8, AA[0], AA[1], 1.0, 1.0, [])
    many = PairedStats(2, 1, AA[0], AA[1], 1.0, 1.0, _rnd(31, 65))
    same = PairedStats(7, 6, AA[0], AA[1], 2.0, 5.0, _rnd(32, 20))
    pairs = [(none1, many), (many, none2), (same, same)]
    for zs in ([], [0.05], Z8):
        a2 = _check(post, pairs, zs)
    assert a2[2] is False                    # a tie goes to sample 1
    assert a2[0] != a2[1]


def test_one_thousand_pairs_bit_exact(post):
    big = PairedStats(120, 80, AA[0], AA[1], 1.0, 1.0, _rnd(41, 1000))
    small = PairedStats(4, 4, 66000.0, 39000.0, 1.0, 1.0, _rnd(42, 7))
    _check(post, [(big, small)], [0.1])


def test_second_launch_slice_bit_equal():
    """The driver launches in slices of 8192 pairs; a slice after the first indexes its rows of A's f by the workgroup and
    its outputs by first + workgroup.  8192 + 3 elements, the case list's small elements (at most 40 drawing pairs) under
    both hyperparameter settings tiled, one z so that the row buffer is used: every row equals, bit for bit, the row of
    the same element in a call on the distinct elements alone (which test_case_list_bit_exact holds against the
    restatement)."""
    distinct = [(paired_stats(s1, h), paired_stats(s2, h)) for h in HYPERS for _, s1, s2 in cases()
                if max(len(s1[4]), len(s2[4])) <= 40]
    assert len(distinct) == 18 and 8192 % len(distinct) != 0     # the second slice starts inside the tiling

    def run(pairs):
        return capi.selftest_exact_paired_compare([stats6(a) for a, _ in pairs], [a.m for a, _ in pairs],
                                                  [stats6(b) for _, b in pairs], [b.m for _, b in pairs], [0.05])
    want = run(distinct)
    n = 8192 + 3
    got = run([distinct[j % len(distinct)] for j in range(n)])
    assert got.shape == (n, 6)
    assert np.array_equal(got, want[np.arange(n) % len(distinct)])
    assert len({row.tobytes() for row in want}) == len(distinct)  # (no two elements share a row: a misplaced one shows)


# ---- whole batches ----

class Problem:
    """a two-isoform paired-end problem for add_problem: n10 / n01 pairs compatible with one isoform, nd with both, their
    fragment lengths drawn inside the batch's fragment-length range (tests/test_gpu_exact_paired.py's)"""

    def __init__(self, rng, start, il, n10, n01, nd, hyper=None):
        N = n10 + n01 + nd
        self.match = np.zeros((N, 2))
        self.fraglen = np.zeros((N, 2), np.int32)
        kind = rng.permutation(np.array([0] * n10 + [1] * n01 + [2] * nd))
        for i, k in enumerate(kind):
            f = rng.integers(start, start + il, size=2)
            if k in (0, 2):
                self.match[i, 0], self.fraglen[i, 0] = 1.0, f[0]
            if k in (1, 2):
                self.match[i, 1], self.fraglen[i, 1] = 1.0, f[1]
        self.n10, self.n01, self.hyper = n10, n01, hyper
        draws = [i for i in range(N) if kind[i] == 2]
        self.order = sorted(draws, key=lambda i: (self.fraglen[i, 0], self.fraglen[i, 1], i))

    def stats(self, start, prob):
        hyper = self.hyper or (1.0, 1.0)
        pairs = [(prob[self.fraglen[i, 0] - start], prob[self.fraglen[i, 1] - start]) for i in self.order]
        A = ass_sums(ISOLEN, start, len(prob))
        return PairedStats(self.n10, self.n01, A[0], A[1], hyper[0], hyper[1], pairs)


NDS = [0, 1, 15, 16, 17, 40, 63, 64, 65, 129]
THREE = (5, 17, 29)            # three-isoform events
ONLY_IN_2 = (8, 21)            # a hyperparameter below 1 in sample 1: eligible in sample 2 only
ONLY_IN_1 = (12,)              # ... in sample 2
N_EVENTS = 40


def _batches(orc, chains=2, iters=310, burn=10, lag=1, exact1=True, exact2=True):
    out = []
    for which, (var, seed) in enumerate(((900.0, 77), (1600.0, 78))):
        start, prob = fragment_dist(MEAN, var, 4.0, READ_LEN)
        rng = np.random.default_rng(50 + which)
        b = miso_amd.Batch(READ_LEN, paired=True, mean=MEAN, var=var, exact_paired=(exact1, exact2)[which], chains=chains,
                           iters=iters, burn=burn, lag=lag)
        probs = []
        for i in range(N_EVENTS):
            if i in THREE:
                ex3, iso3, _, pos3, cig3 = simulate_pe(orc, 3, 120, mean=MEAN, var=var, seed=5 + i)
                b.add_event(miso_amd.Gene(ex3, iso3), pos3, cig3)
                probs.append(None)
                continue
            hyper = (2.0, 5.0) if i % 4 == 1 else None
            if i in (ONLY_IN_2, ONLY_IN_1)[which]:
                hyper = (0.5, 0.5)
            nd = NDS[(i + 3 * which) % len(NDS)]
            q = Problem(rng, start, len(prob), int(rng.integers(0, 30)), int(rng.integers(0, 30)), nd, hyper=hyper)
            b.add_problem(q.match, ISOLEN, NOEXONS, fraglen=q.fraglen, hyper=q.hyper)
            probs.append(q)
        b.run(seed=seed, first_event_id=900)
        out.append((b, probs, start, prob))
    return out


def test_batches_bit_exact_and_the_kde_comparison_untouched(orc, post):
    (b1, p1, s1, f1), (b2, p2, s2, f2) = _batches(orc)
    b1.compare(b2)
    before = [b1.comparison(i) for i in range(N_EVENTS)]
    b1.compare_exact_paired(b2, ZS)
    assert b1.last_kernels().split(",")[-1] == "exact_paired_compare"
    assert b1.compare_ms()[1] > 0.0
    n_cmp = 0
    for i in range(N_EVENTS):
        got = b1.exact_comparison(i)
        if i in THREE or i in ONLY_IN_1 or i in ONLY_IN_2:
            assert got is None, i
            continue
        n_cmp += 1
        want, _ = post.compare(p1[i].stats(s1, f1), p2[i].stats(s2, f2), ZS)
        assert np.array_equal(np.concatenate([got[:5], got[5]]), want), (i, got, want)
        assert got[0] == b1.exact_summary(i)[0][0] and got[1] == b2.exact_summary(i)[0][0], i
    assert n_cmp == N_EVENTS - len(THREE) - len(ONLY_IN_1) - len(ONLY_IN_2)
    b1.compare(b2)
    for i in range(N_EVENTS):
        for a, b in zip(before[i], b1.comparison(i)):
            assert np.array_equal(a, b, equal_nan=True), i
    # a second call with other z replaces the first
    b1.compare_exact_paired(b2, [0.3])
    got = b1.exact_comparison(0)
    want, _ = post.compare(p1[0].stats(s1, f1), p2[0].stats(s2, f2), [0.3])
    assert len(got[5]) == 1 and np.array_equal(np.concatenate([got[:5], got[5]]), want)
    # ... and the single-end comparison stays the error it is on paired batches
    with pytest.raises(miso_amd.InternalError, match="Invalid value"):
        b1.compare_exact(b2, ZS)


def test_errors(orc):
    (b1, _, _, _), (b2, _, _, _) = _batches(orc, exact2=False)
    for a, b in ((b1, b2), (b2, b1)):        # the mode is missing on either side
        with pytest.raises(miso_amd.InternalError, match="Invalid value"):
            a.compare_exact_paired(b, ZS)
    b3 = _batches(orc)[1][0]
    for zs in ([1.0], [-1.0], [float("nan")], [0.01 * k for k in range(9)]):
        with pytest.raises(miso_amd.InternalError, match="Invalid value"):
            b1.compare_exact_paired(b3, zs)
    short = miso_amd.Batch(READ_LEN, paired=True, mean=MEAN, var=900.0, exact_paired=True, chains=2, iters=310, burn=10, lag=1)
    start, prob = fragment_dist(MEAN, 900.0, 4.0, READ_LEN)
    q = Problem(np.random.default_rng(1), start, len(prob), 3, 4, 5)
    short.add_problem(q.match, ISOLEN, NOEXONS, fraglen=q.fraglen)
    short.run(seed=1, first_event_id=0)
    with pytest.raises(miso_amd.InternalError, match="Invalid value"):
        b1.compare_exact_paired(short, ZS)   # event-count mismatch
    se = []
    for seed in (1, 2):
        b = miso_amd.Batch(READ_LEN, exact=True, chains=2, iters=310, burn=10, lag=1)
        b.add_problem(np.array([[1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]), [1500, 1000], [3, 2])
        b.run(seed=seed, first_event_id=0)
        se.append(b)
    with pytest.raises(miso_amd.InternalError, match="Invalid value"):
        se[0].compare_exact_paired(se[1], ZS)   # single-end batches
    good = PairedStats(1, 1, AA[0], AA[1], 1.0, 1.0, [(0.01, 0.002)])
    bad_h = [1.0, 1.0, AA[0], AA[1], 0.5, 1.0]
    with pytest.raises(miso_amd.InternalError, match="Invalid value"):
        capi.selftest_exact_paired_compare([stats6(good)], [good.m], [bad_h], [good.m], ZS)
    with pytest.raises(miso_amd.InternalError, match="Invalid value"):
        capi.selftest_exact_paired_compare([stats6(good)], [[(0.01, 2.0 ** -64)]], [stats6(good)], [good.m], ZS)
    with pytest.raises(miso_amd.InternalError, match="Invalid value"):
        capi.selftest_exact_paired_compare([stats6(good)], [good.m], [stats6(good)], [good.m], [1.5])


def test_cdf_against_the_modes_own_draws(orc):
    """S = 5000 independent rows per sample: the fraction of index-paired differences <= z is a binomial proportion with
    success probability H(z), so |fraction - H| <= 5 sd + 1 / S (5 sd: 6e-7 per comparison, ~200 comparisons; the bound of
    tests/test_gpu_exact_compare.py)"""
    S = 5000
    (b1, _, _, _), (b2, _, _, _) = _batches(orc, chains=2, iters=2500, burn=0, lag=1)
    b1.compare_exact_paired(b2, ZS)
    worst, n = 0.0, 0
    for i in range(N_EVENTS):
        got = b1.exact_comparison(i)
        if got is None:
            continue
        x1, x2 = b1.result(i).samples[:, 0], b2.result(i).samples[:, 0]
        assert len(x1) == len(x2) == S
        d = x1 - x2
        n += 1
        for z, h in zip(ZS, np.clip(got[5], 0.0, 1.0)):
            frac = float((d <= z).mean())
            bound = 5 * np.sqrt(h * (1 - h) / S) + 1.0 / S
            worst = max(worst, abs(frac - h) / bound)
            assert abs(frac - h) <= bound, (i, z, frac, h, bound)
    print("worst |fraction - H| / bound %.3f over %d events x %d points" % (worst, n, len(ZS)))
