"""GPU: the all-pairs comparison (miso_batch_compare_pairs, miso_amd/csrc/kernels_compare_pairs.hip) against
its restatements (tests/_pairs_ref.py): every double by its bits, every count as an integer.  Columns are placed with
SamplesBatch (miso_batch_from_samples) at the smallest shapes at which each piece can go wrong: fewer draws than threads,
one more and one fewer than a power of two, unequal columns, a chunk of several draws per thread, and the limit."""
import math

import numpy as np
import pytest

import _pairs_ref as PR
import miso_amd
from miso_amd import capi, workload

pytestmark = pytest.mark.gpu

TAUS = (0.05, 0.2, 0.25, 0.5)


def _got(b, i, k):
    med, lo, hi, gt, lt, ge, fin, M = b.pair_comparison(i)
    return med[k], lo[k], hi[k], int(gt[k]), int(lt[k]), [int(v) for v in ge[k]], bool(fin[k]), M


def _check(b, i, s1, s2, level, taus, ref=PR.brute, label=""):
    for k in range(s1.shape[1]):
        want, got = ref(s1[:, k], s2[:, k], level, taus), _got(b, i, k)
        assert PR.same(got, want), (label, i, k, got, want)


SHAPES = [(2, 2, 0.5), (2, 2, 0.95), (3, 5, 0.95), (64, 64, 0.95), (255, 257, 0.9), (256, 256, 0.95), (1000, 450, 0.95),
          (4097, 300, 0.95)]


@pytest.mark.parametrize("S1,S2,level", SHAPES)
def test_chosen_columns_bit_for_bit(S1, S2, level):
    """one event per kind of column, two isoforms each (the second: the first kind's columns the other way round)"""
    cols = [PR.columns(kind, S1, S2) for kind in PR.KINDS]
    extra = PR.columns("uniform", S1, S2, seed=1)
    ev1 = [np.stack([a, extra[0]], 1) for a, _ in cols]
    ev2 = [np.stack([b, extra[1]], 1) for _, b in cols]
    b1, b2 = capi.SamplesBatch(ev1), capi.SamplesBatch(ev2)
    b1.compare_pairs(b2, level, TAUS)
    assert b1.last_kernels().split(",")[-1] == "compare_pairs"
    for i, kind in enumerate(PR.KINDS):
        _check(b1, i, ev1[i], ev2[i], level, TAUS, label=kind)
    assert b1.pair_comparison(0)[7] == S1 * S2
    # the samples swapped
    b2.compare_pairs(b1, level, TAUS)
    for i, kind in enumerate(PR.KINDS):
        _check(b2, i, ev2[i], ev1[i], level, TAUS, label=kind + " swapped")


def test_the_limit_against_count_and_bisect():
    S = 8192
    rng = np.random.default_rng(5)
    ev1 = [np.stack([rng.random(S), np.round(rng.beta(3, 5, S), 4)], 1)]
    ev2 = [np.stack([rng.random(S), np.round(rng.beta(4, 4, S), 4)], 1)]
    b1, b2 = capi.SamplesBatch(ev1), capi.SamplesBatch(ev2)
    b1.compare_pairs(b2, 0.95, TAUS)
    _check(b1, 0, ev1[0], ev2[0], 0.95, TAUS, ref=PR.bisect, label="8192 x 8192")
    assert b1.pair_comparison(0)[7] == S * S


def test_a_threshold_on_a_difference_and_the_rounding_artefact():
    """dyadic values: 0.75 - 0.5 is 0.25 itself and counts in |d| >= 0.25; 0.3 - 0.1 is the double below 0.2 and does not"""
    b1 = capi.SamplesBatch([np.array([[0.75, 0.3], [0.5, 0.3]])])
    b2 = capi.SamplesBatch([np.array([[0.5, 0.1], [0.75, 0.1], [1.0, 0.1]])])
    b1.compare_pairs(b2, 0.5, (0.25, 0.2, 0.19))
    ge = b1.pair_comparison(0)[5]
    # differences 0.25, 0, -0.25, 0, -0.25, -0.5;  six times 0.19999999999999998
    assert ge.tolist() == [[4, 4, 4], [0, 0, 6]]
    _check(b1, 0, np.array([[0.75, 0.3], [0.5, 0.3]]), np.array([[0.5, 0.1], [0.75, 0.1], [1.0, 0.1]]), 0.5, (0.25, 0.2, 0.19))


def test_mixed_isoform_counts_and_columns_that_are_not_finite():
    rng = np.random.default_rng(8)
    S1, S2, Ks = 300, 211, [2, 3, 5, 3, 2, 5]

    def sample(S):
        evs = []
        for K in Ks:
            x = rng.dirichlet(np.ones(K), S)
            evs.append(np.round(x, 4))
        return evs
    ev1, ev2 = sample(S1), sample(S2)
    ev1[1][17, 2] = np.nan              # event 1, isoform 2 of sample 1
    ev2[3][200, 0] = np.inf             # event 3, isoform 0 of sample 2
    ev1[5][0, 4] = -np.inf
    b1, b2 = capi.SamplesBatch(ev1), capi.SamplesBatch(ev2)
    b1.compare_pairs(b2, 0.9, (0.1, 0.2))
    fins = [b1.pair_comparison(i)[6].tolist() for i in range(len(Ks))]
    assert fins == [[True] * 2, [True, True, False], [True] * 5, [False, True, True], [True] * 2, [True] * 4 + [False]]
    for i in range(len(Ks)):
        _check(b1, i, ev1[i], ev2[i], 0.9, (0.1, 0.2))
    med, lo, hi, gt, lt, ge, fin, M = b1.pair_comparison(1)
    assert math.isnan(med[2]) and math.isnan(lo[2]) and math.isnan(hi[2]) and (gt[2], lt[2]) == (0, 0) and ge[2].tolist() == [0, 0]
    # the same events without the three values: every other column is what it was
    clean1, clean2 = [e.copy() for e in ev1], [e.copy() for e in ev2]
    clean1[1][17, 2] = clean2[3][200, 0] = clean1[5][0, 4] = 0.5
    c1, c2 = capi.SamplesBatch(clean1), capi.SamplesBatch(clean2)
    c1.compare_pairs(c2, 0.9, (0.1, 0.2))
    for i, K in enumerate(Ks):
        for k in range(K):
            if fins[i][k]:
                assert PR.same(_got(b1, i, k), _got(c1, i, k)), (i, k)


@pytest.mark.parametrize("taus", [(), (0.2,), (0.05, 0.2, 0.25, 0.5)])
def test_number_of_thresholds(taus):
    a, b = PR.columns("ties", 130, 77)
    a2, b2 = PR.columns("on_threshold", 130, 77)
    ev1, ev2 = [np.stack([a, a2], 1)], [np.stack([b, b2], 1)]
    x1, x2 = capi.SamplesBatch(ev1), capi.SamplesBatch(ev2)
    x1.compare_pairs(x2, 0.95, taus)
    assert x1.pair_comparison(0)[5].shape == (2, len(taus))
    _check(x1, 0, ev1[0], ev2[0], 0.95, taus)


def test_refusals_launch_nothing():
    rng = np.random.default_rng(2)
    ok1, ok2 = capi.SamplesBatch([rng.random((20, 2)), rng.random((20, 3))]), capi.SamplesBatch([rng.random((9, 2)), rng.random((9, 3))])

    def refused(x, y, level=0.95, taus=(0.2,), match="Invalid value"):
        with pytest.raises(capi.InternalError, match=match) as err:
            x.compare_pairs(y, level, taus)
        assert "compare_pairs" not in x.last_kernels()
        with pytest.raises(capi.InternalError, match="has not run"):
            x.pair_comparison(0)
        return str(err.value)

    big = capi.SamplesBatch([np.zeros((8193, 2)), np.zeros((8193, 3))])
    for x, y in ((big, ok2), (ok1, big)):
        assert PR.refusal(8193, 9, 0.95, (0.2,)) in refused(x, y)
    assert "differ in events" in refused(ok1, capi.SamplesBatch([rng.random((9, 2))]))
    assert "differ in isoforms" in refused(ok1, capi.SamplesBatch([rng.random((9, 2)), rng.random((9, 4))]))
    for tau in (0.0, 1.0, -0.2, 1.5, float("nan")):
        assert PR.refusal(20, 9, 0.95, (0.2, tau)) in refused(ok1, ok2, taus=(0.2, tau))
    assert PR.refusal(20, 9, 0.95, (0.1,) * 5) in refused(ok1, ok2, taus=(0.1,) * 5)
    for level in (0.0, 1.0, -0.5, 1.5, float("nan")):
        assert PR.refusal(20, 9, level, (0.2,)) in refused(ok1, ok2, level=level)
    # a batch that has not run
    b = capi.Batch(36, iters=40, burn=10, lag=1, chains=2)
    exons, isoforms, pos, cig = workload.event_reads(3, K=2, n_reads=50)
    b.add_event(capi.Gene(exons, isoforms), pos, cig)
    one = capi.SamplesBatch([rng.random((9, 2))])
    refused(b, one, match="not launched")
    with pytest.raises(capi.InternalError, match="not launched"):
        one.compare_pairs(b)
    # ... and after all that the call still works
    ok1.compare_pairs(ok2, 0.95, (0.2,))
    assert ok1.pair_comparison(1)[7] == 180


def test_the_other_results_keep_their_bits():
    rng = np.random.default_rng(4)
    ev1 = [np.round(rng.dirichlet(np.ones(K), 400), 4) for K in (2, 3, 5)]
    ev2 = [np.round(rng.dirichlet(np.ones(K), 400), 4) for K in (2, 3, 5)]
    b1, b2 = capi.SamplesBatch(ev1), capi.SamplesBatch(ev2)
    b1.summarize(0.95)
    b2.summarize(0.95)
    b1.compare(b2)
    before = [(b1.comparison(i), b1.summary(i), b2.summary(i)) for i in range(3)]
    b1.compare_pairs(b2)
    after = [(b1.comparison(i), b1.summary(i), b2.summary(i)) for i in range(3)]
    for x, y in zip(before, after):
        for p, q in zip(x, y):
            assert all(PR.bits(u).tolist() == PR.bits(v).tolist() for u, v in zip(p, q))
    assert b1.pair_comparison(2)[5].shape == (5, 2)       # the default thresholds
    _check(b1, 2, ev1[2], ev2[2], 0.95, (0.1, 0.2))
    assert b1.compare_pairs_ms() > 0


def test_as_text_is_the_comparison_of_the_printed_draws():
    """as_text=True: every draw as "%.4f" prints it and float() reads it back, ties of the decimal expansion included"""
    rng = np.random.default_rng(13)
    ev1 = [np.stack([rng.random(333), np.r_[0.00005, 0.00015, 0.12345, 0.99995, rng.random(329)]], 1)]
    ev2 = [np.stack([rng.random(150), np.r_[0.00025, 0.5, rng.random(148)]], 1)]
    b1, b2 = capi.SamplesBatch(ev1), capi.SamplesBatch(ev2)
    b1.compare_pairs(b2, 0.95, TAUS, as_text=True)
    printed = lambda x: np.array([[float("%.4f" % v) for v in row] for row in x])
    _check(b1, 0, printed(ev1[0]), printed(ev2[0]), 0.95, TAUS, label="as text")
    b1.compare_pairs(b2, 0.95, TAUS)
    _check(b1, 0, ev1[0], ev2[0], 0.95, TAUS, label="as computed")


@pytest.mark.parametrize("paired,K", [(False, 2), (True, 3)])
def test_sampler_batches(paired, K):
    """resident samples of two runs of the same events (other seeds, other lengths): 300 and 240 rows"""
    n = 24
    b1 = workload.build_batch(100, n, K=K, n_reads=60, iters=200, burn=50, lag=1, chains=2, paired=paired)
    b2 = workload.build_batch(100, n, K=K, n_reads=60, iters=170, burn=50, lag=1, chains=2, paired=paired)
    b1.run(device=0, seed=5, first_event_id=0)
    b2.run(device=0, seed=6, first_event_id=0)
    b1.compare_pairs(b2, 0.95, (0.1, 0.2))
    assert b1.last_kernels().split(",")[-1] == "compare_pairs"
    for i in range(n):
        s1, s2 = b1.result(i).samples, b2.result(i).samples
        assert s1.shape == (300, K) and s2.shape == (240, K)
        _check(b1, i, s1, s2, 0.95, (0.1, 0.2), label="paired" if paired else "single")


def test_launched_and_not_yet_synced():
    """as miso_batch_compare: a batch that was launched is taken, synced or not -- the pass runs in sample 1's stream, behind
    its sampler, and waits for sample 2's"""
    b1 = workload.build_batch(300, 6, K=2, n_reads=60, iters=150, burn=50, lag=1, chains=2)
    b2 = workload.build_batch(300, 6, K=2, n_reads=60, iters=130, burn=50, lag=1, chains=2)
    for s, b in enumerate((b1, b2)):
        b.upload(0)
        b.launch(seed=40 + s, first_event_id=0)
    b1.compare_pairs(b2, 0.9, (0.2,))
    for b in (b1, b2):
        b.sync()
        b.download()
    for i in range(6):
        _check(b1, i, b1.result(i).samples, b2.result(i).samples, 0.9, (0.2,), label="unsynced")


def test_text_batches():
    """columns decoded from `.miso` text; an event outside the fast grammar is not finite, in either sample"""
    rng = np.random.default_rng(9)
    S1, S2, Ks = 120, 75, [2, 4, 2, 3]

    def sample(S, spoil):
        evs = [np.round(rng.dirichlet(np.ones(K), S), 4) for K in Ks]
        bodies = []
        for e, x in enumerate(evs):
            rows = [",".join("%.4f" % v for v in r) + "\t-12.5\n" for r in x]
            if e == spoil:
                rows[3] = rows[3].replace("\t", "e0\t")       # an exponent
            bodies.append("".join(rows).encode())
        offs = np.concatenate([[0], np.cumsum([len(t) for t in bodies])]).astype(np.int64)
        return evs, capi.SamplesBatch.from_text(b"".join(bodies), offs, Ks, S)
    ev1, b1 = sample(S1, 1)
    ev2, b2 = sample(S2, 2)
    assert [int(s != 0) for s in b1.status] == [0, 1, 0, 0] and [int(s != 0) for s in b2.status] == [0, 0, 1, 0]
    b1.compare_pairs(b2, 0.95, (0.2,))
    for i in (0, 3):
        _check(b1, i, ev1[i], ev2[i], 0.95, (0.2,), label="text")
    for i in (1, 2):
        med, lo, hi, gt, lt, ge, fin, M = b1.pair_comparison(i)
        assert not fin.any() and np.isnan(med).all() and np.isnan(lo).all() and np.isnan(hi).all()
        assert not gt.any() and not lt.any() and not ge.any() and M == S1 * S2


def test_against_the_exact_mode():
    """exact=True batches of 2 000 rows: the all-pairs P(|delta| >= tau) against compare_exact's 1 - H(tau) + H(-tau),
    within five standard deviations by the U-statistic bound (tests/test_pairs_ref.py) plus 5e-6 for the tables"""
    S = 2000
    rng = np.random.default_rng(21)
    b = []
    plan = []
    for e in range(16):
        eff = (int(rng.integers(40, 400)), int(rng.integers(40, 400)))
        counts = []
        for _ in range(2):
            n, psi, both = int(rng.integers(20, 301)), rng.random(), rng.random() * 0.7
            cls = rng.choice(3, size=n, p=[(1 - both) * psi, (1 - both) * (1 - psi), both])
            counts.append(tuple(int((cls == c).sum()) for c in range(3)))
        plan.append((counts, eff))
    for which in (0, 1):
        x = miso_amd.Batch(36, exact=True, chains=2, iters=1000, burn=0, lag=1)
        for counts, eff in plan:
            n10, n01, n11 = counts[which]
            match = np.concatenate([np.tile([1.0, 0.0], (n10, 1)), np.tile([0.0, 1.0], (n01, 1)),
                                    np.tile([1.0, 1.0], (n11, 1))]).reshape(-1, 2)
            x.add_problem(match, [eff[0] + 35, eff[1] + 35], [1, 1])
        x.run(seed=31 + which, first_event_id=500)
        b.append(x)
    taus = (0.1, 0.2)
    b[0].compare_exact(b[1], [0.1, -0.1, 0.2, -0.2])
    b[0].compare_pairs(b[1], 0.95, taus)
    bound = 5 * math.sqrt((2 * S - 1) / (4.0 * S * S)) + 5e-6
    worst = 0.0
    for i in range(len(plan)):
        ex = b[0].exact_comparison(i)
        assert ex is not None
        H = ex[5]
        med, lo, hi, gt, lt, ge, fin, M = b[0].pair_comparison(i)
        assert M == S * S and fin.all()
        for j in range(2):
            want = 1 - H[2 * j] + H[2 * j + 1]
            got = ge[0, j] / M
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= bound, (i, taus[j], got, want, bound)
        _check(b[0], i, b[0].result(i).samples, b[1].result(i).samples, 0.95, taus, label="exact")
    print("worst |all pairs - exact| %.5f, bound %.5f" % (worst, bound))
