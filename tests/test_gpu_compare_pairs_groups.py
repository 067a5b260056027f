"""GPU: delta psi between two pooled groups of replicates (miso_batch_compare_pairs_groups,
miso_amd/csrc/kernels_compare_pairs_groups.hip) against its restatement (tests/_group_pairs_ref.py:
tests/_pairs_ref.py on the concatenated columns): every double by its bits, every count as an integer.  Columns are placed
with SamplesBatch; the shapes are the smallest at which each piece can go wrong -- fewer pooled draws than threads, one
more and one fewer than a power of two a replicate, unequal groups --, MISO's defaults, 5 000 rows and the limit."""
import math

import numpy as np
import pytest

import _group_pairs_ref as GR
import _pairs_ref as PR
from miso_amd import capi, workload

pytestmark = pytest.mark.gpu

TAUS = (0.05, 0.2, 0.25, 0.5)


def _got(g, i, k):
    med, lo, hi, gt, lt, ge, fin, M = g.pair_comparison(i)
    return med[k], lo[k], hi[k], int(gt[k]), int(lt[k]), [int(v) for v in ge[k]], bool(fin[k]), M


def _batches(groups):
    """groups[r][e]: replicate r's array [S, K] of event e"""
    return [capi.SamplesBatch(evs) for evs in groups]


def _check(g, i, evs1, evs2, level, taus, ref=GR.brute, label=""):
    """event i of the result against the restatement on the replicates' arrays evs1[r], evs2[r] ([S, K] each)"""
    for k in range(evs1[0].shape[1]):
        want = ref([x[:, k] for x in evs1], [x[:, k] for x in evs2], level, taus)
        got = _got(g, i, k)
        assert PR.same(got, want), (label, i, k, got, want)


def _kinds(n1, n2, S):
    """one event per kind of column, two isoforms each (the second: uniform draws of other seeds); per replicate"""
    cols = [GR.group_columns(kind, n1, n2, S) for kind in PR.KINDS]
    extra = GR.group_columns("uniform", n1, n2, S, seed=100)
    r1 = [[np.stack([c[0][r], extra[0][r]], 1) for c in cols] for r in range(n1)]
    r2 = [[np.stack([c[1][r], extra[1][r]], 1) for c in cols] for r in range(n2)]
    return r1, r2


@pytest.mark.parametrize("n1,n2,S,level", [(1, 1, 2, 0.5), (1, 1, 2, 0.95), (2, 3, 3, 0.95), (3, 3, 64, 0.95), (2, 2, 255, 0.9),
                                           (3, 2, 257, 0.95), (4, 1, 256, 0.95)])
def test_every_kind_of_column_bit_for_bit(n1, n2, S, level):
    r1, r2 = _kinds(n1, n2, S)
    b1, b2 = _batches(r1), _batches(r2)
    g = capi.compare_pairs_groups(b1, b2, level, TAUS)
    assert g.n_pairs == n1 * S * n2 * S and g.kernel_ms > 0
    for i, kind in enumerate(PR.KINDS):
        _check(g, i, [r[i] for r in r1], [r[i] for r in r2], level, TAUS, label=kind)
    # the order of the replicates within a group does not matter
    h = capi.compare_pairs_groups(b1[::-1], b2[::-1], level, TAUS)
    assert h.out.tolist() == g.out.tolist()
    if (n1, n2) == (1, 1):                                # one against one: the pairwise pass, bit for bit
        b1[0].compare_pairs(b2[0], level, TAUS)
        for i in range(len(PR.KINDS)):
            for k in range(2):
                assert PR.same(_got(g, i, k), _got(b1[0], i, k)), (i, k)


@pytest.mark.parametrize("n1,n2,S", [(3, 3, 2700), (3, 3, 5000), (2, 2, 8192)])
def test_defaults_five_thousand_rows_and_the_limit(n1, n2, S):
    rng = np.random.default_rng(S)
    r1 = [[np.stack([rng.random(S), np.round(rng.beta(3, 5, S), 4)], 1)] for _ in range(n1)]
    r2 = [[np.stack([rng.random(S), np.round(rng.beta(4, 4, S), 4)], 1)] for _ in range(n2)]
    g = capi.compare_pairs_groups(_batches(r1), _batches(r2), 0.95, TAUS)
    _check(g, 0, [r[0] for r in r1], [r[0] for r in r2], 0.95, TAUS, ref=GR.bisect, label="%d+%d x %d" % (n1, n2, S))
    assert g.n_pairs == n1 * n2 * S * S
    if S == 8192:
        assert g.n_pairs == 268_435_456


def test_refusals_launch_nothing_and_name_the_group():
    rng = np.random.default_rng(2)

    def batch(n=2, K=2, S=20):
        return capi.SamplesBatch([rng.random((S, K)) for _ in range(n)])
    good1, good2 = [batch(), batch()], [batch(), batch(), batch()]
    good1[0].compare_pairs(good2[0], 0.9, (0.2,))
    before = [_got(good1[0], i, k) for i in range(2) for k in range(2)]

    def refused(g1, g2, level=0.95, taus=(0.2,), match="Invalid"):
        with pytest.raises(capi.InternalError, match=match) as err:
            capi.compare_pairs_groups(g1, g2, level, taus)
        return str(err.value)

    big = [capi.SamplesBatch([np.zeros((8192, 2))]) for _ in range(3)]
    assert GR.refusal(3, 2, 8192, 0.95, (0.2,)) in refused(big, big[:2], match=r"group 1: Too many samples")
    assert GR.refusal(2, 3, 8192, 0.95, (0.2,)) in refused(big[:2], big, match=r"group 2: Too many samples")
    refused([batch(), batch(S=21)], good2, match=r"group 1 batch 1: .*samples per event")
    refused(good1, [batch(), batch(S=19)], match=r"group 2 batch 1: .*samples per event")
    refused(good1, [batch(), batch(), batch(n=3)], match=r"group 2 batch 2: .*differ in events")
    refused([batch(), batch(K=3)], good2, match=r"group 1 batch 1: .*differ in isoforms")
    refused([], good2, match="at least one batch")
    assert GR.refusal(2, 3, 20, 0.95, (0.1,) * 5) in refused(good1, good2, taus=(0.1,) * 5)
    for tau in (1.0, 0.0, -0.2, float("nan")):
        assert GR.refusal(2, 3, 20, 0.95, (0.2, tau)) in refused(good1, good2, taus=(0.2, tau))
    for level in (0.0, 1.0, float("nan")):
        assert GR.refusal(2, 3, 20, level, (0.2,)) in refused(good1, good2, level=level)
    empty = capi.Batch(36, iters=50, burn=10, lag=1, chains=1)          # never filled
    refused(good1 + [empty], good2, match=r"group 1 batch 2: batch not launched")
    # ... nothing was touched, and the batches are still good for a call
    assert all(PR.same(x, y) for x, y in zip(before, [_got(good1[0], i, k) for i in range(2) for k in range(2)]))
    g = capi.compare_pairs_groups(good1, good2)
    assert g.n_pairs == 40 * 60 and g.pair_comparison(1)[5].shape == (2, 2)      # the default thresholds
    with pytest.raises(IndexError):
        g.pair_comparison(2)


def test_replicates_that_disagree_and_a_constant_group():
    """the pooled median is not the mean of the pairwise ones (tests/test_group_pairs_ref.py), on the device too"""
    d1, d2 = GR.disagreeing(200)
    S = 200
    c2 = [np.random.default_rng(r).random(S) for r in range(3)]
    # isoform 0: the replicates that disagree; isoform 1: a constant group of three against a spread sample
    r1 = [[np.stack([d1[r], np.full(S, 0.37)], 1)] for r in range(3)]
    r2 = [[np.stack([d2[0], c2[0]], 1)]]
    b1, b2 = _batches(r1), _batches(r2)
    g = capi.compare_pairs_groups(b1, b2, 0.95, (0.2,))
    _check(g, 0, [r[0] for r in r1], [r[0] for r in r2], 0.95, (0.2,))
    med = g.pair_comparison(0)[0][0]
    pairwise = []
    for b in b1:
        b.compare_pairs(b2[0], 0.95, (0.2,))
        pairwise.append(b.pair_comparison(0)[0][0])
    assert 0.54 < med < 0.59 and med - sum(pairwise) / 3 > 0.12
    # a spread group of three against the constant one, the other way round
    r3 = [[np.stack([c2[r], d1[r]], 1)] for r in range(3)]
    g = capi.compare_pairs_groups(_batches(r3), b1[:2], 0.95, (0.2,))
    _check(g, 0, [r[0] for r in r3], [r[0] for r in r1[:2]], 0.95, (0.2,))


def test_mixed_isoform_counts_and_columns_that_are_not_finite():
    rng = np.random.default_rng(8)
    S, Ks = 150, [2, 3, 5, 3, 2, 5]
    r1 = [[np.round(rng.dirichlet(np.ones(K), S), 4) for K in Ks] for _ in range(3)]
    r2 = [[np.round(rng.dirichlet(np.ones(K), S), 4) for K in Ks] for _ in range(2)]
    r1[1][1][17, 2] = np.nan            # event 1, isoform 2, replicate 1 of group 1
    r2[1][3][149, 0] = np.inf           # event 3, isoform 0, replicate 1 of group 2
    r1[2][5][0, 4] = -np.inf
    g = capi.compare_pairs_groups(_batches(r1), _batches(r2), 0.9, (0.1, 0.2))
    fins = [g.pair_comparison(i)[6].tolist() for i in range(len(Ks))]
    assert fins == [[True] * 2, [True, True, False], [True] * 5, [False, True, True], [True] * 2, [True] * 4 + [False]]
    for i in range(len(Ks)):
        _check(g, i, [r[i] for r in r1], [r[i] for r in r2], 0.9, (0.1, 0.2))
    med, lo, hi, gt, lt, ge, fin, M = g.pair_comparison(1)
    assert math.isnan(med[2]) and math.isnan(lo[2]) and math.isnan(hi[2]) and (gt[2], lt[2]) == (0, 0) and ge[2].tolist() == [0, 0]
    assert M == 450 * 300


def test_text_batches_with_an_event_one_replicate_did_not_decode():
    rng = np.random.default_rng(9)
    S, Ks = 75, [2, 4, 2, 3]

    def sample(spoil):
        evs = [np.round(rng.dirichlet(np.ones(K), S), 4) for K in Ks]
        bodies = []
        for e, x in enumerate(evs):
            rows = [",".join("%.4f" % v for v in r) + "\t-12.5\n" for r in x]
            if e == spoil:
                rows[3] = rows[3].replace("\t", "e0\t")       # an exponent: outside the fast grammar
            bodies.append("".join(rows).encode())
        offs = np.concatenate([[0], np.cumsum([len(t) for t in bodies])]).astype(np.int64)
        return evs, capi.SamplesBatch.from_text(b"".join(bodies), offs, Ks, S)
    g1 = [sample(None), sample(1), sample(None)]
    g2 = [sample(None), sample(None)]
    assert [int(s != 0) for s in g1[1][1].status] == [0, 1, 0, 0]
    g = capi.compare_pairs_groups([b for _, b in g1], [b for _, b in g2], 0.95, (0.2,))
    for i in (0, 2, 3):
        _check(g, i, [evs[i] for evs, _ in g1], [evs[i] for evs, _ in g2], 0.95, (0.2,), label="text")
    med, lo, hi, gt, lt, ge, fin, M = g.pair_comparison(1)
    assert not fin.any() and np.isnan(med).all() and np.isnan(lo).all() and np.isnan(hi).all()
    assert not gt.any() and not lt.any() and not ge.any() and M == 3 * S * 2 * S


@pytest.mark.parametrize("taus", [(), (0.2,), (0.05, 0.2, 0.25, 0.5)])
def test_number_of_thresholds(taus):
    t1, t2 = GR.group_columns("ties", 2, 3, 77)
    o1, o2 = GR.group_columns("on_threshold", 2, 3, 77)
    r1 = [[np.stack([t1[r], o1[r]], 1)] for r in range(2)]
    r2 = [[np.stack([t2[r], o2[r]], 1)] for r in range(3)]
    g = capi.compare_pairs_groups(_batches(r1), _batches(r2), 0.95, taus)
    assert g.pair_comparison(0)[5].shape == (2, len(taus))
    _check(g, 0, [r[0] for r in r1], [r[0] for r in r2], 0.95, taus)


@pytest.mark.parametrize("paired,K", [(False, 2), (True, 3)])
def test_as_text_on_sampler_batches(paired, K):
    """three seeds as replicates of either group, 200 rows each: as_text is the comparison of the draws as "%.4f" prints
    them; without it, of the draws themselves.  Launched and not yet synced: the pass waits for every batch."""
    n = 6
    groups = []
    for first_seed, iters in ((5, 150), (15, 150)):
        bs = []
        for r in range(3):
            b = workload.build_batch(100, n, K=K, n_reads=60, iters=iters, burn=50, lag=1, chains=2, paired=paired)
            b.upload(0)
            b.launch(seed=first_seed + r, first_event_id=0)
            bs.append(b)
        groups.append(bs)
    g_text = capi.compare_pairs_groups(groups[0], groups[1], 0.95, (0.1, 0.2), as_text=True)
    g_raw = capi.compare_pairs_groups(groups[0], groups[1], 0.95, (0.1, 0.2))
    for bs in groups:
        for b in bs:
            b.sync()
            b.download()
    printed = lambda x: np.array([[float("%.4f" % v) for v in row] for row in x])  # noqa: E731
    for i in range(n):
        s1, s2 = [b.result(i).samples for b in groups[0]], [b.result(i).samples for b in groups[1]]
        assert s1[0].shape == (200, K)
        _check(g_raw, i, s1, s2, 0.95, (0.1, 0.2), label="as computed")
        _check(g_text, i, [printed(x) for x in s1], [printed(x) for x in s2], 0.95, (0.1, 0.2), label="as text")


def test_pooled_counts_are_the_sums_of_the_pairwise_passes_and_nothing_else_moves():
    """device against device: n_gt0, n_lt0, n_abs_ge summed over Batch.compare_pairs of every (i, j); and the batches' own
    earlier compare_pairs, compare and summarize results keep their bits through the group calls"""
    rng = np.random.default_rng(4)
    Ks = (2, 3, 5)
    r1 = [[np.round(rng.dirichlet(np.ones(K), 300), 4) for K in Ks] for _ in range(3)]
    r2 = [[np.round(rng.dirichlet(np.ones(K), 300), 4) for K in Ks] for _ in range(2)]
    b1, b2 = _batches(r1), _batches(r2)
    for b in b1 + b2:
        b.summarize(0.95)
    sums = [[np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros((K, 2), np.int64)] for K in Ks]
    for x in b1[::-1]:
        for y in b2[::-1]:                                 # (ends with b1[0] against b2[0]: the results kept below)
            x.compare_pairs(y, 0.9, (0.1, 0.2))
            for e in range(len(Ks)):
                _, _, _, gt, lt, ge, fin, M = x.pair_comparison(e)
                assert fin.all() and M == 90000
                sums[e][0] += gt; sums[e][1] += lt; sums[e][2] += ge
    b1[0].compare(b2[0])

    def stored():
        return [(b1[0].comparison(i), b1[0].summary(i), b2[0].summary(i), b1[0].pair_comparison(i)[:6]) for i in range(len(Ks))]
    before = stored()
    g = capi.compare_pairs_groups(b1, b2, 0.9, (0.1, 0.2))
    for e in range(len(Ks)):
        _, _, _, gt, lt, ge, fin, M = g.pair_comparison(e)
        assert M == 900 * 600 and fin.all()
        assert gt.tolist() == sums[e][0].tolist() and lt.tolist() == sums[e][1].tolist() and ge.tolist() == sums[e][2].tolist()
    # a second call with other arguments
    g2 = capi.compare_pairs_groups(b2, b1, 0.5, (0.3,), as_text=True)
    assert g2.pair_comparison(2)[5].shape == (5, 1)
    for x, y in zip(before, stored()):
        for p, q in zip(x, y):
            assert all(PR.bits(u).tolist() == PR.bits(v).tolist() if np.asarray(u).dtype.kind == "f"
                       else np.asarray(u).tolist() == np.asarray(v).tolist() for u, v in zip(p, q))
    # ... and the first call's own results are still its own
    assert g.pair_comparison(0)[5].shape == (2, 2) and g.n_pairs == 900 * 600
    assert b1[0].pair_comparison(0)[7] == 90000
