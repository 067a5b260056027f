"""The quantiles of delta psi from the exact CDF on the device, paired-end (csrc/kernels_exact_paired_delta.hip,
miso_batch_exact_delta_quantiles on paired-end batches).

Bit for bit against the restatement (tests/_exact_delta_ref.py, itself checked against mpmath in
tests/test_exact_delta_ref.py): caller-given elements (miso_selftest_exact_paired_delta_quantiles) on the case list of the
paired comparison and on the drawing-pair counts around the block of 16 and the chunk of 64, and whole batches.  Then the
quantiles against the mode's own draws.
"""
import numpy as np
import pytest

import miso_amd
from miso_amd import capi
from _exact_delta_ref import PROBS, paired_cdf, paired_delta_quantiles, search
from _exact_paired_ref import PairedStats, ass_sums, fragment_dist
from _exact_paired_compare_ref import HYPERS, PairedCompare, cases, paired_stats, stats6
from _problems import simulate_pe

pytestmark = pytest.mark.gpu

READ_LEN = 36
MEAN = 250.0
ISOLEN, NOEXONS = [1500, 1000], [3, 2]
AA = (60000.0, 43000.0)


@pytest.fixture(scope="module")
def post(orc):
    return PairedCompare(orc)


def _rnd(seed, n):
    return np.random.default_rng(seed).uniform(1e-5, 0.0133, size=(n, 2))


def _run(pairs, probs):
    return capi.selftest_exact_paired_delta_quantiles([stats6(a) for a, _ in pairs], [a.m for a, _ in pairs],
                                                      [stats6(b) for _, b in pairs], [b.m for _, b in pairs], probs)


def _check(post, pairs, probs=PROBS):
    """pairs: [(PairedStats of sample 1, of sample 2)] -> one launch, every element against the restatement; returns which
    elements had A = sample 2"""
    out = _run(pairs, probs)
    assert out.shape == (len(pairs), len(probs) + 1)
    a2 = []
    for j, (a, b) in enumerate(pairs):
        H = paired_cdf(post, a, b)
        want = search(H, probs)
        assert np.array_equal(out[j], want), (j, a.nd, b.nd, out[j], want)
        a2.append(H.a_is_2)
    return a2


@pytest.mark.parametrize("hyper", HYPERS, ids=["h11", "h25"])
def test_case_list_bit_exact(post, hyper):
    pairs = [(paired_stats(s1, hyper), paired_stats(s2, hyper)) for _, s1, s2 in cases()]
    a2 = _check(post, pairs)
    assert any(a2) and not all(a2)           # both outcomes of "A = sample 2"


@pytest.mark.parametrize("counts", [(0, 1, 15, 16), (17, 63, 64, 65)], ids=lambda c: "-".join(map(str, c)))
def test_block_and_chunk_edges_bit_exact(post, counts):
    """nd drawing pairs in sample 1 against nd + 1 in sample 2, and swapped: every count on either side"""
    pairs = []
    for nd in counts:
        a = PairedStats(5, 3, AA[0], AA[1], 1.0, 1.0, _rnd(100 + nd, nd))
        b = PairedStats(2, 6, 52000.0, 61000.0, 2.0, 5.0, _rnd(200 + nd, nd + 1))
        pairs += [(a, b), (b, a)]
    _check(post, pairs)


def test_a_tie_one_probability_and_errors(post):
    none1 = PairedStats(9, 4, AA[0], AA[1], 1.0, 1.0, [])
    many = PairedStats(2, 1, AA[0], AA[1], 1.0, 1.0, _rnd(31, 65))
    same = PairedStats(7, 6, AA[0], AA[1], 2.0, 5.0, _rnd(32, 20))
    pairs = [(none1, many), (many, none1), (same, same)]
    a2 = _check(post, pairs, [0.5])
    assert a2[2] is False                    # a tie goes to sample 1
    assert a2[0] != a2[1]
    good = PairedStats(1, 1, AA[0], AA[1], 1.0, 1.0, [(0.01, 0.002)])
    for bad_p in ([], [0.0], [1.0], [0.5, 1.5], [0.1] * 5):
        with pytest.raises(miso_amd.InternalError, match="Invalid value"):
            _run([(good, good)], bad_p)
    bad_h = [1.0, 1.0, AA[0], AA[1], 0.5, 1.0]
    with pytest.raises(miso_amd.InternalError, match="Invalid value"):
        capi.selftest_exact_paired_delta_quantiles([stats6(good)], [good.m], [bad_h], [good.m], [0.5])
    with pytest.raises(miso_amd.InternalError, match="Invalid value"):
        capi.selftest_exact_paired_delta_quantiles([stats6(good)], [[(0.01, 2.0 ** -64)]], [stats6(good)], [good.m], [0.5])


# ---- whole batches ----

class Problem:
    """a two-isoform paired-end problem for add_problem: n10 / n01 pairs compatible with one isoform, nd with both, their
    fragment lengths drawn inside the batch's fragment-length range"""

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


def _batches(orc, chains=2, iters=310, burn=10, lag=1, n_events=N_EVENTS):
    out = []
    for which, (var, seed) in enumerate(((900.0, 87), (1600.0, 88))):
        start, prob = fragment_dist(MEAN, var, 4.0, READ_LEN)
        rng = np.random.default_rng(60 + which)
        b = miso_amd.Batch(READ_LEN, paired=True, mean=MEAN, var=var, exact_paired=True, chains=chains, iters=iters, burn=burn, lag=lag)
        probs = []
        for i in range(n_events):
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


def test_batches_bit_exact(orc, post):
    (b1, p1, s1, f1), (b2, p2, s2, f2) = _batches(orc)
    with pytest.raises(miso_amd.InternalError, match="has not run"):
        b1.exact_delta_quantiles(b2)
    b1.compare_exact_paired(b2, [0.1, -0.1])
    before = [b1.exact_comparison(i) for i in range(N_EVENTS)]
    b1.exact_delta_quantiles(b2)
    assert b1.last_kernels().split(",")[-2:] == ["exact_paired_compare", "exact_paired_delta_quantiles"]
    assert b1.exact_delta_ms() > 0.0
    n_cmp = 0
    for i in range(N_EVENTS):
        got = b1.exact_delta(i)
        if i in THREE or i in ONLY_IN_1 or i in ONLY_IN_2:
            assert got is None and before[i] is None, i
            continue
        n_cmp += 1
        want = paired_delta_quantiles(post, p1[i].stats(s1, f1), p2[i].stats(s2, f2), PROBS)
        assert np.array_equal(np.concatenate([got[0], [got[1]]]), want), (i, got, want)
        after = b1.exact_comparison(i)
        assert after[:5] == before[i][:5] and np.array_equal(after[5], before[i][5]), i
    assert n_cmp == N_EVENTS - len(THREE) - len(ONLY_IN_1) - len(ONLY_IN_2)
    # a new comparison discards the quantiles
    b1.compare_exact_paired(b2)
    with pytest.raises(miso_amd.InternalError, match="has not run"):
        b1.exact_delta(0)


def test_quantiles_against_the_modes_own_draws(orc):
    """S = 5000 independent rows per sample: the fraction of index-paired differences <= q_k is a binomial proportion with
    success probability p_k, so |fraction - p_k| <= 5 sd + 1 / S; the same for the fraction <= 0 and H(0)"""
    S, n_events = 5000, 25
    (b1, _, _, _), (b2, _, _, _) = _batches(orc, chains=2, iters=2500, burn=0, lag=1, n_events=n_events)
    b1.compare_exact_paired(b2)
    b1.exact_delta_quantiles(b2, PROBS)
    worst, n = 0.0, 0
    for i in range(n_events):
        got = b1.exact_delta(i)
        if got is None:
            continue
        q, H0 = got
        x1, x2 = b1.result(i).samples[:, 0], b2.result(i).samples[:, 0]
        assert len(x1) == len(x2) == S
        d = x1 - x2
        n += 1
        for z, p in list(zip(q, PROBS)) + [(0.0, min(max(H0, 0.0), 1.0))]:
            frac = float((d <= z).mean())
            bound = 5 * np.sqrt(p * (1 - p) / S) + 1.0 / S
            worst = max(worst, abs(frac - p) / bound)
            print("event %d z %.6f p %.6f fraction %.6f bound %.6f" % (i, z, p, frac, bound))
            assert abs(frac - p) <= bound, (i, z, frac, p, bound)
    assert n == 20
    print("worst |fraction - p| / bound %.3f over %d events" % (worst, n))
