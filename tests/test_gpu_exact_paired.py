"""The paired-end exact-posterior mode on the device (csrc/kernels_exact_paired.hip, miso_batch_set_exact_paired; DESIGN.md
section 17).

Bit for bit against its restatement (tests/_exact_paired_ref.py, itself checked against mpmath in
tests/test_exact_paired_ref.py): the posterior stage alone (miso_selftest_exact_paired) and whole batches -- samples, log
scores, the reassignment, the exact summaries.  Then the mode's contract: the other events of a batch are untouched, the
mean agrees with the default paired sampler, stop = CONVERGENT_MEAN and the header fields work on such a batch.
"""
import numpy as np
import pytest

import miso_amd
from miso_amd import capi
from _exact_paired_ref import (PairedPosterior, PairedStats, ass_sums, eligible, fragment_dist, simulated_case,
                               synthetic_cases)
from _problems import simulate_pe

pytestmark = pytest.mark.gpu

READ_LEN = 36
MEAN = 250.0
PROBS = [0.001, 0.025, 0.5, 0.975, 0.999]
HYPERS = [(1.0, 1.0), (2.0, 5.0)]
ISOLEN, NOEXONS = [1500, 1000], [3, 2]
KW = dict(chains=2, iters=310, burn=10, lag=1)      # S = 600 rows: one full sweep of 512 and a partial one
S = 600


@pytest.fixture(scope="module")
def post(orc):
    return PairedPosterior(orc)


@pytest.fixture(scope="module")
def sim400(orc):
    return simulated_case(orc, 400)


def test_posterior_stage_bit_exact(orc, post, sim400):
    cases = [c[1:] for c in synthetic_cases()]
    cases.append((sim400["n10"], sim400["n01"], sim400["A"][0], sim400["A"][1], sim400["pairs"]))
    for n in (60, 1000):
        c = simulated_case(orc, n)
        cases.append((c["n10"], c["n01"], c["A"][0], c["A"][1], c["pairs"]))
    combos = [(c, h) for c in cases for h in HYPERS]
    stats = [[c[0], c[1], c[2], c[3], h[0], h[1]] for c, h in combos]
    out8, icdf = capi.selftest_exact_paired(stats, [c[4] for c, _ in combos], PROBS)
    for j, (c, h) in enumerate(combos):
        tab = post.tabulate(PairedStats(c[0], c[1], c[2], c[3], h[0], h[1], c[4]))
        where = (c[:4], len(c[4]), h)
        assert np.array_equal(out8[j], post.out8(tab)), (where, out8[j], post.out8(tab))
        assert np.array_equal(icdf[j], post.icdf(tab, PROBS)), where


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
        self.kind, self.n10, self.n01, self.hyper = kind, n10, n01, hyper
        # the contract's draw order: the drawing pairs by their fragment-length rows, ties by read index
        draws = [i for i in range(N) if kind[i] == 2]
        self.order = sorted(draws, key=lambda i: (self.fraglen[i, 0], self.fraglen[i, 1], i))

    def stats(self, start, prob, hyper):
        pairs = [(prob[self.fraglen[i, 0] - start], prob[self.fraglen[i, 1] - start]) for i in self.order]
        A = ass_sums(ISOLEN, start, len(prob))
        return PairedStats(self.n10, self.n01, A[0], A[1], hyper[0], hyper[1], pairs)

    def add(self, b):
        return b.add_problem(self.match, ISOLEN, NOEXONS, fraglen=self.fraglen, hyper=self.hyper)


def check_exact_event(post, b, i, prob, tab, seed, event_id):
    r = b.result(i)
    samples, ll = post.draw(tab, seed, event_id, S)
    assert np.array_equal(r.samples, samples), i
    assert np.array_equal(r.loglik, ll), i
    assert ((r.samples > 0) & (r.samples < 1)).all()
    assert (np.abs(r.samples.sum(1) - 1.0) <= 2.0 ** -52).all()
    assert (r.rundata.noAccepted, r.rundata.noRejected, r.rundata.noSamples) == (S, 0, S), i
    want = np.where(prob.kind == 0, 0, 1).astype(np.int32)
    picks = post.assignment(tab, samples[-1], seed, event_id)
    for rank, read in enumerate(prob.order):
        want[read] = picks[rank]
    assert np.array_equal(r.assignment, want), i
    got = b.exact_summary(i, 0.95)
    assert got is not None, i
    for g, w in zip(got, post.summary(tab, 0.95)):
        assert np.array_equal(g, w), i


def _six(orc, exact_paired, var, stop=capi.MISO_STOP_FIXEDNO):
    """0, 1, 17 and 400 drawing pairs (add_problem), a three-isoform event and an event with a hyperparameter of 0.5
    (add_event)"""
    start, prob = fragment_dist(MEAN, var, 4.0, READ_LEN)
    rng = np.random.default_rng(23)
    probs = [Problem(rng, start, len(prob), 9, 4, 0), Problem(rng, start, len(prob), 3, 2, 1, hyper=(2.0, 5.0)),
             Problem(rng, start, len(prob), 5, 8, 17), Problem(rng, start, len(prob), 120, 80, 400)]
    b = miso_amd.Batch(READ_LEN, paired=True, mean=MEAN, var=var, exact_paired=exact_paired, counts_trace=True, stop=stop,
                       **KW)
    for q in probs:
        q.add(b)
    ex3, iso3, _, pos3, cig3 = simulate_pe(orc, 3, 150, mean=MEAN, var=var, seed=5)
    b.add_event(miso_amd.Gene(ex3, iso3), pos3, cig3)
    ex2, iso2, _, pos2, cig2 = simulate_pe(orc, 2, 200, mean=MEAN, var=var, seed=6)
    b.add_event(miso_amd.Gene(ex2, iso2), pos2, cig2, hyper=(0.5, 0.5))
    b.run(seed=77, first_event_id=900)
    return b, probs, (start, prob)


@pytest.mark.parametrize("var", [900.0, 1600.0], ids=["sd30-dense", "sd40-plain"])
def test_batch_of_six_bit_exact_and_the_others_untouched(orc, post, var):
    mode, probs, (start, prob) = _six(orc, True, var)
    plain, _, _ = _six(orc, False, var)
    assert "exact_paired_sample" in mode.last_kernels().split(",") and "exact_paired_sample" not in plain.last_kernels()
    ks = {k["name"]: k for k in mode.launch_stats()["kernels"]}
    assert ks["exact_paired_sample"]["chains"] == 4
    for i, q in enumerate(probs):
        hyper = q.hyper or (1.0, 1.0)
        ps = q.stats(start, prob, hyper)
        assert eligible(2, (ps.base.e0, ps.base.e1), hyper)
        check_exact_event(post, mode, i, q, post.tabulate(ps), 77, 900 + i)
    for i in (4, 5):       # three isoforms; a hyperparameter of 0.5
        assert mode.exact_summary(i) is None
        a, e = plain.result(i, trace=True), mode.result(i, trace=True)
        assert np.array_equal(a.samples, e.samples, equal_nan=True) and np.array_equal(a.loglik, e.loglik, equal_nan=True), i
        assert np.array_equal(a.assignment, e.assignment) and (a.counts_hash == e.counts_hash).all(), i
        assert np.array_equal(a.counts_trace, e.counts_trace), i
        assert (a.rundata.noAccepted, a.rundata.noRejected) == (e.rundata.noAccepted, e.rundata.noRejected), i


def test_event_from_alignments_and_mean_against_the_default_paired_sampler(orc, post, sim400):
    """the simulated 400-pair event through add_event: bit-equal to the restatement, and the mode's mean against the default
    paired sampler over 8 event ids, test_statistics.py's rule 4 se + 2e-3"""
    c = sim400
    gene = miso_amd.Gene(c["exons"], c["isoforms"])
    e = miso_amd.Batch(READ_LEN, paired=True, mean=MEAN, var=900.0, exact_paired=True, **KW)
    e.add_event(gene, c["pos"], c["cig"])
    e.run(seed=500, first_event_id=0)
    assert e.last_kernels() == "exact_paired_sample"
    start, prob = fragment_dist(MEAN, 900.0, 4.0, READ_LEN)
    both = [i for i in range(len(c["match"])) if c["match"][i, 0] > 0 and c["match"][i, 1] > 0]
    order = sorted(both, key=lambda i: (c["fraglen"][i, 0], c["fraglen"][i, 1], i))
    pairs = [(prob[c["fraglen"][i, 0] - start], prob[c["fraglen"][i, 1] - start]) for i in order]
    tab = post.tabulate(PairedStats(c["n10"], c["n01"], c["A"][0], c["A"][1], 1.0, 1.0, pairs))
    samples, ll = post.draw(tab, 500, 0, S)
    r = e.result(0)
    assert np.array_equal(r.samples, samples) and np.array_equal(r.loglik, ll)
    exact_mean = e.exact_summary(0)[0][0]
    assert exact_mean == tab["mean0"]
    d = miso_amd.Batch(READ_LEN, paired=True, mean=MEAN, var=900.0, iters=4000, burn=1000, lag=1, chains=1)
    for _ in range(8):
        d.add_event(gene, c["pos"], c["cig"])
    d.run(seed=500, first_event_id=0)
    means = np.array([d.result(i).samples[:, 0].mean() for i in range(8)])
    se = np.sqrt(means.var(ddof=1) / 8)
    print("exact %.6f, default paired sampler %.6f +- %.6f" % (exact_mean, means.mean(), se))
    assert abs(means.mean() - exact_mean) < 4 * se + 2e-3


def test_convergent_mean_and_header_fields(orc):
    b, probs, _ = _six(orc, True, 900.0, stop=capi.MISO_STOP_CONVERGENT_MEAN)
    assert "exact_paired_sample" in b.last_kernels().split(",")
    fields = b.header_fields([0, 1, 2, 3])
    assert all(f[1] == "100.00" for f in fields), fields
    # the eligible events alone: done after round one
    start, prob = fragment_dist(MEAN, 900.0, 4.0, READ_LEN)
    only = miso_amd.Batch(READ_LEN, paired=True, mean=MEAN, var=900.0, exact_paired=True, stop=capi.MISO_STOP_CONVERGENT_MEAN,
                          max_iters=100000, **KW)
    for q in probs:
        q.add(only)
    only.run(seed=3, first_event_id=0)
    assert only.rounds() == 1 and only.last_kernels() == "exact_paired_sample"
    assert all(f[1] == "100.00" for f in only.header_fields([0, 1, 2, 3]))


def test_errors():
    with pytest.raises(miso_amd.InternalError, match="Invalid value"):
        miso_amd.Batch(READ_LEN, exact_paired=True)
    with pytest.raises(miso_amd.InternalError, match="Invalid value"):
        miso_amd.Batch(READ_LEN, exact_paired=True, paired=True, mean=MEAN, var=900.0, algo=capi.MISO_ALGO_MARGINAL)
    # the single-end switch on a paired-end batch stays the error it is
    with pytest.raises(miso_amd.InternalError, match="Invalid value"):
        miso_amd.Batch(READ_LEN, exact=True, paired=True, mean=MEAN, var=900.0)
