"""The exact-posterior mode on the device (csrc/kernels_exact.hip, miso_batch_set_exact).

Bit for bit against its restatement (tests/_exact_ref.py, itself checked against mpmath in tests/test_exact_ref.py):
the posterior stage alone (miso_selftest_exact) and whole batches -- samples, log scores, the reassignment, the exact
summaries --, events built straight from class counts with miso_batch_add_problem.  Then the mode's contract: the other
events of a batch are untouched, the draws follow the posterior's law, the mean agrees with the default sampler, and the
other front ends (files, diagnostics, stop = CONVERGENT_MEAN) work on an exact batch.
"""
import mpmath as mp
import numpy as np
import pytest

import miso_amd
from miso_amd import capi
from _exact_ref import CASES, HYPERS, Posterior, case_stats, eligible
from _problems import expr_for, flat, se_gene, simulate_se

pytestmark = pytest.mark.gpu

READ_LEN = 36
PROBS = [0.001, 0.025, 0.5, 0.975, 0.999]
# S = chains (iters - burn) / lag
SHAPES = {1: dict(chains=1, iters=1, burn=0, lag=1), 63: dict(chains=3, iters=21, burn=0, lag=1),
          65: dict(chains=5, iters=15, burn=2, lag=1), 3000: dict(chains=6, iters=1200, burn=200, lag=2)}
SMALL = [c for c in CASES if sum(c[:3]) <= 1000]


@pytest.fixture(scope="module")
def post(orc):
    return Posterior(orc)


_tabs = {}


def tab_of(post, case, hyper):
    key = (tuple(case), tuple(hyper))
    if key not in _tabs:
        _tabs[key] = post.tabulate(case_stats(case, hyper))
    return _tabs[key]


def add_case(b, case, hyper=None):
    """an event of n10 + n01 + n11 reads with these effective lengths (overhang 1: isoform length - read length + 1)"""
    n10, n01, n11, e0, e1 = case
    match = np.concatenate([np.tile([1.0, 0.0], (n10, 1)), np.tile([0.0, 1.0], (n01, 1)), np.tile([1.0, 1.0], (n11, 1))]).reshape(-1, 2)
    return b.add_problem(match, [e0 + READ_LEN - 1, e1 + READ_LEN - 1], [1, 1], hyper=hyper)


def check_exact_event(post, b, i, case, hyper, seed, event_id, S, assignment=True):
    tab = tab_of(post, case, hyper)
    r = b.result(i)
    samples, ll = post.draw(tab, seed, event_id, S)
    where = (case, hyper, S, event_id)
    assert np.array_equal(r.samples, samples), where
    assert np.array_equal(r.loglik, ll), where
    assert (r.rundata.noAccepted, r.rundata.noRejected, r.rundata.noSamples) == (S, 0, S), where
    n10, n01, n11 = case[:3]
    if assignment:
        want = np.concatenate([np.zeros(n10, np.int32), np.ones(n01, np.int32), post.assignment(samples[-1], seed, event_id, n11)])
        assert np.array_equal(r.assignment[:len(want)], want), where
    got = b.exact_summary(i, 0.95)
    assert got is not None, where
    for g, w in zip(got, post.summary(tab, 0.95)):
        assert np.array_equal(g, w), where


def test_posterior_stage_bit_exact(post):
    combos = [(c, h) for c in CASES for h in HYPERS[:2]]
    stats = [[c[0], c[1], sum(c[:3]), c[3], c[4], h[0], h[1]] for c, h in combos]
    out8, icdf = capi.selftest_exact(stats, PROBS)
    for j, (c, h) in enumerate(combos):
        tab = tab_of(post, c, h)
        want = [tab[k] for k in ("mean0", "mean1", "tL", "tR", "Z", "tm", "h", "gmax")]
        assert np.array_equal(out8[j], np.array(want, dtype=np.float64)), (c, h, out8[j], want)
        assert np.array_equal(icdf[j], post.icdf(tab, PROBS)), (c, h)


@pytest.mark.parametrize("S", sorted(SHAPES))
def test_batches_bit_exact_on_the_case_list(post, S):
    combos = [(c, h) for c in CASES for h in HYPERS[:2]]
    b = miso_amd.Batch(READ_LEN, exact=True, **SHAPES[S])
    for c, h in combos:
        add_case(b, c, h)
    b.run(seed=2024, first_event_id=700)
    assert b.last_kernels() == "exact_sample"
    ks = b.launch_stats()["kernels"]
    assert [k["name"] for k in ks] == ["exact_sample"] and ks[0]["chains"] == len(combos)
    for i, (c, h) in enumerate(combos):
        # (the reassignment of tens of thousands of reads is restated once, at S = 65)
        check_exact_event(post, b, i, c, h, 2024, 700 + i, S, assignment=(S == 65 or c[2] <= 1000))


@pytest.mark.parametrize("n_events", [1, 65, 300])
def test_batch_sizes_bit_exact(post, n_events):
    S = 63
    combos = [(SMALL[i % len(SMALL)], HYPERS[(i // len(SMALL)) % 2]) for i in range(n_events)]
    b = miso_amd.Batch(READ_LEN, exact=True, **SHAPES[S])
    for c, h in combos:
        add_case(b, c, h)
    b.run(seed=9, first_event_id=5)
    for i, (c, h) in enumerate(combos):
        check_exact_event(post, b, i, c, h, 9, 5 + i, S, assignment=i < 24)


def _mixed(exact, first_event_id=40, pin=None, order=None):
    """eligible events interleaved with a three-isoform event, an h = 0.5 event and an event without effective length"""
    kw = dict(chains=2, iters=60, burn=10, lag=1)
    b = miso_amd.Batch(READ_LEN, exact=exact, counts_trace=True, **kw)
    rng = np.random.default_rng(5)
    m3 = (rng.random((200, 3)) < 0.6).astype(np.float64)
    m3[m3.sum(1) == 0, 0] = 1.0
    events = [("exact", CASES[3], HYPERS[0]), ("k3", None, None), ("exact", CASES[2], HYPERS[1]), ("h", CASES[3], HYPERS[2]),
              ("exact", CASES[5], HYPERS[0]), ("eff", (11, 5, 17, 0, 140), HYPERS[0]), ("exact", CASES[1], HYPERS[0])]
    if order is not None:
        events = [events[j] for j in order]
    for kind, c, h in events:
        if kind == "k3":
            i = b.add_problem(m3, [300, 280, 250], [1, 1, 1])
        else:
            i = add_case(b, c, h)
        if pin is not None:
            b.set_event_id(i, pin[len(b) - 1])
    b.run(seed=31, first_event_id=first_event_id)
    return b, events, kw["chains"] * (kw["iters"] - kw["burn"])


def test_mixed_batch_leaves_the_other_events_alone(post):
    plain, events, S = _mixed(False)
    mixed, _, _ = _mixed(True)
    assert "exact_sample" in mixed.last_kernels().split(",") and "exact_sample" not in plain.last_kernels()
    for i, (kind, c, h) in enumerate(events):
        if kind == "exact":
            assert eligible(False, 2, c[3:], h)
            check_exact_event(post, mixed, i, c, h, 31, 40 + i, S)
            continue
        assert mixed.exact_summary(i) is None
        a, e = plain.result(i, trace=True), mixed.result(i, trace=True)
        assert np.array_equal(a.samples, e.samples, equal_nan=True) and np.array_equal(a.loglik, e.loglik, equal_nan=True), kind
        assert np.array_equal(a.assignment, e.assignment) and (a.counts_hash == e.counts_hash).all(), kind
        assert np.array_equal(a.counts_trace, e.counts_trace), kind
        assert (a.rundata.noAccepted, a.rundata.noRejected) == (e.rundata.noAccepted, e.rundata.noRejected), kind


def test_ineligible_hyperparameters_on_the_whole_case_list():
    """all ten cases under h = (0.5, 0.5), an unbounded density: the mode takes none of them and changes nothing"""
    kw = dict(chains=2, iters=80, burn=20, lag=1)
    runs = []
    for exact in (False, True):
        b = miso_amd.Batch(READ_LEN, exact=exact, counts_trace=True, **kw)
        for c in CASES:
            add_case(b, c, HYPERS[2])
        b.run(seed=12, first_event_id=300)
        runs.append(b)
    plain, mode = runs
    assert "exact_sample" not in mode.last_kernels() and mode.last_kernels() == plain.last_kernels()
    assert [k["name"] for k in mode.launch_stats()["kernels"]] == [k["name"] for k in plain.launch_stats()["kernels"]]
    for i, c in enumerate(CASES):
        assert not eligible(False, 2, c[3:], HYPERS[2]) and mode.exact_summary(i) is None, c
        a, e = plain.result(i, trace=True), mode.result(i, trace=True)
        assert np.array_equal(a.samples, e.samples, equal_nan=True) and np.array_equal(a.loglik, e.loglik, equal_nan=True), c
        assert np.array_equal(a.assignment, e.assignment) and (a.counts_hash == e.counts_hash).all(), c
        assert np.array_equal(a.counts_trace, e.counts_trace), c
        assert all(getattr(a.rundata, f) == getattr(e.rundata, f) for f, _ in capi.RunData._fields_), c


def test_convergent_mean_rounds_of_the_other_events(orc, post):
    """stop = CONVERGENT_MEAN on a batch that mixes exact events with sampler events that need further rounds: the
    sampler events go through the same rounds to the same bits as without the mode, the exact events stay as the first
    round left them"""
    kw = dict(iters=200, burn=50, lag=2, chains=3, stop=1, max_iters=3000)
    S = 3 * (200 - 50) // 2
    rng = np.random.default_rng(3)
    plan = []
    for e in range(9):
        if e % 3 == 1:
            plan.append(("exact", SMALL[e % len(SMALL)], HYPERS[(e // 3) % 2]))
            continue
        K = int(rng.integers(3, 7))
        exons, isoforms = se_gene(K)
        og = orc.gene(flat(exons), isoforms)
        orc.rng_seed(900 + e)
        rc, _, pos, cig = orc.simulate_reads(og, expr_for(K), int(rng.integers(20, 600)), 36)
        assert rc == 0
        plan.append(("sampler", (exons, isoforms, pos, cig), None))
    runs = []
    for exact in (False, True):
        b = miso_amd.Batch(READ_LEN, exact=exact, **kw)
        for kind, c, h in plan:
            if kind == "exact":
                add_case(b, c, h)
            else:
                b.add_event(miso_amd.Gene(c[0], c[1]), c[2], c[3])
        b.run(seed=5, first_event_id=1000)
        runs.append(b)
    plain, mode = runs
    assert plain.rounds() > 1 and mode.rounds() > 1 and "exact_sample" in mode.last_kernels().split(",")
    changed = 0
    for i, (kind, c, h) in enumerate(plan):
        if kind == "exact":
            check_exact_event(post, mode, i, c, h, 5, 1000 + i, S)
            continue
        a, e = plain.result(i), mode.result(i)
        assert np.array_equal(a.samples, e.samples) and np.array_equal(a.loglik, e.loglik) and np.array_equal(a.assignment, e.assignment)
        assert (a.rundata.noAccepted, a.rundata.noRejected) == (e.rundata.noAccepted, e.rundata.noRejected)
        changed += int(a.rundata.noAccepted + a.rundata.noRejected != 3 * 200)
    assert changed > 0          # some sampler event did run a further round


def test_exact_events_do_not_depend_on_neighbours_or_sharding(post):
    base, events, S = _mixed(True)
    # the same events in another order, in a batch that starts at another id, each pinned to the id it had
    order = [6, 3, 0, 5, 2, 1, 4]
    other, _, _ = _mixed(True, first_event_id=9000, pin=[40 + j for j in order], order=order)
    for pos, j in enumerate(order):
        a, e = base.result(j), other.result(pos)
        assert np.array_equal(a.samples, e.samples, equal_nan=True) and np.array_equal(a.loglik, e.loglik, equal_nan=True), events[j][0]
        assert np.array_equal(a.assignment, e.assignment), events[j][0]
    # ... and an eligible event alone in its batch
    b = miso_amd.Batch(READ_LEN, exact=True, chains=2, iters=60, burn=10, lag=1)
    add_case(b, CASES[5], HYPERS[0])
    b.run(seed=31, first_event_id=44)
    assert np.array_equal(b.result(0).samples, base.result(4).samples)


def _mp_cdf_at(case, hyper, tab, t_sorted):
    """the posterior's CDF at ascending logit-space points, mpmath at 30 digits: the density is integrated interval by
    interval -- a five-point Gauss-Legendre rule on the short ones (between neighbouring draws), mp.quad on the others"""
    mp.mp.dps = 30
    n10, n01, n11, e0, e1 = case
    a, b, n = mp.mpf(n10) + mp.mpf(hyper[0]), mp.mpf(n01) + mp.mpf(hyper[1]), mp.mpf(n10 + n01 + n11)
    e0, e1, gmax = mp.mpf(e0), mp.mpf(e1), mp.mpf(float(tab["gmax"]))

    def f(t):
        em = mp.exp(-t)
        x, y = 1 / (1 + em), em / (1 + em)
        return mp.exp(a * mp.log(x) + b * mp.log(y) - n * mp.log(x * e0 + y * e1) - gmax)
    tm, tL, tR = (mp.mpf(float(tab[k])) for k in ("tm", "tL", "tR"))
    # five-point Gauss-Legendre on [-1, 1]
    s1, s2 = mp.sqrt(5 - 2 * mp.sqrt(mp.mpf(10) / 7)) / 3, mp.sqrt(5 + 2 * mp.sqrt(mp.mpf(10) / 7)) / 3
    w1, w2 = (322 + 13 * mp.sqrt(70)) / 900, (322 - 13 * mp.sqrt(70)) / 900
    gl = [(mp.mpf(0), mp.mpf(128) / 225), (s1, w1), (-s1, w1), (s2, w2), (-s2, w2)]
    short = (tR - tL) / 256
    pts = sorted({tm - 300, tL, tm, tR, tm + 300} | {mp.mpf(float(t)) for t in t_sorted})
    cum, acc = {pts[0]: mp.mpf(0)}, mp.mpf(0)
    for lo, hi in zip(pts[:-1], pts[1:]):
        if hi - lo <= short:
            c, r = (lo + hi) / 2, (hi - lo) / 2
            acc += r * sum(w * f(c + r * x) for x, w in gl)
        else:
            acc += mp.quad(f, [lo, hi])
        cum[hi] = acc
    return np.array([float(cum[mp.mpf(float(t))] / acc) for t in t_sorted])


@pytest.mark.parametrize("case,hyper", [(CASES[3], HYPERS[0]), (CASES[6], HYPERS[0]), (CASES[4], HYPERS[1])],
                         ids=["statistics-event", "mass-at-1e-5", "h2_5"])
def test_law_of_the_draws(post, case, hyper):
    S = 3000
    b = miso_amd.Batch(READ_LEN, exact=True, **SHAPES[S])
    add_case(b, case, hyper)
    b.run(seed=77, first_event_id=3)
    x = b.result(0).samples
    tab = tab_of(post, case, hyper)
    # Kolmogorov-Smirnov distance of the draws to the posterior, in logit space (a monotone map of psi), level 1e-3
    t = np.sort(np.log(x[:, 0]) - np.log(x[:, 1]))
    F = _mp_cdf_at(case, hyper, tab, t)
    i = np.arange(1, S + 1)
    D = max(np.abs(F - i / S).max(), np.abs(F - (i - 1) / S).max())
    print("KS distance %.4f, bound %.4f" % (D, 1.95 / np.sqrt(S)))
    assert D < 1.95 / np.sqrt(S)
    # the draws' Chen-Shao order statistics bracket the exact quantiles: 4 sd of an order statistic, sqrt(p (1 - p) / S) / density
    b.summarize(0.95)
    _, lo, hi = b.summary(0)
    _, qlo, qhi = b.exact_summary(0, 0.95)
    for p, got, q in ((0.025, lo[0], qlo[0]), (0.975, hi[0], qhi[0])):
        tq = post.invert(tab, np.array([p]) * tab["Z"])
        g = post.point(tab["st"], tq)[0][0]
        dens = np.exp(g - tab["gmax"]) / (tab["Z"] * q * (1 - q))       # density of psi at the quantile
        bound = 4 * np.sqrt(p * (1 - p) / S) / dens
        print("p = %.3f: order statistic %.6g, exact quantile %.6g, bound %.3g" % (p, got, q, bound))
        assert abs(got - q) < bound, (p, got, q, bound)


def test_exact_mean_against_the_default_sampler(orc, post):
    """the event of test_statistics.py: the exact mean against the default mode's over 8 event ids, 4 se + 2e-3"""
    exons, isoforms, g, pos, cig = simulate_se(orc, 2, 1000, seed=42)
    gene = miso_amd.Gene(exons, isoforms)
    e = miso_amd.Batch(READ_LEN, exact=True, iters=4000, burn=1000, lag=1, chains=1)
    e.add_event(gene, pos, cig)
    e.run(seed=500, first_event_id=0)
    exact_mean = e.exact_summary(0)[0][0]
    assert abs(e.result(0).samples[:, 0].mean() - exact_mean) < 4 * e.result(0).samples[:, 0].std() / np.sqrt(3000)
    d = miso_amd.Batch(READ_LEN, iters=4000, burn=1000, lag=1, chains=1)
    for _ in range(8):
        d.add_event(gene, pos, cig)
    d.run(seed=500, first_event_id=0)
    means = np.array([d.result(i).samples[:, 0].mean() for i in range(8)])
    se = np.sqrt(means.var(ddof=1) / 8)
    print("exact %.6f, default sampler %.6f +- %.6f" % (exact_mean, means.mean(), se))
    assert abs(means.mean() - exact_mean) < 4 * se + 2e-3


def test_errors():
    with pytest.raises(miso_amd.InternalError, match="Invalid value"):
        miso_amd.Batch(READ_LEN, exact=True, paired=True, mean=250.0, var=900.0)
    with pytest.raises(miso_amd.InternalError, match="Invalid value"):
        miso_amd.Batch(READ_LEN, exact=True, algo=capi.MISO_ALGO_MARGINAL)


def test_other_front_ends_on_an_exact_batch(tmp_path):
    kw = dict(chains=6, iters=300, burn=100, lag=2)
    S = 600
    # stop = CONVERGENT_MEAN: an exact event is done after the first round
    b = miso_amd.Batch(READ_LEN, exact=True, stop=capi.MISO_STOP_CONVERGENT_MEAN, max_iters=100000, **kw)
    for c in (CASES[3], CASES[5], CASES[2]):
        add_case(b, c)
    b.run(seed=3, first_event_id=0)
    assert b.rounds() == 1 and b.last_kernels() == "exact_sample"
    # chain diagnostics: independent draws
    b.diagnose()
    for i in range(3):
        rhat, ess, mcse, _ = b.diagnostics(i)
        assert (np.abs(rhat - 1) < 0.02).all() and (ess > 0.5 * S).all(), (rhat, ess)   # (the estimators' own noise at 600 draws)
    # the file writer and the header fields
    paths = [str(tmp_path / ("ev%d.miso" % i)) for i in range(3)]
    fields = b.header_fields([0, 1, 2])
    assert all(f[1] == "100.00" for f in fields), fields
    b.write_miso_files([0, 1, 2], paths, ["#header %d\n" % i for i in range(3)])
    for i, p in enumerate(paths):
        lines = open(p).read().splitlines()
        assert lines[0] == "#header %d" % i and len(lines) == 2 + S
        first = [float(v) for v in lines[2].split("\t")[0].split(",")]
        assert lines[1] == "sampled_psi\tlog_score" and (np.abs(first - b.result(i).samples[0]) <= 5.0001e-5).all()
