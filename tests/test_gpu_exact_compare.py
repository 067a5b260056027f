"""The exact comparison on the device (csrc/kernels_exact_compare.hip, miso_batch_compare_exact).

Bit for bit against its restatement (tests/_exact_compare_ref.py, itself checked against mpmath in
tests/test_exact_compare_ref.py): the kernel on caller-given statistics (miso_selftest_exact_compare) on the issue's pair
list, and through two batches of events built straight from class counts.  Then the one statistical test: the CDF of
psi_1 - psi_2 against the exact mode's own independent draws.
"""
import numpy as np
import pytest

import miso_amd
from miso_amd import capi
from _exact_compare_ref import HYPERS, PAIRS, ZS, compare, pair_rows
from _exact_ref import Posterior

pytestmark = pytest.mark.gpu

READ_LEN = 36
COMBOS = [(p, h) for h in HYPERS for p in PAIRS]


@pytest.fixture(scope="module")
def post(orc):
    return Posterior(orc)


@pytest.fixture(scope="module")
def list_ref(post):
    """the restatement on the whole pair list at all six z, computed once"""
    return np.array([compare(post, *pair_rows(p, h), zs=ZS) for p, h in COMBOS])


@pytest.mark.parametrize("n_z", [0, 1, 6])
def test_pair_list_bit_exact(list_ref, n_z):
    rows = [pair_rows(p, h) for p, h in COMBOS]
    out = capi.selftest_exact_compare([r[0] for r in rows], [r[1] for r in rows], ZS[:n_z])
    assert out.shape == (len(COMBOS), 5 + n_z)
    for j, (p, h) in enumerate(COMBOS):
        assert np.array_equal(out[j], list_ref[j, :5 + n_z]), (p, h, out[j], list_ref[j, :5 + n_z])


def test_selftest_errors():
    r1, r2 = pair_rows(PAIRS[1], HYPERS[0])
    other = list(r2)
    other[4] = np.nextafter(r2[4], np.inf)          # e1 one ulp apart
    with pytest.raises(miso_amd.InternalError, match="effective lengths"):
        capi.selftest_exact_compare([r1], [other], [0.1])
    assert capi.selftest_exact_compare([r1], [r2], [0.1]).shape == (1, 6)
    for bad_z in ([1.0], [-1.0], [0.1] * 9):
        with pytest.raises(miso_amd.InternalError, match="Invalid value"):
            capi.selftest_exact_compare([r1], [r2], bad_z)
    low = list(r2)
    low[5] = 0.5                                    # a hyperparameter below 1: not the exact mode's
    with pytest.raises(miso_amd.InternalError, match="eligible"):
        capi.selftest_exact_compare([r1], [low], [])


def _add(b, counts, eff, hyper=None):
    """an event of n10 + n01 + n11 reads with these effective lengths (overhang 1: isoform length - read length + 1)"""
    n10, n01, n11 = counts
    match = np.concatenate([np.tile([1.0, 0.0], (n10, 1)), np.tile([0.0, 1.0], (n01, 1)), np.tile([1.0, 1.0], (n11, 1))]).reshape(-1, 2)
    return b.add_problem(match, [eff[0] + READ_LEN - 1, eff[1] + READ_LEN - 1], [1, 1], hyper=hyper)


def _plan(n_events=48, seed=11):
    """per event: ("k2", counts of sample 1, of sample 2, eff of sample 1, of sample 2, hyper) or ("k3", match1, match2):
    20 - 300 reads, another psi in each sample; three three-isoform events and one event whose effective lengths differ
    between the samples among them"""
    rng = np.random.default_rng(seed)
    plan = []
    for e in range(n_events):
        if e in (5, 20, 41):
            ms = []
            for _ in range(2):
                m = (rng.random((int(rng.integers(20, 301)), 3)) < 0.6).astype(np.float64)
                m[m.sum(1) == 0, 0] = 1.0
                ms.append(m)
            plan.append(("k3", ms[0], ms[1]))
            continue
        eff = (int(rng.integers(40, 400)), int(rng.integers(40, 400)))
        counts = []
        for _ in range(2):
            n, psi, both = int(rng.integers(20, 301)), rng.random(), rng.random() * 0.7
            cls = rng.choice(3, size=n, p=[(1 - both) * psi, (1 - both) * (1 - psi), both])
            counts.append(tuple(int((cls == c).sum()) for c in range(3)))
        eff2 = (eff[0], eff[1] + 1) if e == 30 else eff
        plan.append(("k2", counts[0], counts[1], eff, eff2, HYPERS[e % 2]))
    return plan


def _batches(plan, exact=(True, True), seeds=(101, 202), **shape):
    shape = shape or dict(chains=2, iters=60, burn=10, lag=1)
    out = []
    for which in (0, 1):
        b = miso_amd.Batch(READ_LEN, exact=exact[which], **shape)
        for ev in plan:
            if ev[0] == "k3":
                b.add_problem(ev[1 + which], [300, 280, 250], [1, 1, 1])
            else:
                _add(b, ev[1 + which], ev[3 + which], ev[5])
        b.run(seed=seeds[which], first_event_id=1000)
        out.append(b)
    return out


def _row(counts, eff, hyper):
    return [float(counts[0]), float(counts[1]), float(sum(counts)), float(eff[0]), float(eff[1]), float(hyper[0]), float(hyper[1])]


def test_through_batches_bit_exact(post):
    plan = _plan()
    assert len(plan) == 48 and sum(ev[0] == "k3" for ev in plan) == 3
    b1, b2 = _batches(plan)
    b1.compare(b2)
    before = [b1.comparison(i) for i in range(len(plan))]
    with pytest.raises(miso_amd.InternalError, match="has not run"):
        b1.exact_comparison(0)
    b1.compare_exact(b2, ZS)
    assert b1.last_kernels().split(",")[-1] == "exact_compare"
    first = b1.exact_comparison(0)
    for i, ev in enumerate(plan):
        got = b1.exact_comparison(i)
        if ev[0] == "k3" or ev[3] != ev[4]:
            assert got is None, i
            continue
        want = compare(post, _row(ev[1], ev[3], ev[5]), _row(ev[2], ev[4], ev[5]), ZS)
        assert np.array_equal(np.concatenate([got[:5], got[5]]), want), (i, ev, got, want)
        # the means are the exact summaries' own
        assert got[0] == b1.exact_summary(i)[0][0] and got[1] == b2.exact_summary(i)[0][0]
    # the sampled comparison is untouched, and can be made again
    after = [b1.comparison(i) for i in range(len(plan))]
    b1.compare(b2)
    again = [b1.comparison(i) for i in range(len(plan))]
    for x, y, z in zip(before, after, again):
        assert all(np.array_equal(p, q) and np.array_equal(p, r) for p, q, r in zip(x, y, z))
    # another set of points replaces the first; none at all is allowed
    b1.compare_exact(b2, [0.3])
    assert len(b1.exact_comparison(0)[5]) == 1
    b1.compare_exact(b2)
    assert len(b1.exact_comparison(0)[5]) == 0 and b1.exact_comparison(0)[:5] == first[:5]


def test_batch_errors():
    plan = _plan(n_events=6)
    for exact in ((False, True), (True, False), (False, False)):
        b1, b2 = _batches(plan, exact=exact)
        with pytest.raises(miso_amd.InternalError, match="Invalid value"):
            b1.compare_exact(b2, [0.1])
    b1, b2 = _batches(plan)
    for bad_z in ([1.0], [0.0, -1.5], [0.1] * 9):
        with pytest.raises(miso_amd.InternalError, match="Invalid value"):
            b1.compare_exact(b2, bad_z)
    b3, _ = _batches(plan[:5])
    with pytest.raises(miso_amd.InternalError, match="Invalid value"):
        b1.compare_exact(b3, [0.1])


def test_cdf_against_the_modes_own_draws():
    """S = 5000 independent rows per sample: the fraction of index-paired differences <= z is a binomial proportion with
    success probability H(z), so |fraction - H| <= 5 sd + 1 / S (5 sd: 6e-7 per comparison, ~100 comparisons)"""
    S = 5000
    plan = [ev for ev in _plan(n_events=20, seed=12) if ev[0] == "k2" and ev[3] == ev[4]]
    plan += [("k2", p[0], p[1], p[2], p[2], h) for p in PAIRS if sum(p[0]) + sum(p[1]) <= 2000 for h in HYPERS]
    b1, b2 = _batches(plan, chains=2, iters=2500, burn=0, lag=1)
    b1.compare_exact(b2, ZS)
    worst = 0.0
    for i, ev in enumerate(plan):
        H = b1.exact_comparison(i)[5]
        x1, x2 = b1.result(i).samples[:, 0], b2.result(i).samples[:, 0]
        assert len(x1) == len(x2) == S
        d = x1 - x2
        for z, h in zip(ZS, np.clip(H, 0.0, 1.0)):
            frac = float((d <= z).mean())
            bound = 5 * np.sqrt(h * (1 - h) / S) + 1.0 / S
            worst = max(worst, abs(frac - h) / bound)
            assert abs(frac - h) <= bound, (i, ev, z, frac, h, bound)
    print("worst |fraction - H| / bound %.3f over %d events x %d points" % (worst, len(plan), len(ZS)))
