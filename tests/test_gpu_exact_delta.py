"""The quantiles of delta psi from the exact CDF on the device, single-end (csrc/kernels_exact_delta.hip,
miso_batch_exact_delta_quantiles).

Bit for bit against the restatement (tests/_exact_delta_ref.py, itself checked against mpmath in
tests/test_exact_delta_ref.py): the kernel on caller-given statistics (miso_selftest_exact_delta_quantiles) on the pair list of
the exact comparison, and through two batches of events built straight from class counts.  Then the contract -- the errors, the
stored comparison untouched, a new comparison discards the quantiles -- and the one statistical test: the quantiles against the
exact mode's own independent draws.
"""
import numpy as np
import pytest

import miso_amd
from miso_amd import capi
from _exact_compare_ref import HYPERS, PAIRS, pair_rows
from _exact_delta_ref import PROBS, delta_quantiles
from _exact_ref import Posterior

pytestmark = pytest.mark.gpu

READ_LEN = 36
COMBOS = [(p, h) for h in HYPERS for p in PAIRS]
ZS = [0.1, -0.1]


@pytest.fixture(scope="module")
def post(orc):
    return Posterior(orc)


@pytest.fixture(scope="module")
def list_ref(post):
    """the restatement on the whole pair list at the three probabilities, computed once: [24, 4]"""
    return np.array([delta_quantiles(post, *pair_rows(p, h), probs=PROBS) for p, h in COMBOS])


@pytest.mark.parametrize("n_p", [1, 3])
def test_pair_list_bit_exact(list_ref, n_p):
    """(the quantile of a probability does not depend on the others given with it: the columns of the three-probability
    reference serve both calls)"""
    assert len(COMBOS) == 24
    rows = [pair_rows(p, h) for p, h in COMBOS]
    out = capi.selftest_exact_delta_quantiles([r[0] for r in rows], [r[1] for r in rows], PROBS[:n_p])
    assert out.shape == (len(COMBOS), n_p + 1)
    for j, (p, h) in enumerate(COMBOS):
        want = np.concatenate([list_ref[j, :n_p], list_ref[j, 3:]])
        assert np.array_equal(out[j], want), (p, h, out[j], want)


def test_selftest_errors():
    r1, r2 = pair_rows(PAIRS[1], HYPERS[0])
    assert capi.selftest_exact_delta_quantiles([r1], [r2], [0.5]).shape == (1, 2)
    for bad_p in ([0.0], [1.0], [0.5, 1.5], [], [0.1, 0.2, 0.3, 0.4, 0.5]):       # p of 0, 1 or 1.5; n_p of 0 and 5
        with pytest.raises(miso_amd.InternalError, match="Invalid value"):
            capi.selftest_exact_delta_quantiles([r1], [r2], bad_p)
    other = list(r2)
    other[4] = np.nextafter(r2[4], np.inf)          # e1 one ulp apart
    with pytest.raises(miso_amd.InternalError, match="effective lengths"):
        capi.selftest_exact_delta_quantiles([r1], [other], [0.5])
    low = list(r2)
    low[5] = 0.5                                    # a hyperparameter below 1: not the exact mode's
    with pytest.raises(miso_amd.InternalError, match="eligible"):
        capi.selftest_exact_delta_quantiles([r1], [low], [0.5])


def _add(b, counts, eff, hyper=None):
    """an event of n10 + n01 + n11 reads with these effective lengths (overhang 1: isoform length - read length + 1)"""
    n10, n01, n11 = counts
    match = np.concatenate([np.tile([1.0, 0.0], (n10, 1)), np.tile([0.0, 1.0], (n01, 1)), np.tile([1.0, 1.0], (n11, 1))]).reshape(-1, 2)
    return b.add_problem(match, [eff[0] + READ_LEN - 1, eff[1] + READ_LEN - 1], [1, 1], hyper=hyper)


def _plan(n_events=48, seed=21):
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


def _batches(plan, seeds=(101, 202), **shape):
    shape = shape or dict(chains=2, iters=60, burn=10, lag=1)
    out = []
    for which in (0, 1):
        b = miso_amd.Batch(READ_LEN, exact=True, **shape)
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


def _same(a, b):
    return a[:5] == b[:5] and np.array_equal(a[5], b[5])


def test_through_batches_bit_exact(post):
    plan = _plan()
    assert len(plan) == 48 and sum(ev[0] == "k3" for ev in plan) == 3
    b1, b2 = _batches(plan)
    with pytest.raises(miso_amd.InternalError, match="has not run"):
        b1.exact_delta_quantiles(b2)
    b1.compare_exact(b2, ZS)
    with pytest.raises(miso_amd.InternalError, match="has not run"):
        b1.exact_delta(0)
    before = [b1.exact_comparison(i) for i in range(len(plan))]
    b1.exact_delta_quantiles(b2)
    assert b1.last_kernels().split(",")[-2:] == ["exact_compare", "exact_delta_quantiles"]
    assert b1.exact_delta_ms() > 0.0
    n_none = 0
    for i, ev in enumerate(plan):
        got = b1.exact_delta(i)
        if ev[0] == "k3" or ev[3] != ev[4]:
            assert got is None and before[i] is None, i
            n_none += 1
            continue
        want = delta_quantiles(post, _row(ev[1], ev[3], ev[5]), _row(ev[2], ev[4], ev[5]), PROBS)
        assert np.array_equal(np.concatenate([got[0], [got[1]]]), want), (i, ev, got, want)
        assert got[0][1] <= got[0][0] <= got[0][2]
    assert n_none == 4
    # the stored comparison is what it was
    for i in range(len(plan)):
        after = b1.exact_comparison(i)
        assert (after is None and before[i] is None) or _same(after, before[i]), i
    # other probabilities replace the first; bad ones leave them
    b1.exact_delta_quantiles(b2, [0.25])
    one = b1.exact_delta(0)
    assert len(one[0]) == 1
    for bad_p in ([], [0.0], [0.5, 1.0], [0.1] * 5):
        with pytest.raises(miso_amd.InternalError, match="Invalid value"):
            b1.exact_delta_quantiles(b2, bad_p)
    again = b1.exact_delta(0)
    assert np.array_equal(again[0], one[0]) and again[1] == one[1]
    # a new comparison discards them
    b1.compare_exact(b2)
    with pytest.raises(miso_amd.InternalError, match="has not run"):
        b1.exact_delta(0)


def test_quantiles_against_the_modes_own_draws():
    """S = 5000 independent rows per sample: the fraction of index-paired differences <= q_k is a binomial proportion with
    success probability p_k, so |fraction - p_k| <= 5 sd + 1 / S; the same for the fraction <= 0 and H(0)"""
    S = 5000
    plan = [ev for ev in _plan(n_events=22, seed=22) if ev[0] == "k2" and ev[3] == ev[4]]
    assert len(plan) == 20
    b1, b2 = _batches(plan, chains=2, iters=2500, burn=0, lag=1)
    b1.compare_exact(b2)
    b1.exact_delta_quantiles(b2, PROBS)
    worst = 0.0
    for i, ev in enumerate(plan):
        q, H0 = b1.exact_delta(i)
        x1, x2 = b1.result(i).samples[:, 0], b2.result(i).samples[:, 0]
        assert len(x1) == len(x2) == S
        d = x1 - x2
        for z, p in list(zip(q, PROBS)) + [(0.0, min(max(H0, 0.0), 1.0))]:
            frac = float((d <= z).mean())
            bound = 5 * np.sqrt(p * (1 - p) / S) + 1.0 / S
            worst = max(worst, abs(frac - p) / bound)
            print("event %d z %.6f p %.6f fraction %.6f bound %.6f" % (i, z, p, frac, bound))
            assert abs(frac - p) <= bound, (i, ev, z, frac, p, bound)
    print("worst |fraction - p| / bound %.3f over %d events" % (worst, len(plan)))
