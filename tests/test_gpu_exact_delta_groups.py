"""The quantiles of delta psi between two groups of replicates from the exact posteriors, on the device
(csrc/kernels_exact_delta_groups.hip: miso_exact_delta_groups, miso_batch_get_exact_stats, miso_batch_exact_delta_groups;
DESIGN.md section 20a).

Bit for bit against the restatement (tests/_exact_delta_groups_ref.py, itself checked against mpmath in
tests/test_exact_delta_groups_ref.py) at (n1, n2) = (1, 1), (2, 1), (1, 2), (3, 3), (8, 8) and on the issue's three cases at
their own shapes, each call over five comparable events with two events a launch (three launches, the last ragged); bit for
bit against the pairwise kernels on the same statistics; the errors; the batches' route; and the one statistical test, against
the exact mode's own draws pooled over all pairs of replicates.  The restatement's pairwise tables are made once per pair of
rows and shared by every test of the module.
"""
import numpy as np
import pytest

import miso_amd
from miso_amd import capi
from _exact_compare_ref import HYPERS, PAIRS, pair_rows
from _exact_delta_groups_ref import EFF, MixtureCdf, case_rows, group_delta, rows_of
from _exact_ref import Posterior

pytestmark = pytest.mark.gpu

READ_LEN = 36
P4 = (0.5, 0.025, 0.975, 0.25)
Z8 = (0.1, -0.1, 0.2, -0.2, 0.0, 0.5, -0.9, 0.999)
_pairs = {}         # the restatement's pairwise CDFs by their two rows


@pytest.fixture(scope="module")
def post(orc):
    return Posterior(orc)


def _r(counts, hyper=HYPERS[0], eff=EFF):
    return rows_of([counts], hyper, eff)[0]


def _call(events, probs, zs, per_launch=2):
    s1 = np.array([e[0] for e in events], dtype=np.float64)
    s2 = np.array([e[1] for e in events], dtype=np.float64)
    return capi.exact_delta_groups(s1, s2, probs, zs, max_events_per_launch=per_launch)


def _check(post, events, probs, zs, per_launch=2):
    """one call over `events` = [(rows of group 1, rows of group 2)]: every row against the restatement, bit for bit; a
    non-comparable event keeps its row"""
    res = _call(events, probs, zs, per_launch)
    assert res.out.shape == (len(events), 2 + len(probs) + 1 + len(zs)) and res.kernel_ms >= 0.0
    n_ok = 0
    for i, (g1, g2) in enumerate(events):
        want = group_delta(post, g1, g2, probs, zs, _pairs)
        if want is None:
            assert res.was_exact[i] == 0 and res.row(i) is None and np.isnan(res.out[i]).all(), i
            continue
        n_ok += 1
        assert res.was_exact[i] == 1, i
        assert np.array_equal(res.out[i], want), (i, res.out[i], want, res.out[i] - want)
    return res, n_ok


A, B, C3 = (11, 5, 17), (3, 9, 20), (40, 10, 25)
X, Y = (5, 11, 17), (20, 3, 9)
MID, WIDE, NARROW = (30, 30, 30), (3, 3, 3), (3000, 3000, 3000)


def test_pairs_of_one_replicate_equal_the_pairwise_kernels():
    """(1, 1) on the exact comparison's own pair list: q and H0 are exact_delta_quantiles', H(z) is exact_compare's cdf, the
    means are its means -- device against device, bit for bit"""
    combos = [(p, h) for h in HYPERS for p in PAIRS]
    rows = [pair_rows(p, h) for p, h in combos]
    res = _call([([r[0]], [r[1]]) for r in rows], P4[:3], Z8, per_launch=5)
    dq = capi.selftest_exact_delta_quantiles([r[0] for r in rows], [r[1] for r in rows], P4[:3])
    cmp_ = capi.selftest_exact_compare([r[0] for r in rows], [r[1] for r in rows], Z8)
    assert res.was_exact.all()
    assert np.array_equal(res.out[:, 2:6], dq)
    assert np.array_equal(res.out[:, 6:], cmp_[:, 5:])
    assert np.array_equal(res.out[:, :2], cmp_[:, :2])


@pytest.mark.parametrize("n1,n2,n_p,n_z", [(1, 1, 3, 1), (2, 1, 4, 0), (1, 2, 1, 8)])
def test_small_groups_bit_exact(post, n1, n2, n_p, n_z):
    g1 = [_r(A), _r(B), _r(C3), _r(A, HYPERS[1]), _r(MID)]
    g2 = [_r(X), _r(Y), _r(X), _r(Y, HYPERS[1]), _r(WIDE)]
    events = [([g1[(i + a) % 3 if i < 3 else i] for a in range(n1)], [g2[(i + 2 * b) % 3 if i < 3 else i] for b in range(n2)])
              for i in range(5)]
    _, n_ok = _check(post, events, P4[:n_p], Z8[:n_z])
    assert n_ok == 5


def test_three_by_three_bit_exact_and_mean_of_pairwise_cdfs(post):
    """five comparable events -- the 3 x 3 case, one whose pairs take both outcomes of "A is the group-2 replicate", the tie
    (identical replicates), one under HYPERS[1], one mixed -- and two that are not: a hyperparameter below 1 in one replicate,
    e0 one ulp apart in one replicate"""
    both = ([_r(MID), _r(A), _r(MID)], [_r(WIDE), _r(NARROW), _r(X)])
    tie = ([_r(A)] * 3, [_r(A)] * 3)
    h1 = ([_r(A, HYPERS[1]), _r(B, HYPERS[1]), _r(A, HYPERS[1])], [_r(X, HYPERS[1]), _r(X, HYPERS[1]), _r(Y, HYPERS[1])])
    mixed = ([_r(A), _r(B), _r(C3)], [_r(X), _r(Y), _r(X)])
    low = ([_r(A), _r(B, (0.5, 1.0)), _r(C3)], [_r(X), _r(Y), _r(X)])
    ulp = ([_r(A), _r(B), _r(C3)], [_r(X), _r(Y, eff=(np.nextafter(float(EFF[0]), np.inf), EFF[1])), _r(X)])
    events = [case_rows("3x3agreeing", HYPERS[0]), low, both, tie, ulp, h1, mixed]
    zs = Z8[:1]
    res, n_ok = _check(post, events, P4[:3], zs)
    assert n_ok == 5 and list(res.was_exact) == [1, 0, 1, 1, 0, 1, 1]
    outcomes = {H.a_is_2 for H in MixtureCdf(post, both[0], both[1], _pairs).pairs}
    assert outcomes == {True, False}
    assert not any(H.a_is_2 for H in MixtureCdf(post, tie[0], tie[1], _pairs).pairs)
    # H(z) and H(0) are the a-major mean of the pairwise kernel's cdfs at the same z
    for i in (0, 2, 3, 5, 6):
        g1, g2 = events[i]
        pairs = [(a, b) for a in g1 for b in g2]
        cdf = capi.selftest_exact_compare([p[0] for p in pairs], [p[1] for p in pairs], [0.0] + list(zs))[:, 5:]
        for col, got in ((0, res.out[i, 5]), (1, res.out[i, 6])):
            s = np.float64(0.0)
            for v in cdf[:, col]:
                s = s + v
            assert got == s / np.float64(9), (i, col)


@pytest.mark.parametrize("name,n_p,n_z", [("disagreeing", 4, 8), ("sharp+wide", 1, 0)])
def test_issue_cases_bit_exact(post, name, n_p, n_z):
    """the case under both hyperparameter pairs and with its replicates permuted: five comparable events"""
    g1, g2 = case_rows(name, HYPERS[0])
    h1, h2 = case_rows(name, HYPERS[1])
    events = [(g1, g2), (h1, h2), (g1[::-1], g2), (g1[1:] + g1[:1], g2[::-1]), (h1[::-1], h2[::-1])]
    res, n_ok = _check(post, events, P4[:n_p], Z8[:n_z])
    assert n_ok == 5
    # a permutation inside a group moves H by a reordered sum's rounding at most
    hcols = res.out[:, 2 + n_p:]
    assert np.abs(hcols[2] - hcols[0]).max() <= 1e-12 and np.abs(hcols[3] - hcols[0]).max() <= 1e-12
    assert np.abs(hcols[4] - hcols[1]).max() <= 1e-12


def test_eight_by_eight_bit_exact(post):
    """64 pairs an event, the limit: replicates repeat, so that the restatement tabulates few pairs, but every one of the 64
    terms is added on the device"""
    def ev(a, b, c, hyper=HYPERS[0]):
        return [_r(a, hyper)] * 4 + [_r(b, hyper)] * 4, [_r(c, hyper)] * 8
    events = [ev(A, B, X), ev(B, C3, Y), ev(MID, A, WIDE), ev(A, B, X, HYPERS[1]), ev(C3, C3, C3)]
    _, n_ok = _check(post, events, P4[:1], Z8[:1])
    assert n_ok == 5


def test_launch_ranges_do_not_change_the_bits():
    g1 = [_r(A), _r(B)]
    events = [(g1, [_r(X)]), (g1[::-1], [_r(Y)]), (g1, [_r(Y)]), ([_r(C3), _r(A)], [_r(X)]), (g1, [_r(WIDE)])]
    one = _call(events, P4[:3], Z8[:2], per_launch=0)
    for per in (1, 2, 5, 7):
        assert np.array_equal(_call(events, P4[:3], Z8[:2], per_launch=per).out, one.out), per
    none = capi.exact_delta_groups(np.zeros((0, 2, 7)), np.zeros((0, 1, 7)), P4[:3], ())   # no event: no work, no error
    assert none.out.shape == (0, 6) and none.kernel_ms == 0.0


def test_errors_before_any_launch():
    ok1, ok2 = [[_r(A)]], [[_r(X)]]
    assert _call([(ok1[0], ok2[0])], [0.5], ()).was_exact[0] == 1
    bad = [
        (np.zeros((1, 0, 7)), ok2, [0.5], ()),                  # n1 = 0
        (np.tile(_r(A), (1, 9, 1)), ok2, [0.5], ()),            # n1 = 9
        (ok1, np.tile(_r(X), (1, 9, 1)), [0.5], ()),            # n2 = 9
        (ok1, ok2, [0.1, 0.2, 0.3, 0.4, 0.5], ()),              # n_p = 5
        (ok1, ok2, [], ()),                                     # n_p = 0
        (ok1, ok2, [1.0], ()),                                  # p = 1
        (ok1, ok2, [0.5], [1.0]),                               # z = 1
        (ok1, ok2, [0.5], [0.0] * 9),                           # n_z = 9
    ]
    for s1, s2, p, z in bad:
        with pytest.raises(miso_amd.InternalError, match="Invalid value"):
            capi.exact_delta_groups(s1, s2, p, z)
    with pytest.raises(ValueError):
        capi.exact_delta_groups(np.zeros((2, 1, 7)), np.zeros((1, 1, 7)))


# ---- through batches ----
N_EVENTS = 12
K3, UNEQUAL = 4, 9          # a three-isoform event; an event whose e1 differs in one replicate


def _plan(seed=31):
    """per event its effective lengths, hyperparameters and, per replicate (3 + 2), the class counts: another read set in
    every replicate, psi around one value per group"""
    rng = np.random.default_rng(seed)
    plan = []
    for e in range(N_EVENTS):
        eff = (int(rng.integers(40, 400)), int(rng.integers(40, 400)))
        psis = (rng.random(), rng.random())
        counts = []
        for rep in range(5):
            n, both = int(rng.integers(20, 301)), rng.random() * 0.7
            psi = min(max(psis[0 if rep < 3 else 1] + rng.normal(0, 0.05), 0.02), 0.98)
            cls = rng.choice(3, size=n, p=[(1 - both) * psi, (1 - both) * (1 - psi), both])
            counts.append(tuple(int((cls == c).sum()) for c in range(3)))
        plan.append((eff, HYPERS[e % 2], counts))
    return plan


def _batches(plan, **shape):
    shape = shape or dict(chains=2, iters=60, burn=10, lag=1)
    rng = np.random.default_rng(5)
    out = []
    for rep in range(5):
        b = miso_amd.Batch(READ_LEN, exact=True, **shape)
        for e, (eff, hyper, counts) in enumerate(plan):
            if e == K3:
                m = (rng.random((50, 3)) < 0.6).astype(np.float64)
                m[m.sum(1) == 0, 0] = 1.0
                b.add_problem(m, [300, 280, 250], [1, 1, 1])
                continue
            n10, n01, n11 = counts[rep]
            match = np.concatenate([np.tile([1.0, 0.0], (n10, 1)), np.tile([0.0, 1.0], (n01, 1)), np.tile([1.0, 1.0], (n11, 1))]).reshape(-1, 2)
            e1 = eff[1] + (1 if e == UNEQUAL and rep == 3 else 0)
            b.add_problem(match, [eff[0] + READ_LEN - 1, e1 + READ_LEN - 1], [1, 1], hyper=hyper)
        b.run(seed=300 + rep, first_event_id=2000)
        out.append(b)
    return out[:3], out[3:]


def _stats(plan, e, rep):
    eff, hyper, counts = plan[e]
    c = counts[rep]
    e1 = eff[1] + (1 if e == UNEQUAL and rep == 3 else 0)
    return [float(c[0]), float(c[1]), float(sum(c)), float(eff[0]), float(e1), float(hyper[0]), float(hyper[1])]


def test_through_batches(post):
    plan = _plan()
    g1, g2 = _batches(plan)
    zs = (0.1, -0.1)
    # what the batches hold already: a pairwise exact comparison with its quantiles, and summaries
    g1[0].compare_exact(g2[0], zs)
    g1[0].exact_delta_quantiles(g2[0])
    for b in g1 + g2:
        b.summarize()
    def stored():
        return ([g1[0].exact_comparison(i) for i in range(N_EVENTS)], [g1[0].exact_delta(i) for i in range(N_EVENTS)],
                [[b.summary(i) for i in range(N_EVENTS)] for b in g1 + g2], [b.last_kernels() for b in g1 + g2])
    before = repr(stored())
    # exact_stats is what the events were built from
    for rep, b in enumerate(g1 + g2):
        for e in range(N_EVENTS):
            st, was = b.exact_stats(e)
            assert was == (e != K3), (rep, e)
            if e != K3:
                assert list(st) == _stats(plan, e, rep), (rep, e)
    res = capi.exact_delta_groups_batches(g1, g2, P4[:3], zs)
    assert res.kernel_ms > 0.0
    assert [i for i in range(N_EVENTS) if not res.was_exact[i]] == [K3, UNEQUAL]
    # the wrapper equals the statistics route, and both the restatement, bit for bit
    take = [e for e in range(N_EVENTS) if e not in (K3,)]
    s1 = [[_stats(plan, e, rep) for rep in range(3)] for e in take]
    s2 = [[_stats(plan, e, rep) for rep in range(3, 5)] for e in take]
    direct = capi.exact_delta_groups(s1, s2, P4[:3], zs)
    for j, e in enumerate(take):
        assert res.was_exact[e] == direct.was_exact[j], e
        if e == UNEQUAL:
            assert res.row(e) is None and np.isnan(res.out[e]).all()
            continue
        assert np.array_equal(res.out[e], direct.out[j]), e
    for e in (0, 1):
        assert np.array_equal(res.out[e], group_delta(post, s1[take.index(e)], s2[take.index(e)], P4[:3], zs, _pairs)), e
    assert repr(stored()) == before


def test_batch_errors_name_the_group_and_the_index():
    from test_gpu_exact_paired import ISOLEN, MEAN, NOEXONS, Problem
    from _exact_paired_ref import fragment_dist
    shape = dict(chains=2, iters=60, burn=10, lag=1)
    m = np.tile([1.0, 1.0], (30, 1))

    def single(exact):
        b = miso_amd.Batch(READ_LEN, exact=exact, **shape)
        b.add_problem(m, [200, 150], [1, 1])
        b.run(seed=7, first_event_id=1)
        return b
    ex = [single(True) for _ in range(3)]
    plain = single(False)
    start, prob = fragment_dist(MEAN, 900.0, 4.0, READ_LEN)
    pe = miso_amd.Batch(READ_LEN, paired=True, mean=MEAN, var=900.0, exact_paired=True, **shape)
    q = Problem(np.random.default_rng(1), start, len(prob), 5, 5, 20)
    pe.add_problem(q.match, ISOLEN, NOEXONS, fraglen=q.fraglen)
    pe.run(seed=7, first_event_id=1)
    assert capi.exact_delta_groups_batches(ex[:2], ex[2:], [0.5]).was_exact[0] == 1
    with pytest.raises(miso_amd.InternalError, match="group 2 batch 1: .*exact-posterior mode"):
        capi.exact_delta_groups_batches(ex[:2], [ex[2], plain], [0.5])
    with pytest.raises(miso_amd.InternalError, match="group 1 batch 1: .*paired-end"):
        capi.exact_delta_groups_batches([ex[0], pe], ex[1:], [0.5])
    assert pe.exact_stats(0)[1] is False and plain.exact_stats(0)[1] is False
    for b1, b2, p, z in (([], ex, [0.5], ()), (ex * 3, ex, [0.5], ()), (ex[:1], ex[1:], [1.0], ()), (ex[:1], ex[1:], [0.5], [-1.0])):
        with pytest.raises(miso_amd.InternalError, match="Invalid value"):
            capi.exact_delta_groups_batches(b1, b2, p, z)


def test_quantiles_against_the_pooled_draws():
    """S = 5000 independent rows per replicate.  The fraction of ALL N1 N2 differences <= q_k is a two-sample U-statistic with
    mean p_k and variance at most p (1 - p) / min(N1, N2) <= p (1 - p) / S: |fraction - p_k| <= 5 sd + 1 / S; the same for
    the fraction <= 0 and H(0)"""
    S = 5000
    plan = _plan(seed=32)
    g1, g2 = _batches(plan, chains=2, iters=2500, burn=0, lag=1)
    res = capi.exact_delta_groups_batches(g1, g2, P4[:3])
    worst, n = 0.0, 0
    for e in range(N_EVENTS):
        row = res.row(e)
        if e in (K3, UNEQUAL):
            assert row is None
            continue
        _, _, q, H0, _ = row
        x1 = np.concatenate([b.result(e).samples[:, 0] for b in g1])
        x2 = np.sort(np.concatenate([b.result(e).samples[:, 0] for b in g2]))
        assert len(x1) == 3 * S and len(x2) == 2 * S
        for zq, p in list(zip(q, P4[:3])) + [(0.0, min(max(H0, 0.0), 1.0))]:
            # #{(i, j): x1_i - x2_j <= z} = sum_i #{j: x2_j >= x1_i - z}
            cnt = (len(x2) - np.searchsorted(x2, x1 - zq, side="left")).sum()
            frac = float(cnt) / (len(x1) * len(x2))
            bound = 5 * np.sqrt(p * (1 - p) / S) + 1.0 / S
            worst = max(worst, abs(frac - p) / bound)
            print("event %d z %.6f p %.6f fraction %.6f bound %.6f" % (e, zq, p, frac, bound))
            assert abs(frac - p) <= bound, (e, zq, frac, p, bound)
        n += 1
    assert n == N_EVENTS - 2
    print("worst |fraction - p| / bound %.3f over %d events" % (worst, n))
