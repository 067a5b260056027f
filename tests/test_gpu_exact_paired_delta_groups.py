"""The quantiles of delta psi between two groups of PAIRED-END replicates from the exact posteriors on the device
(csrc/kernels_exact_paired_delta_groups.hip, miso_exact_paired_delta_groups, miso_batch_exact_paired_delta_groups; DESIGN.md
section 20b).

Bit for bit against the restatement (tests/_exact_paired_delta_groups_ref.py, itself checked against mpmath in
tests/test_exact_paired_delta_groups_ref.py) on caller-given elements: every group shape from 1 x 1 to 8 x 8, the issue's two
cases under both hyperparameter pairs, the drawing-pair counts around the block of 16 and the chunk of 64, both widths of the
caller's sweep, launch ranges, a tie of the windows, events that are not comparable, the errors.  Device against device: one
replicate each is the pairwise kernel, H(z) the a-major mean of the pairwise comparison's.  Then whole batches, and the
quantiles against the mode's own draws.
"""
import numpy as np
import pytest

import miso_amd
from miso_amd import capi
from _exact_paired_compare_ref import HYPERS, PairedCompare, stats6
from _exact_paired_delta_groups_ref import GROUP_CASES, _TablesOnce, case_stats, group_delta
from _exact_paired_ref import PairedStats, fragment_dist
from _problems import simulate_pe
from test_gpu_exact_paired_delta import ISOLEN, MEAN, NOEXONS, READ_LEN, Problem

pytestmark = pytest.mark.gpu

AA, BB = (60000.0, 43000.0), (52000.0, 61000.0)
P4 = [0.5, 0.025, 0.975, 0.25]
Z8 = [0.1, -0.1, 0.2, -0.2, 0.0, 0.45, -0.6, 0.03]


@pytest.fixture(scope="module")
def post(orc):
    return _TablesOnce(PairedCompare(orc))


def _rnd(seed, n):
    return np.random.default_rng(seed).uniform(1e-5, 0.0133, size=(n, 2))


def _ps(n10, n01, nd, seed, A=AA, hyper=HYPERS[0]):
    return PairedStats(n10, n01, A[0], A[1], hyper[0], hyper[1], _rnd(seed, nd))


def _groups(events):
    """events: [(group 1's PairedStats, group 2's)], as many replicates in every event -> the two groups as
    capi.exact_paired_delta_groups takes them"""
    out = []
    for g in (0, 1):
        out.append([([stats6(ev[g][r]) for ev in events], [ev[g][r].m for ev in events]) for r in range(len(events[0][g]))])
    return out


def _call(events, probs, zs, per_launch=0):
    g1, g2 = _groups(events)
    return capi.exact_paired_delta_groups(g1, g2, probs, zs, max_events_per_launch=per_launch)


def _check(post, events, probs, zs, per_launch=0):
    res = _call(events, probs, zs, per_launch)
    assert res.out.shape == (len(events), 2 + len(probs) + 1 + len(zs)) and res.kernel_ms > 0.0
    for j, (g1, g2) in enumerate(events):
        want = group_delta(post, g1, g2, probs, zs)
        assert res.was_exact[j] == 1, j
        assert np.array_equal(res.out[j], want), (j, res.out[j], want)
    return res


def test_pairs_of_one_replicate_equal_the_pairwise_kernels():
    """device against device: (1, 1) is exact_paired_delta_quantiles, H(z) and the means exact_paired_compare's"""
    pairs = [(case_stats(n, h)[0][k], case_stats(n, h)[1][0]) for n in GROUP_CASES for h in HYPERS for k in (0, 1)]
    pairs += [(b, a) for a, b in pairs[:4]]
    zs = Z8[:3]
    res = _call([([a], [b]) for a, b in pairs], P4[:3], zs)
    s1, m1, s2, m2 = [stats6(a) for a, _ in pairs], [a.m for a, _ in pairs], [stats6(b) for _, b in pairs], [b.m for _, b in pairs]
    q = capi.selftest_exact_paired_delta_quantiles(s1, m1, s2, m2, P4[:3])
    c = capi.selftest_exact_paired_compare(s1, m1, s2, m2, zs)
    assert res.was_exact.all()
    assert np.array_equal(res.out[:, 2:6], q)
    assert np.array_equal(res.out[:, 6:], c[:, 5:]) and np.array_equal(res.out[:, :2], c[:, :2])


@pytest.mark.parametrize("n1,n2,n_p,n_z", [(1, 1, 3, 1), (2, 1, 4, 0), (1, 2, 1, 8)])
def test_small_groups_bit_exact(post, n1, n2, n_p, n_z):
    reps = [_ps(20, 80, 30, 1), _ps(80, 20, 17, 2), _ps(30, 35, 5, 3, BB, HYPERS[1])]
    _check(post, [(reps[:n1], reps[n1:n1 + n2])], P4[:n_p], Z8[:n_z])


def test_three_by_three_block_and_chunk_edges_and_mean_of_pairwise_cdfs(post):
    """the drawing-pair counts around exact_pair_logsum's block of 16 and chunk of 64 spread over the replicates of one
    call; H(z_j) is the a-major mean of the pairwise comparison kernel's cdf, device against device"""
    nds = [0, 1, 15, 16, 17, 63, 64, 65, 16, 64, 0, 33]
    reps = [_ps(3 + 5 * k, 40 - 3 * k, nd, 300 + k, AA if k % 3 else BB) for k, nd in enumerate(nds)]
    events = [(reps[0:3], reps[3:6]), (reps[6:9], reps[9:12])]
    zs = Z8[:4]
    res = _check(post, events, P4[:1], zs)
    for j, (g1, g2) in enumerate(events):
        pairs = [(a, b) for a in g1 for b in g2]
        c = capi.selftest_exact_paired_compare([stats6(a) for a, _ in pairs], [a.m for a, _ in pairs],
                                               [stats6(b) for _, b in pairs], [b.m for _, b in pairs], zs)
        for k in range(len(zs)):
            s = np.float64(0.0)
            for v in c[:, 5 + k]:
                s = s + v
            assert res.out[j, 4 + k] == s / np.float64(9.0), (j, k)
    # a permutation inside the groups: H moves by at most 1e-12 (N <= 64 terms in [0, 1])
    perm = _call([(g1[::-1], g2[1:] + g2[:1]) for g1, g2 in events], P4[:1], zs)
    assert np.abs(perm.out[:, 3:] - res.out[:, 3:]).max() <= 1e-12


@pytest.mark.parametrize("hyper", HYPERS, ids=["h11", "h25"])
@pytest.mark.parametrize("name,n_p,n_z", [("disagreeing", 4, 5), ("two-mode", 3, 4)])
def test_issue_cases_bit_exact(post, name, n_p, n_z, hyper):
    g1, g2 = case_stats(name, hyper)
    _check(post, [(g1, g2)], P4[:n_p], Z8[:n_z])


def test_eight_by_eight_bit_exact(post):
    """64 pairs an event, the limit: replicates repeat, so that the restatement tabulates few pairs, but every one of the 64
    terms is added on the device"""
    a, b, c, d = _ps(20, 80, 30, 11), _ps(80, 20, 17, 12), _ps(22, 75, 40, 13, BB), _ps(3, 9, 0, 14)
    events = [([a] * 4 + [b] * 4, [c] * 8), ([b] * 4 + [d] * 4, [a] * 4 + [c] * 4)]
    _check(post, events, P4[:1], Z8[:1])


def test_launch_ranges_do_not_change_the_bits(post):
    """five comparable events and one that is not: three ranges at two events a launch, the last ragged"""
    a, b, c, d = _ps(20, 80, 30, 21), _ps(80, 20, 17, 22), _ps(22, 75, 40, 23, BB), _ps(3, 9, 1, 24)
    low = PairedStats(5, 5, AA[0], AA[1], 0.5, 1.0, _rnd(25, 4))          # a hyperparameter below 1: not eligible
    events = [([a, b], [c]), ([b, a], [d]), ([a, low], [c]), ([a, b], [d]), ([d, c], [a]), ([c, c], [b])]
    ok = [0, 1, 3, 4, 5]
    one = _call(events, P4[:3], Z8[:2], per_launch=2)
    assert list(one.was_exact) == [1, 1, 0, 1, 1, 1] and one.row(2) is None and np.isnan(one.out[2]).all()
    for per in (0, 1, 5, 7):
        other = _call(events, P4[:3], Z8[:2], per_launch=per)
        assert np.array_equal(other.out[ok], one.out[ok]) and list(other.was_exact) == list(one.was_exact), per
    assert np.array_equal(one.out[3], group_delta(post, [a, b], [d], P4[:3], Z8[:2]))
    none = capi.exact_paired_delta_groups([(np.zeros((0, 6)), [])], [(np.zeros((0, 6)), [])], P4[:3], ())   # no event: no work
    assert none.out.shape == (0, 6) and none.kernel_ms == 0.0


def test_a_tie_of_the_windows_goes_to_group_1(post):
    same = _ps(7, 6, 20, 32, AA, HYPERS[1])
    twin = PairedStats(7, 6, AA[0], AA[1], HYPERS[1][0], HYPERS[1][1], same.m)
    other = _ps(9, 4, 0, 33)
    res = _check(post, [([same, other], [twin])], P4[:3], Z8[:1])
    H = post.cdf(same, twin)
    assert H.a_is_2 is False
    assert abs(res.out[0, 0] - (H.tabs[0]["mean0"] + post.cdf(other, twin).tabs[0]["mean0"]) / 2) < 1e-15


def test_errors_before_any_launch():
    good = _ps(1, 1, 1, 41)
    g = ([stats6(good)], [good.m])
    assert capi.exact_paired_delta_groups([g], [g], [0.5]).was_exact[0] == 1
    tiny = ([stats6(good)], [[(0.01, 2.0 ** -64)]])
    negative = ([[-1.0, 1.0, AA[0], AA[1], 1.0, 1.0]], [good.m])
    bad = [
        ([], [g], [0.5], ()),                                   # n1 = 0
        ([g] * 9, [g], [0.5], ()),                              # n1 = 9
        ([g], [g] * 9, [0.5], ()),                              # n2 = 9
        ([g], [g], [0.1, 0.2, 0.3, 0.4, 0.5], ()),              # n_p = 5
        ([g], [g], [], ()),                                     # n_p = 0
        ([g], [g], [1.0], ()),                                  # p = 1
        ([g], [g], [0.5], [1.0]),                               # z = 1
        ([g], [g], [0.5], [0.0] * 9),                           # n_z = 9
        ([g], [tiny], [0.5], ()),                               # a pair probability below 2^-63
        ([negative], [g], [0.5], ()),                           # a negative count
    ]
    for g1, g2, p, z in bad:
        with pytest.raises(miso_amd.InternalError, match="Invalid value"):
            capi.exact_paired_delta_groups(g1, g2, p, z)
    with pytest.raises(miso_amd.InternalError, match="Invalid value"):
        capi.exact_paired_delta_groups([g], [g], [0.5], (), max_events_per_launch=-1)
    with pytest.raises(ValueError):
        capi.exact_paired_delta_groups([g], [([stats6(good)] * 2, [good.m] * 2)])


# ---- through batches ----
N_EVENTS = 12
K3, NOT_IN_ONE = 4, 9          # a three-isoform event; an event that one batch's mode does not take (a hyperparameter below 1)
NDS = [0, 1, 15, 16, 17, 40, 63, 64, 65, 129]
VARS = (900.0, 1600.0, 1225.0, 700.0)


def _batches(orc, n_events=N_EVENTS, **shape):
    """2 + 2 paired-end batches over the same events, each with its own fragment-length distribution and read pairs"""
    shape = shape or dict(chains=2, iters=60, burn=10, lag=1)
    out = []
    for rep, var in enumerate(VARS):
        start, prob = fragment_dist(MEAN, var, 4.0, READ_LEN)
        rng = np.random.default_rng(70 + rep)
        b = miso_amd.Batch(READ_LEN, paired=True, mean=MEAN, var=var, exact_paired=True, **shape)
        probs = []
        for i in range(n_events):
            if i == K3:
                ex3, iso3, _, pos3, cig3 = simulate_pe(orc, 3, 120, mean=MEAN, var=var, seed=5 + i)
                b.add_event(miso_amd.Gene(ex3, iso3), pos3, cig3)
                probs.append(None)
                continue
            hyper = (2.0, 5.0) if i % 4 == 1 else None
            if i == NOT_IN_ONE and rep == 2:
                hyper = (0.5, 0.5)
            lean = 0.25 if rep < 2 else 0.6
            n_one = int(rng.integers(10, 50))
            n10 = int(round(n_one * min(max(lean + rng.normal(0, 0.08), 0.05), 0.95)))
            q = Problem(rng, start, len(prob), n10, n_one - n10, NDS[(i + 3 * rep) % len(NDS)], hyper=hyper)
            b.add_problem(q.match, ISOLEN, NOEXONS, fraglen=q.fraglen, hyper=q.hyper)
            probs.append(q)
        b.run(seed=400 + rep, first_event_id=3000)
        out.append((b, probs, start, prob))
    return out


def test_through_batches(orc, post):
    made = _batches(orc)
    bs = [m[0] for m in made]
    g1, g2 = bs[:2], bs[2:]
    zs = (0.1, -0.1)
    # what the batches hold already: a pairwise exact comparison with its quantiles, and summaries
    g1[0].compare_exact_paired(g2[0], zs)
    g1[0].exact_delta_quantiles(g2[0])
    for b in bs:
        b.summarize()

    def stored():
        return ([g1[0].exact_comparison(i) for i in range(N_EVENTS)], [g1[0].exact_delta(i) for i in range(N_EVENTS)],
                [[b.summary(i) for i in range(N_EVENTS)] for b in bs], [b.last_kernels() for b in bs])
    before = repr(stored())
    # exact_paired_element is what the events were built from: the statistics, and the pairs in record order
    elements = [[b.exact_paired_element(e) for e in range(N_EVENTS)] for b in bs]
    for rep, (b, probs, start, prob) in enumerate(made):
        for e in range(N_EVENTS):
            st, m, was = elements[rep][e]
            assert was == (e != K3 and not (e == NOT_IN_ONE and rep == 2)), (rep, e)
            if was:
                want = probs[e].stats(start, prob)
                assert list(st) == [float(v) for v in stats6(want)] and m.tobytes() == want.m.tobytes(), (rep, e)
            else:
                assert len(m) == 0
    res = capi.exact_paired_delta_groups_batches(g1, g2, P4[:3], zs)
    assert res.kernel_ms > 0.0
    assert [i for i in range(N_EVENTS) if not res.was_exact[i]] == [K3, NOT_IN_ONE]
    assert res.row(K3) is None and np.isnan(res.out[[K3, NOT_IN_ONE]]).all()
    # the wrapper equals the caller-given route fed from the batches' elements, and both the restatement, bit for bit
    groups = [[([el[0] for el in elements[rep]], [el[1] for el in elements[rep]]) for rep in reps] for reps in ((0, 1), (2, 3))]
    direct = capi.exact_paired_delta_groups(groups[0], groups[1], P4[:3], zs)
    assert list(direct.was_exact) == list(res.was_exact)
    ok = [e for e in range(N_EVENTS) if res.was_exact[e]]
    assert np.array_equal(res.out[ok], direct.out[ok])
    for e in (0, 5):
        ps = [made[rep][1][e].stats(made[rep][2], made[rep][3]) for rep in range(4)]
        assert np.array_equal(res.out[e], group_delta(post, ps[:2], ps[2:], P4[:3], zs)), e
    assert repr(stored()) == before


def test_batch_errors_name_the_group_and_the_index():
    shape = dict(chains=2, iters=60, burn=10, lag=1)
    start, prob = fragment_dist(MEAN, 900.0, 4.0, READ_LEN)
    q = Problem(np.random.default_rng(1), start, len(prob), 5, 5, 20)

    def paired(mode):
        b = miso_amd.Batch(READ_LEN, paired=True, mean=MEAN, var=900.0, exact_paired=mode, **shape)
        b.add_problem(q.match, ISOLEN, NOEXONS, fraglen=q.fraglen)
        b.run(seed=7, first_event_id=1)
        return b
    ex = [paired(True) for _ in range(3)]
    plain = paired(False)
    se = miso_amd.Batch(READ_LEN, exact=True, **shape)
    se.add_problem(np.tile([1.0, 1.0], (30, 1)), [200, 150], [1, 1])
    se.run(seed=7, first_event_id=1)
    assert capi.exact_paired_delta_groups_batches(ex[:2], ex[2:], [0.5]).was_exact[0] == 1
    with pytest.raises(miso_amd.InternalError, match="group 2 batch 1: .*paired exact-posterior mode"):
        capi.exact_paired_delta_groups_batches(ex[:2], [ex[2], plain], [0.5])
    with pytest.raises(miso_amd.InternalError, match="group 1 batch 1: .*single-end"):
        capi.exact_paired_delta_groups_batches([ex[0], se], ex[1:], [0.5])
    assert se.exact_paired_element(0)[2] is False and plain.exact_paired_element(0)[2] is False
    # the single-end pass keeps its error on paired-end batches
    with pytest.raises(miso_amd.InternalError, match="group 1 batch 0: .*paired-end"):
        capi.exact_delta_groups_batches(ex[:1], ex[1:], [0.5])
    for b1, b2, p, z in (([], ex, [0.5], ()), (ex * 3, ex, [0.5], ()), (ex[:1], ex[1:], [1.0], ()), (ex[:1], ex[1:], [0.5], [-1.0])):
        with pytest.raises(miso_amd.InternalError, match="Invalid value"):
            capi.exact_paired_delta_groups_batches(b1, b2, p, z)


def test_quantiles_against_the_pooled_draws(orc):
    """S = 5000 independent rows per replicate, all from one launch of each batch.  The fraction of ALL N1 N2 differences
    <= q_k is a two-sample U-statistic with mean p_k and variance at most p (1 - p) / min(N1, N2) <= p (1 - p) / S:
    |fraction - p_k| <= 5 sd + 1 / S; the same for the fraction <= 0 and H(0)"""
    S, n_events = 5000, 10
    made = _batches(orc, n_events=n_events, chains=2, iters=2500, burn=0, lag=1)
    g1, g2 = [m[0] for m in made[:2]], [m[0] for m in made[2:]]
    res = capi.exact_paired_delta_groups_batches(g1, g2, P4[:3])
    worst, n = 0.0, 0
    for e in range(n_events):
        row = res.row(e)
        if e in (K3, NOT_IN_ONE):
            assert row is None
            continue
        _, _, q, H0, _ = row
        x1 = np.concatenate([b.result(e).samples[:, 0] for b in g1])
        x2 = np.sort(np.concatenate([b.result(e).samples[:, 0] for b in g2]))
        assert len(x1) == 2 * S and len(x2) == 2 * S
        for zq, p in list(zip(q, P4[:3])) + [(0.0, min(max(H0, 0.0), 1.0))]:
            # #{(i, j): x1_i - x2_j <= z} = sum_i #{j: x2_j >= x1_i - z}
            cnt = (len(x2) - np.searchsorted(x2, x1 - zq, side="left")).sum()
            frac = float(cnt) / (len(x1) * len(x2))
            bound = 5 * np.sqrt(p * (1 - p) / S) + 1.0 / S
            worst = max(worst, abs(frac - p) / bound)
            print("event %d z %.6f p %.6f fraction %.6f bound %.6f" % (e, zq, p, frac, bound))
            assert abs(frac - p) <= bound, (e, zq, frac, p, bound)
        n += 1
    assert n == n_events - 2
    print("worst |fraction - p| / bound %.3f over %d events" % (worst, n))
