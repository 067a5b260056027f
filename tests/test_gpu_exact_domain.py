"""The exact-posterior family on the device over the eligible domain's sweep (tests/_exact_domain.py; DESIGN.md sections
15 - 20b), through the entry points that take raw statistics:

  * against the restatements bit for bit, at inputs the fixed case lists do not hold (both selects of exact_point, the
    clamps of exact_cdf_at, the partial blocks and chunks of exact_pair_logsum, the fext points of exact_paired_table), the
    probabilities extended by the two extreme draws;
  * against the closed forms directly, at the tolerances of tests/test_exact_domain_ref.py -- this part does not read the
    restatements, so it stands if they and the kernels share a mistake;
  * identities between the device's own outputs: bit equalities where DESIGN.md states them, tolerances elsewhere;
  * an event beyond the fence runs the sampler, in either mode, as the same event does without the mode.
"""
import numpy as np
import pytest

import miso_amd
from miso_amd import capi
import _exact_domain as D
from _exact_compare_ref import ZS, compare
from _exact_delta_ref import PROBS as DELTA_PROBS
from _exact_delta_ref import delta_quantiles, paired_delta_quantiles
from _exact_paired_compare_ref import PairedCompare
from _exact_paired_ref import PairedStats, fragment_dist
from _exact_ref import Posterior, Stats
from test_exact_compare_ref import H_TOL
from test_exact_delta_ref import C
from test_gpu_exact import READ_LEN, add_case
from test_gpu_exact_paired import MEAN, Problem

pytestmark = pytest.mark.gpu

MEAN_TOL, QUANT_TOL = D.MEAN_TOL, D.QUANT_TOL
EQ = D.eq_cases()
C0 = {r: D.c0_cases(r) for r in D.RATIOS}
POOL = EQ + [c for r in D.RATIOS for c in C0[r]]
CORNERS = [c for c in POOL if D.HYPER_MAX in c[5:] or c[3] / c[4] in (D.RATIO_MAX, 1.0 / D.RATIO_MAX) or c[3] in (D.LEN_MIN, D.LEN_MAX)]
# bit for bit against the restatement: the fence's corners, then every seventh case of the sweep, at most 64 rows a test
BIT_ROWS = (CORNERS + POOL[::7])
BIT_PARTS = [BIT_ROWS[i:i + 64] for i in range(0, len(BIT_ROWS), 64)]
MIRROR = [4, 3, 2, 1, 0, 6, 5]          # ALL_PROBS[MIRROR[k]] = 1 - ALL_PROBS[k]
TOL7 = np.array([QUANT_TOL] * 5 + [C] * 2)
PAIRED = D.ratio_cases() + D.peq_cases()
PAIRS = D.compare_pairs()
BEYOND = [(5, 5, 0, 100, 100, 1.0, 1e20), (5, 5, 0, 100, 100, 1e30, 1.0)]      # the two inputs that gave garbage and NaN


@pytest.fixture(scope="module")
def post(orc):
    return Posterior(orc)


@pytest.fixture(scope="module")
def ppost(orc):
    return PairedCompare(orc)


def device(cases):
    out8, icdf = capi.selftest_exact([D.row7(c) for c in cases], D.ALL_PROBS)
    return out8, icdf


def device_paired(pcases):
    return capi.selftest_exact_paired([D.stats6(pc) for pc in pcases], [pc[7] for pc in pcases], D.ALL_PROBS)


# ---- bit for bit against the restatements ----

@pytest.mark.parametrize("part", range(len(BIT_PARTS)))
def test_single_end_bit_exact_on_the_sweep(post, part):
    cases = BIT_PARTS[part]
    assert 0 < len(cases) <= 64
    out8, icdf = device(cases)
    for j, c in enumerate(cases):
        tab = post.tabulate(Stats(*D.row7(c)))
        want = np.array([tab[k] for k in ("mean0", "mean1", "tL", "tR", "Z", "tm", "h", "gmax")], dtype=np.float64)
        assert np.array_equal(out8[j], want), (c, out8[j], want)
        assert np.array_equal(icdf[j], post.icdf(tab, D.ALL_PROBS)), c


def test_paired_end_bit_exact_on_every_block_and_chunk_boundary(ppost):
    out8, icdf = device_paired(PAIRED)
    for j, pc in enumerate(PAIRED):
        tab = ppost.tabulate(PairedStats(*pc[1:8]))
        assert np.array_equal(out8[j], ppost.out8(tab)), (pc[0], out8[j], ppost.out8(tab))
        assert np.array_equal(icdf[j], ppost.icdf(tab, D.ALL_PROBS)), pc[0]


# ---- against the closed forms ----

def test_equal_lengths_against_the_beta_law():
    out8, icdf = device(EQ)
    D.assert_eq("device, EQ", EQ, out8[:, :2], icdf)


@pytest.mark.parametrize("ratio", D.RATIOS, ids=lambda r: "ratio%.3g" % r)
def test_unequal_lengths_against_the_substituted_beta_law(ratio):
    out8, icdf = device(C0[ratio])
    D.assert_c0("device, C0 e0/e1 = %g" % ratio, C0[ratio], icdf)
    assert np.abs(out8[:, :2].sum(axis=1) - 1.0).max() < 1e-14


def test_unequal_lengths_means():
    cases = D.c0_mean_cases()
    out8, _ = device(cases)
    for c, m in zip(cases, out8):
        want = D.c0_mean(c)
        assert abs(m[0] - want) < MEAN_TOL and abs(m[1] - (1.0 - want)) < MEAN_TOL, (c, m[:2], want)


_paired_out = []


def paired_device():
    """the paired sweep's one launch, made once for the tests below"""
    if not _paired_out:
        _paired_out.extend(device_paired(PAIRED))
    return _paired_out


@pytest.mark.parametrize("j", range(len(D.ratio_cases())), ids=[pc[0] for pc in D.ratio_cases()])
def test_paired_ratio_family_against_quadrature(j):
    """RATIO at every pair count: a pair dropped or read twice leaves a factor (1 + x) behind, and the reference knows no pairs"""
    out8, icdf = paired_device()
    D.assert_ratio(PAIRED[j], out8[j, :2], icdf[j])


def test_paired_constant_factors_against_the_beta_law():
    out8, icdf = paired_device()
    n = len(D.ratio_cases())
    D.assert_eq("device, PEQ / PMIN", [pc[8] for pc in PAIRED[n:]], out8[n:, :2], icdf[n:])


def _pair_rows():
    return [D.row7(p[1]) for p in PAIRS], [D.row7(p[2]) for p in PAIRS]


def test_comparisons_against_the_closed_forms():
    r1, r2 = _pair_rows()
    out = capi.selftest_exact_compare(r1, r2, ZS)
    dq = capi.selftest_exact_delta_quantiles(r1, r2, DELTA_PROBS)
    for j, (name, c1, c2) in enumerate(PAIRS):
        D.assert_log_d0(name, c1, c2, out[j, 2])
        a1, b1, a2, b2 = c1[0] + c1[5], c1[1] + c1[6], c2[0] + c2[5], c2[1] + c2[6]
        assert abs(out[j, 0] - a1 / (a1 + b1)) < MEAN_TOL and abs(out[j, 1] - a2 / (a2 + b2)) < MEAN_TOL, name
        assert (np.diff(out[j, 5:]) >= 0).all() and (out[j, 5:] >= 0).all() and (out[j, 5:] <= 1).all(), name
        assert dq[j, 3] == out[j, 5 + ZS.index(0.0)], name          # H0 is the comparison's H(0.0), DESIGN.md section 20
        D.assert_pair_shape(name, dq[j, 3], dq[j, :3])
        if name.startswith("opposite-ends"):                        # the whole mass of the difference lies below every z of ZS
            assert np.abs(out[j, 5:] - 1.0).max() <= H_TOL, (name, out[j, 5:])


# ---- bit for bit: the comparisons at the new pairs ----

def test_comparisons_bit_exact(post):
    r1, r2 = _pair_rows()
    out = capi.selftest_exact_compare(r1, r2, ZS)
    dq = capi.selftest_exact_delta_quantiles(r1, r2, DELTA_PROBS)
    for j, (name, _, _) in enumerate(PAIRS):
        assert np.array_equal(out[j], compare(post, r1[j], r2[j], ZS)), name
        assert np.array_equal(dq[j], delta_quantiles(post, r1[j], r2[j])), name


def _paired_pairs():
    """pairs of paired-end elements: two constant-factor elements (Beta laws: a closed form for log_d0), two RATIO elements
    across a chunk boundary, a self-pair"""
    by = {pc[0]: pc for pc in PAIRED}
    return [("peq", by["peq-17"], by["peq-1"]), ("ratio", by["ratio-65"], by["ratio-81"]), ("self", by["ratio-17"], by["ratio-17"])]


def test_paired_comparisons_bit_exact_and_closed_form(ppost):
    pp = _paired_pairs()
    s1, m1 = [D.stats6(p[1]) for p in pp], [p[1][7] for p in pp]
    s2, m2 = [D.stats6(p[2]) for p in pp], [p[2][7] for p in pp]
    out = capi.selftest_exact_paired_compare(s1, m1, s2, m2, ZS)
    dq = capi.selftest_exact_paired_delta_quantiles(s1, m1, s2, m2, DELTA_PROBS)
    for j, (name, p1, p2) in enumerate(pp):
        ps1, ps2 = PairedStats(*p1[1:8]), PairedStats(*p2[1:8])
        want, _ = ppost.compare(ps1, ps2, ZS)
        assert np.array_equal(out[j], want), (name, out[j], want)
        assert np.array_equal(dq[j], paired_delta_quantiles(ppost, ps1, ps2)), name
        assert dq[j, 3] == out[j, 5 + ZS.index(0.0)], name
        D.assert_pair_shape(name, dq[j, 3], dq[j, :3])
    # the log normalisers' sizes, for the project's bound on log_d0: |log Z_12| <= |log_d0| + |log Z_1| + |log Z_2|
    lz1, lz2 = device_paired([p[1] for p in pp])[0][:, 7], device_paired([p[2] for p in pp])[0][:, 7]
    weights = [2.0 * sum(sum(q[8][:3]) + q[8][0] + q[8][1] + q[8][5] + q[8][6] for q in p[1:]) for p in pp]
    bounds = [D.log_d0_bound(2.0 * (abs(a) + abs(b)) + abs(d), w) for a, b, d, w in zip(lz1, lz2, out[:, 2], weights)]
    # a constant factor per pair and equal A: the pairs' normalisers cancel in log_d0 as the lengths' do
    c1, c2 = pp[0][1][8], pp[0][2][8]
    want, _ = D.log_d0_reference((c1[0], c1[1], 0, 1.0, 1.0, c1[5], c1[6]), (c2[0], c2[1], 0, 1.0, 1.0, c2[5], c2[6]))
    assert abs(out[0, 2] - want) <= bounds[0], (out[0, 2], want, bounds[0])
    # groups of one replicate each are the plain pair, bit for bit; swapped samples
    g = capi.exact_paired_delta_groups([(s1, m1)], [(s2, m2)], DELTA_PROBS, ZS)
    assert g.was_exact.all() and np.array_equal(g.out[:, 2:6], dq) and np.array_equal(g.out[:, 6:], out[:, 5:])
    sw = capi.selftest_exact_paired_compare(s2, m2, s1, m1, ZS)
    dsw = capi.selftest_exact_paired_delta_quantiles(s2, m2, s1, m1, DELTA_PROBS)
    _assert_swapped(out, dq, sw, dsw, [p[0] for p in pp], bounds)


# ---- identities on the device's own outputs ----

def test_swapping_the_isoform_labels_mirrors_the_posterior():
    cases = BIT_ROWS
    out8, icdf = device(cases)
    sw8, swq = device([D.swap_labels(c) for c in cases])
    assert np.abs(sw8[:, 0] - out8[:, 1]).max() < 2 * MEAN_TOL and np.abs(sw8[:, 1] - out8[:, 0]).max() < 2 * MEAN_TOL
    # q'(p) = 1 - q(1 - p): the swapped posterior's x against the 1 - x of the mirrored probability, and the other way round
    for col in (0, 1):
        d = np.abs(swq[:, :, col] - icdf[:, MIRROR, 1 - col])
        bad = np.nonzero((d >= 2 * TOL7).any(axis=1))[0]
        assert len(bad) == 0, [(D.case_id(cases[k]), d[k].tolist()) for k in bad[:5]]


def test_equal_lengths_do_not_depend_on_n11_or_the_length():
    base = EQ[::4]
    other = [(c[0], c[1], [7, 10 ** 6, 0][i % 3], e, e, c[5], c[6]) for i, c in enumerate(base)
             for e in ([D.LEN_MAX, 1.0, 1e-5, 31.0][i % 4],)]
    a8, aq = device(base)
    b8, bq = device(other)
    assert np.abs(a8[:, :2] - b8[:, :2]).max() < 2 * MEAN_TOL
    assert (np.abs(aq - bq) < 2 * TOL7[None, :, None]).all()


def _assert_swapped(out, dq, sw, dsw, names, bounds):
    """samples swapped: the means change places exactly; the same log_d0, hence Bayes factor, both within bounds[j]
    (_exact_domain.log_d0_bound) of the truth; H(z) <-> 1 - H(-z) within 1e-5 and q(p) <-> -q(1 - p) within 2 C, as
    tests/test_exact_delta_ref.py has them"""
    for j, name in enumerate(names):
        assert (out[j, 0], out[j, 1]) == (sw[j, 1], sw[j, 0]), name
        bound = 2 * bounds[j]
        assert abs(out[j, 2] - sw[j, 2]) <= bound, (name, out[j, 2], sw[j, 2], bound)
        assert abs(out[j, 4] - sw[j, 4]) <= (bound + 8 * 2.0 ** -53 * (abs(out[j, 2]) + abs(out[j, 4]) * np.log(10.0) + 1.0)) / np.log(10.0), name
        for k, z in enumerate(ZS):
            if -z in ZS:
                assert abs(sw[j, 5 + ZS.index(-z)] - (1.0 - out[j, 5 + k])) <= 1e-5, (name, z)
        q, qs = dict(zip(DELTA_PROBS, dq[j, :3])), dict(zip(DELTA_PROBS, dsw[j, :3]))
        for p, o in ((0.5, 0.5), (0.025, 0.975), (0.975, 0.025)):
            assert abs(qs[p] + q[o]) <= 2 * C, (name, p, qs[p], q[o])
        assert abs((1.0 - dsw[j, 3]) - dq[j, 3]) <= 1e-5, name


def test_swapping_the_samples_of_a_pair():
    r1, r2 = _pair_rows()
    out, sw = capi.selftest_exact_compare(r1, r2, ZS), capi.selftest_exact_compare(r2, r1, ZS)
    dq, dsw = capi.selftest_exact_delta_quantiles(r1, r2, DELTA_PROBS), capi.selftest_exact_delta_quantiles(r2, r1, DELTA_PROBS)
    _assert_swapped(out, dq, sw, dsw, [p[0] for p in PAIRS], [D.log_d0_reference(p[1], p[2])[1] for p in PAIRS])


def test_replicate_groups_of_one_and_permuted_replicates():
    r1, r2 = _pair_rows()
    out = capi.selftest_exact_compare(r1, r2, ZS)
    dq = capi.selftest_exact_delta_quantiles(r1, r2, DELTA_PROBS)
    g = capi.exact_delta_groups(np.array(r1)[:, None, :], np.array(r2)[:, None, :], DELTA_PROBS, ZS)
    assert g.was_exact.all()
    assert np.array_equal(g.out[:, 2:6], dq) and np.array_equal(g.out[:, 6:], out[:, 5:]) and np.array_equal(g.out[:, :2], out[:, :2])
    # three replicates a group, all with one pair of lengths; the replicates of both groups permuted
    e = 150.0
    reps = [D.row7((n10, n01, n11, e, e, 1.0, 1.0)) for n10, n01, n11 in [(5, 5, 0), (5 * 10 ** 6, 5 * 10 ** 6, 0), (0, 10 ** 6, 5),
                                                                           (200010, 199990, 0), (11, 5, 17), (1000, 0, 0)]]
    g1, g2 = np.array([reps[:3], reps[3:]]), np.array([reps[3:], reps[:3]])
    a = capi.exact_delta_groups(g1, g2, DELTA_PROBS, ZS)
    b = capi.exact_delta_groups(g1[:, [2, 0, 1]], g2[:, [1, 2, 0]], DELTA_PROBS, ZS)
    assert a.was_exact.all() and b.was_exact.all()
    assert np.abs(a.out[:, 5:] - b.out[:, 5:]).max() <= 1e-12           # H moves by at most 1e-12
    assert np.abs(a.out[:, 2:5] - b.out[:, 2:5]).max() <= C and np.abs(a.out[:, :2] - b.out[:, :2]).max() < MEAN_TOL


# ---- beyond the fence ----

def test_beyond_the_fence_the_entry_points_refuse():
    ok = D.row7((5, 5, 0, 100, 100, 1.0, 1.0))
    el = capi.C.c_int(-1)
    for c in BEYOND + [(5, 5, 0, 100.0, float("inf"), 1.0, 1.0), (5, 5, 0, 2.0 ** 21, 1.0, 1.0, 1.0)]:
        row = D.row7(c)
        assert capi.lib().miso_exact_eligible(0, 2, capi._p(np.array(row[3:5])), capi._p(np.array(row[5:])), capi.C.byref(el)) == 0
        assert el.value == 0, c
        with pytest.raises(miso_amd.InternalError, match="not eligible"):
            capi.selftest_exact([ok, row], [0.5])
        for fn in (capi.selftest_exact_compare, capi.selftest_exact_delta_quantiles):
            with pytest.raises(miso_amd.InternalError, match="not eligible"):
                fn([ok, row], [ok, row])        # (the same lengths on both sides: only the fence is in the way)
        g = capi.exact_delta_groups(np.array([[ok], [ok]]), np.array([[ok], [row]]))
        assert list(g.was_exact) == [1, 0] and g.row(1) is None
        s6 = [row[0], row[1]] + row[3:]
        ok6 = [ok[0], ok[1]] + ok[3:]
        with pytest.raises(miso_amd.InternalError, match="not eligible"):
            capi.selftest_exact_paired([ok6, s6], [[], []], [0.5])
        for fn in (capi.selftest_exact_paired_compare, capi.selftest_exact_paired_delta_quantiles):
            with pytest.raises(miso_amd.InternalError, match="not eligible"):
                fn([ok6, ok6], [[], []], [ok6, s6], [[], []])
        g = capi.exact_paired_delta_groups([([ok6, ok6], [[], []])], [([ok6, s6], [[], []])])
        assert list(g.was_exact) == [1, 0]


def _same_event(a, e, what):
    assert np.array_equal(a.samples, e.samples, equal_nan=True) and np.array_equal(a.loglik, e.loglik, equal_nan=True), what
    assert np.array_equal(a.assignment, e.assignment) and (a.counts_hash == e.counts_hash).all(), what
    assert np.array_equal(a.counts_trace, e.counts_trace), what
    assert all(getattr(a.rundata, f) == getattr(e.rundata, f) for f, _ in capi.RunData._fields_), what


def test_single_end_batch_beyond_the_fence_runs_the_sampler():
    """the two quoted inputs and a hyperparameter one beyond its bound, next to an eligible event: the mode takes only that
    one, and the others are the sampler's results, bit for bit what a batch without the mode gives"""
    kw = dict(chains=2, iters=60, burn=10, lag=1)
    events = [((5, 5, 0, 100, 100), h) for h in [(1.0, 1e20), (1e30, 1.0), (1.0, D.HYPER_MAX + 1.0), (1.0, 1.0)]]
    runs = []
    for exact in (False, True):
        b = miso_amd.Batch(READ_LEN, exact=exact, counts_trace=True, **kw)
        for c, h in events:
            add_case(b, c, h)
        b.run(seed=12, first_event_id=300)
        runs.append(b)
    plain, mode = runs
    assert "exact_sample" in mode.last_kernels().split(",") and "exact_sample" not in plain.last_kernels()
    assert mode.exact_summary(3) is not None
    for i in range(3):
        assert mode.exact_summary(i) is None, events[i]
        _same_event(plain.result(i, trace=True), mode.result(i, trace=True), events[i])


def test_paired_end_batch_beyond_the_fence_runs_the_sampler():
    kw = dict(chains=2, iters=60, burn=10, lag=1)
    start, prob = fragment_dist(MEAN, 900.0, 4.0, READ_LEN)
    hypers = [(1.0, 1e20), (D.HYPER_MAX + 1.0, 1.0), (1.0, 1.0)]
    runs = []
    for exact_paired in (False, True):
        rng = np.random.default_rng(29)
        b = miso_amd.Batch(READ_LEN, paired=True, mean=MEAN, var=900.0, exact_paired=exact_paired, counts_trace=True, **kw)
        for h in hypers:
            Problem(rng, start, len(prob), 5, 8, 17, hyper=h).add(b)
        b.run(seed=77, first_event_id=900)
        runs.append(b)
    plain, mode = runs
    assert "exact_paired_sample" in mode.last_kernels().split(",") and "exact_paired_sample" not in plain.last_kernels()
    assert mode.exact_summary(2) is not None
    for i in range(2):
        assert mode.exact_summary(i) is None, hypers[i]
        _same_event(plain.result(i, trace=True), mode.result(i, trace=True), hypers[i])
