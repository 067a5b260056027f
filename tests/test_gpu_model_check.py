"""GPU: the posterior predictive model check (csrc/kernels_model_check.hip) against its restatement
(tests/_model_check_ref.py), bit for bit; its law against exact enumeration; the batch's pass against the raw call; and
that it sees what it is for.  The shapes are the smallest at which the kernel can still go wrong: fewer rows than a
wavefront, exactly one pass of the workgroup and one row more, several passes; one class (no binomial), two, the three of
a skipped exon, 7, and the limit of 64; both routines of the sampler and the long table of log factorials in one event."""
import numpy as np
import pytest

import _model_check_ref as R
from miso_amd import capi

pytestmark = pytest.mark.gpu

SEED = 0x1234567890AB          # both key words non-zero
SKIP_PATTERN, SKIP_M = [2, 1, 3], [35, 85, 130]     # exons [1,100] [201,250] [351,450], read length 36


def _rows(rng, S, K):
    return rng.dirichlet(np.ones(K), size=S)


def _events():
    """(name, K, pattern, m, n, samples [S, K])"""
    rng = np.random.default_rng(20)
    ev = []
    ev.append(("k2_c3_n9_s257", 2, SKIP_PATTERN, SKIP_M, [2, 3, 4], _rows(rng, 257, 2)))
    ev.append(("k2_c3_n200_s700", 2, SKIP_PATTERN, SKIP_M, [20, 50, 130], _rows(rng, 700, 2)))
    ev.append(("no_reads", 2, SKIP_PATTERN, SKIP_M, [0, 0, 0], _rows(rng, 63, 2)))
    ev.append(("k2_c1_n1_s1", 2, [3], [40], [1], _rows(rng, 1, 2)))
    ev.append(("k3_c2_n9_s63", 3, [5, 6], [12, 30], [4, 5], _rows(rng, 63, 3)))
    pats = [int(x) for x in rng.choice(np.arange(1, 64), size=7, replace=False)]
    ev.append(("k6_c7_n200_s256", 6, pats, [int(x) for x in rng.integers(1, 90, 7)], [10, 20, 30, 40, 50, 0, 50], _rows(rng, 256, 6)))
    ev.append(("too_many_classes", 64, [1 << (c % 64) for c in range(65)], [1] * 65, [1] * 65, _rows(rng, 1, 64)))
    ev.append(("k64_c64_n200_s63", 64, [1 << c for c in range(64)], [int(x) for x in rng.integers(1, 50, 64)],
               [int(x) for x in rng.multinomial(200, np.ones(64) / 64)], _rows(rng, 63, 64)))
    # one class of probability ~ 1e-4 (inversion) beside a large one (BTRS on ~ 100 000 reads)
    ev.append(("k2_c3_n100000_s63", 2, SKIP_PATTERN, [1, 5000, 5000], [8, 33000, 66992], 0.4 + 0.2 * _rows(rng, 63, 2)))
    # rows: psi_0 = 0 where class 0 has reads; psi_1 = 0 where class 1 has none; psi_2 = 0, so that w_1 / T_1 is exactly 1
    # before the last class; an all-zero row; a NaN row; ordinary rows between
    special = np.array([[0.0, 0.5, 0.5], [0.2, 0.3, 0.5], [0.5, 0.0, 0.5], [0.3, 0.7, 0.0], [0.0, 0.0, 0.0],
                        [0.1, np.nan, 0.2], [0.6, 0.3, 0.1], [0.0, 0.0, 1.0], [1 / 3, 1 / 3, 1 / 3]])
    ev.append(("special_rows", 3, [1, 2, 4], [50, 20, 30], [5, 0, 4], special))
    ev.append(("k2_c2_n9_s256", 2, [1, 2], [85, 35], [6, 3], _rows(rng, 256, 2)))
    return ev


@pytest.fixture(scope="module")
def events():
    return _events()


@pytest.fixture(scope="module")
def reference(orc, events):
    """the restatement of every event, computed once and left unchanged"""
    stats = {}
    out = [R.model_check(orc, pat, m, n, rows, 100 + i, SEED, stats=stats) for i, (_, K, pat, m, n, rows) in enumerate(events)]
    return out, stats


def _device(events, seed=SEED):
    return capi.model_check([e[1] for e in events], [e[2] for e in events], [e[3] for e in events], [e[4] for e in events],
                            [e[5] for e in events], event_id=[100 + i for i in range(len(events))], seed=seed)[0]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same(name, got, want):
    assert got.status == want["status"], (name, got.status, want["status"])
    for f in ("rows", "bad_rows", "exceed"):
        assert getattr(got, f) == want[f], (name, f, getattr(got, f), want[f])
    for f in ("ge", "le"):
        assert np.array_equal(getattr(got, f), want[f]), (name, f, getattr(got, f), want[f])
    for f in ("sum_obs", "sum_rep", "expected"):
        assert np.array_equal(_bits(getattr(got, f)), _bits(want[f])), (name, f, getattr(got, f), want[f])


def test_raw_call_equals_the_restatement_bit_for_bit(events, reference):
    want, stats = reference
    assert stats.get("inversion", 0) > 0 and stats.get("btrs", 0) > 0, stats      # both routines of the sampler were met
    got = _device(events)
    by_name = {e[0]: g for e, g in zip(events, got)}
    assert by_name["no_reads"].status == "no_reads" and by_name["too_many_classes"].status == "too_many_classes"
    assert (by_name["special_rows"].rows, by_name["special_rows"].bad_rows) == (7, 2)
    for e, g, w in zip(events, got, want):
        _same(e[0], g, w)


def test_the_same_call_twice_gives_the_same_bytes(events):
    a, b = _device(events), _device(events)
    for e, x, y in zip(events, a, b):
        _same(e[0], x, {f: getattr(y, f) for f in ("status", "rows", "bad_rows", "exceed", "ge", "le", "sum_obs", "sum_rep", "expected")})
    c = _device(events, seed=SEED + 1)      # ... and the seed is used
    assert any(x.exceed != y.exceed for x, y in zip(a, c))


def test_the_law_on_the_device():
    """the enumeration case of tests/test_model_check_ref.py through the kernel, the same bounds"""
    samples = np.tile(np.array(R.ENUM_PSI), (R.ENUM_ROWS, 1))
    (fit,), _ = capi.model_check([2], [R.ENUM_PATTERN], [R.ENUM_M], [R.ENUM_N], [samples], event_id=[11], seed=2024)
    assert fit.status == "ok"
    R.check_enum({"rows": fit.rows, "bad_rows": fit.bad_rows, "exceed": fit.exceed, "ge": fit.ge, "le": fit.le})


def test_refused_tables_leave_the_results_alone():
    rows = np.full((4, 2), 0.5)
    for pat, m, n in (([4, 1, 3], SKIP_M, [1, 1, 1]), ([0, 1, 3], SKIP_M, [1, 1, 1]), (SKIP_PATTERN, [0, 85, 130], [1, 1, 1]),
                      (SKIP_PATTERN, SKIP_M, [1, -1, 1])):
        with pytest.raises(capi.InternalError):
            capi.model_check([2], [pat], [m], [n], [rows])


# ---- the batch's pass ----
GENE = ([(1, 100), (201, 250), (351, 450)], [(0, 1, 2), (0, 2)])
# one read of every class: on both isoforms (exon 1), on the inclusion isoform alone (exon 2), on the skipping junction
READ = {3: (1, "36M"), 1: (205, "36M"), 2: (80, "21M250N15M")}


def _planted(n01, n10, n11):
    pos, cig = [], []
    for pat, count in ((2, n01), (1, n10), (3, n11)):
        pos += [READ[pat][0]] * count
        cig += [READ[pat][1]] * count
    return pos, cig


def _raw_of_batch(b, n_events, first_id, seed):
    tabs = [b.model_check_table(i) for i in range(n_events)]
    rows = [b.result(i).samples for i in range(n_events)]
    return capi.model_check([r.shape[1] for r in rows], [t["pattern"] for t in tabs], [t["m"] for t in tabs], [t["n"] for t in tabs],
                            rows, event_id=[first_id + i for i in range(n_events)], seed=seed)[0]


def _fit_dict(f):
    return {k: getattr(f, k) for k in ("status", "rows", "bad_rows", "exceed", "ge", "le", "sum_obs", "sum_rep", "expected")}


def _small_batch(model_check, **kw):
    from miso_amd import workload
    b = capi.Batch(36, iters=300, burn=100, lag=2, chains=2, model_check=model_check, **kw)
    for j, (K, n) in enumerate([(2, 400), (3, 250), (2, 0), (5, 300), (2, 37)]):
        exons, isoforms, pos, cig = workload.event_reads(40 + j, K=K, n_reads=max(n, 1))
        b.add_event(capi.Gene(exons, isoforms), pos[:n], cig[:n])
    return b


@pytest.mark.parametrize("exact", [False, True], ids=["chains", "exact"])
def test_batch_pass_equals_the_raw_call_and_only_reads(exact):
    on, off = _small_batch(True, exact=exact), _small_batch(False, exact=exact)
    for b in (on, off):
        b.run(device=0, seed=5, first_event_id=900)
    on.model_check(seed=5)
    got = on.model_fit_many(range(5))
    want = _raw_of_batch(on, 5, 900, 5)
    assert [g.status for g in got] == ["ok", "ok", "no_reads", "ok", "ok"]
    for i, (g, w) in enumerate(zip(got, want)):
        _same("event %d" % i, g, _fit_dict(w))
    assert on.model_check_ms() > 0
    # the switch changes nothing else: samples, scores, assignments, trace hashes, kernels, summaries
    assert on.last_kernels() == off.last_kernels()
    on.summarize()
    off.summarize()
    for i in range(5):
        a, c = on.result(i), off.result(i)
        assert np.array_equal(_bits(a.samples), _bits(c.samples)) and np.array_equal(_bits(a.loglik), _bits(c.loglik))
        assert np.array_equal(a.counts_hash, c.counts_hash) and np.array_equal(a.assignment, c.assignment)
        for x, y in zip(on.summary(i), off.summary(i)):
            assert np.array_equal(_bits(x), _bits(y))
    with pytest.raises(capi.InternalError):
        off.model_check(seed=5)


def test_batch_pass_after_a_further_convergent_round(orc):
    """stop = CONVERGENT_MEAN on a batch that takes a further round: the pass finishes the rounds first and reads the rows
    that the finished launch left"""
    import _convergent_cases as cc
    case = cc.case(orc, "flat_5")
    b = capi.Batch(36, model_check=True, **case.kw)
    for e in case.events:
        b.add_event(capi.Gene(e.exons, e.isoforms), e.pos, e.cig)
    b.upload(0)
    b.launch(seed=case.seed, first_event_id=case.first_id)
    b.model_check(seed=3)                  # no sync() before: finish_rounds is the pass's own
    assert b.rounds() > 1
    n = len(case.events)
    got = b.model_fit_many(range(n))
    b.sync()
    b.download()
    want = _raw_of_batch(b, n, case.first_id, 3)
    assert sum(g.status == "ok" for g in got) >= n - 2
    for i, (g, w) in enumerate(zip(got, want)):
        _same("event %d" % i, g, _fit_dict(w))


def test_it_sees_what_it_is_for():
    """Reads at the model's expectation for psi_0 = 0.5 pass; the same informative counts with the shared class cut to a
    quarter fail, and the tails name the class.  On the CPU, the restatement fed with 400 draws of the closed-form
    posterior (tests/_exact_ref.py) gives p = 0.705 and p = 0.000 (tail_ge of (1,1): 1.0): both conditions hold with room."""
    b = capi.Batch(36, iters=1100, burn=100, lag=5, chains=2, model_check=True)     # 400 kept rows
    g = capi.Gene(*GENE)
    for counts in ((55, 134, 411), (55, 134, 100)):
        b.add_event(g, *_planted(*counts))
    b.run(device=0, seed=42, first_event_id=0)
    b.model_check(seed=42)
    good, bad = b.model_fit_many([0, 1])
    assert good.ok and bad.ok and good.rows == 400 and list(good.n) == [55, 134, 411] and list(bad.n) == [55, 134, 100]
    print("conforming p", good.pvalue, "violating p", bad.pvalue, "tail_ge (1,1)", bad.ge[2] / bad.rows)
    assert good.pvalue >= 0.2
    assert bad.pvalue <= 0.01
    assert bad.ge[2] / bad.rows >= 0.99
