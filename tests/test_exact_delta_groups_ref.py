"""CPU: the restatement of the quantiles of delta psi between two groups of replicates (tests/_exact_delta_groups_ref.py;
DESIGN.md section 20a) against mpmath and against the pairwise restatements, then the writers, the `.miso_exact_stats` table
and the front ends' argument errors.

Against mpmath by section 20's bracketing criterion, with the project's numbers only: with H_mp the mean over the pairs of
the pairwise reference (tests/test_exact_compare_ref.py mp_H),
    H_mp(q - c) - eps_H <= p <= H_mp(q + c) + eps_H,    c = 5e-5, eps_H = 5e-6.
The mixture's error in H is at most the largest pairwise one, the last bracket is 2 / 9^5 = 3.4e-5 < c wide and q lies inside
it.  The three cases are the issue's, under both hyperparameter pairs, at p = 0.5, 0.025, 0.975.
"""
import numpy as np
import pytest

from miso_amd import compare as compare_py
from miso_amd import miso as miso_cli
from miso_amd import run_miso, samples_utils
from _exact_compare_ref import HYPERS, PAIRS, compare, pair_rows
from _exact_delta_groups_ref import GROUP_CASES, MixtureCdf, case_rows, comparable, group_delta
from _exact_delta_ref import PROBS, ROUNDS, delta_quantiles, search
from _exact_ref import Posterior
from test_exact_compare_ref import H_TOL, mp_H

C = 5e-5
INSIDE = 1.0 - 1e-9
assert H_TOL == 5e-6 and ROUNDS == 5
COMBOS = [(name, h) for h in HYPERS for name in GROUP_CASES]
_cache, _pairs = {}, {}


@pytest.fixture(scope="module")
def post(orc):
    return Posterior(orc)


def result(post, name, hyper, swapped=False):
    """(the restatement's [q ..., H0], the mixture) of a case, made once"""
    key = (name, hyper, swapped)
    if key not in _cache:
        g1, g2 = case_rows(name, hyper)
        H = MixtureCdf(post, g2, g1, _pairs) if swapped else MixtureCdf(post, g1, g2, _pairs)
        _cache[key] = (search(H, PROBS), H)
    return _cache[key]


@pytest.mark.parametrize("name,hyper", COMBOS, ids=["%s-h%g_%g" % (n, h[0], h[1]) for n, h in COMBOS])
def test_quantiles_against_mpmath(post, name, hyper):
    res, H = result(post, name, hyper)
    g1, g2 = case_rows(name, hyper)
    zs = []
    for v in res[:3]:
        zs += [min(max(float(v) - C, -INSIDE), INSIDE), min(max(float(v) + C, -INSIDE), INSIDE)]
    total = [0.0] * len(zs)
    k = 0
    for r1 in g1:
        for r2 in g2:
            want = mp_H((r1, r2), list(H.pairs[k].tabs), zs)
            total = [t + w for t, w in zip(total, want)]
            k += 1
    mix = [t / k for t in total]
    for j, p in enumerate(PROBS):
        below, above = mix[2 * j], mix[2 * j + 1]
        print("%s %s p %.3f: q %.9f, H_mp(q - c) %.9f, H_mp(q + c) %.9f, slack %.3g" %
              (name, hyper, p, res[j], below, above, min(p - below, above - p)))
        assert below - H_TOL <= p <= above + H_TOL, (name, hyper, p, res[j], below, above)


@pytest.mark.parametrize("hyper", HYPERS, ids=lambda h: "h%g_%g" % h)
def test_one_replicate_each_is_the_pairwise_result(post, hyper):
    for pair in PAIRS:
        r1, r2 = pair_rows(pair, hyper)
        zs = (0.1, -0.1)
        got = group_delta(post, [r1], [r2], PROBS, zs)
        assert np.array_equal(got[2:6], delta_quantiles(post, r1, r2, PROBS)), pair
        cmp_ = compare(post, r1, r2, zs)
        assert np.array_equal(got[6:], cmp_[5:]) and np.array_equal(got[:2], cmp_[:2]), pair


@pytest.mark.parametrize("name", list(GROUP_CASES))
def test_cdf_is_the_a_major_mean_of_the_pairwise_cdfs(post, name):
    g1, g2 = case_rows(name, HYPERS[0])
    _, H = result(post, name, HYPERS[0])
    zs = (-0.2, 0.0, 0.05, 0.3)
    cols = [compare(post, r1, r2, zs)[5:] for r1 in g1 for r2 in g2]
    for j, z in enumerate(zs):
        s = np.float64(0.0)
        for c in cols:
            s = s + c[j]
        assert H(np.float64(z)) == s / np.float64(len(cols)), (name, z)


@pytest.mark.parametrize("name", list(GROUP_CASES))
def test_permutation_monotone_and_swap(post, name):
    hyper = HYPERS[0]
    res, H = result(post, name, hyper)
    g1, g2 = case_rows(name, hyper)
    # a reordered sum of N <= 64 terms in [0, 1] differs by at most N (N - 1) 2^-53 < 4.5e-13
    Hp = MixtureCdf(post, g1[::-1], g2[1:] + g2[:1], _pairs)
    for z in (-0.5, -0.1, 0.0, 0.1, 0.5) + tuple(res[:3]):
        assert abs(Hp(np.float64(z)) - H(np.float64(z))) <= 1e-12, (name, z)
    q = dict(zip(PROBS, res[:3]))
    assert q[0.025] <= q[0.5] <= q[0.975]
    swapped, _ = result(post, name, hyper, swapped=True)
    qs = dict(zip(PROBS, swapped[:3]))
    for p, other in ((0.5, 0.5), (0.025, 0.975), (0.975, 0.025)):
        assert abs(qs[p] + q[other]) <= 2 * C, (name, p, qs[p], q[other])
    assert 0.0 <= res[3] <= 1.0 and abs((1.0 - swapped[3]) - res[3]) <= 1e-5


def test_pooled_median_is_no_function_of_the_pairwise_medians(post):
    """the disagreeing case: the pooled median lies far from the mean of the pairwise medians, and the pooled interval
    contains both modes"""
    hyper = HYPERS[0]
    res, _ = result(post, "disagreeing", hyper)
    g1, g2 = case_rows("disagreeing", hyper)
    med = [delta_quantiles(post, r1, g2[0], [0.5])[0] for r1 in g1]
    mean = float(np.mean(med))
    print("pooled median %.4f interval [%.4f, %.4f]; pairwise medians %s, their mean %.4f" % (res[0], res[1], res[2], med, mean))
    assert abs(res[0] - 0.5356) < 5e-4 and abs(res[1] + 0.0872) < 5e-4 and abs(res[2] - 0.6770) < 5e-4
    assert not (mean - 0.05 <= res[0] <= mean + 0.05)
    assert res[1] <= min(med) and max(med) <= res[2]


def test_comparability():
    g1, g2 = case_rows("disagreeing", HYPERS[0])
    assert comparable(g1, g2)
    low = [list(r) for r in g1]
    low[1][5] = 0.5
    assert not comparable(low, g2)
    ulp = [list(r) for r in g2]
    ulp[0][3] = np.nextafter(ulp[0][3], np.inf)
    assert not comparable(g1, ulp)


def test_writer(tmp_path):
    path = str(tmp_path / "A_vs_B.miso_group_dpsi_exact")
    header = {"isoforms": "'a','b'", "chrom": "chr1", "strand": "+", "mRNA_starts": "1,1", "mRNA_ends": "9,8"}
    cdf = np.array([0.9, 0.2, 0.95, 0.1])       # H at (0.1, -0.1, 0.2, -0.2)
    rows = [("ev1", 3, 2, (0.61234, 0.2, np.array([0.41236, -0.05, 0.7]), 0.125, cdf), header),
            ("ev2", 3, 0, None, {})]
    assert compare_py.write_group_dpsi_exact(path, rows, [0.1, 0.2]) == 2
    lines = open(path).read().split("\n")
    head = lines[0].split("\t")
    assert head == compare_py.group_dpsi_header_fields([0.1, 0.2])[:6] + ["exact"] + compare_py.group_dpsi_header_fields([0.1, 0.2])[6:]
    f1 = dict(zip(head, lines[1].split("\t")))
    assert f1["group1_replicates"] == "3" and f1["group2_replicates"] == "2" and f1["exact"] == "1"
    assert (f1["group1_posterior_mean"], f1["group2_posterior_mean"], f1["diff"]) == ("0.6123", "0.2000", "0.4123")
    assert (f1["delta_psi_median"], f1["delta_psi_ci_low"], f1["delta_psi_ci_high"]) == ("0.4124", "-0.0500", "0.7000")
    assert (f1["prob_diff_gt_0"], f1["prob_diff_lt_0"]) == ("0.8750", "0.1250")
    assert (f1["prob_abs_diff_ge_0.1"], f1["prob_abs_diff_ge_0.2"]) == ("0.3000", "0.1500")
    assert f1["chrom"] == "chr1" and f1["mRNA_ends"] == "9,8"
    f2 = dict(zip(head, lines[2].split("\t")))
    assert f2["exact"] == "0" and f2["group2_replicates"] == "0" and f2["delta_psi_median"] == "NA" and f2["chrom"] == "NA"
    assert lines[3] == "" and len(lines) == 4
    with pytest.raises(ValueError):
        compare_py.write_group_dpsi_exact(path, rows, [])


def test_exact_stats_table_round_trip(tmp_path):
    path = str(tmp_path / "s.miso_exact_stats")
    rng = np.random.default_rng(3)
    rows = [("ev%d" % i, i % 3 != 0, list(rng.random(7) * 10.0 ** rng.integers(-3, 6, 7))) for i in range(20)]
    rows.append(("third", True, [1.0, 2.0, 3.0, 1.0 / 3.0, np.nextafter(140.0, 141.0), 1.0, 1.0]))
    assert compare_py.write_exact_stats(path, rows) == 21
    back = compare_py.read_exact_stats(path)
    assert list(back) == [r[0] for r in rows]
    for name, was, st in rows:
        assert back[name][0] == bool(was)
        assert np.array(back[name][1]).tobytes() == np.array(st, np.float64).tobytes(), name
    other = str(tmp_path / "not.txt")
    open(other, "w").write("event_name\tx\n")
    with pytest.raises(ValueError, match="no .miso_exact_stats table"):
        compare_py.read_exact_stats(other)


# ---- the front ends' argument errors, each raised before any work ----
def _never(*a, **kw):
    raise AssertionError("work was started")


@pytest.mark.parametrize("extra,message", [
    (["--exact-stats"], "--exact-stats needs the exact-posterior mode"),
    (["--compare", "b.bam", "--exact-stats"], "--exact-stats needs the exact-posterior mode"),
    (["--exact", "--exact-stats", "--paired-end", "250", "30"], "single-end"),
], ids=["no-exact", "no-exact-compare", "paired-end"])
def test_miso_exact_stats_argument_errors(tmp_path, monkeypatch, capsys, extra, message):
    monkeypatch.setattr(miso_cli, "compute_all_genes_psi", _never)
    monkeypatch.setattr(miso_cli, "GenesDispatcher", _never)
    with pytest.raises(SystemExit) as e:
        miso_cli.main(["--run", str(tmp_path / "index"), str(tmp_path / "a.bam"), "--read-len", "36",
                       "--output-dir", str(tmp_path / "out")] + extra)
    assert e.value.code == 2
    assert message in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


def test_run_miso_exact_stats_argument_errors(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(run_miso, "compute_gene_psi", _never)
    monkeypatch.setattr(run_miso, "compare_gene_psi", _never)
    genes = str(tmp_path / "genes.txt")
    base = ["--compute-genes-from-file", genes, "a.bam", str(tmp_path / "o"), "--read-len", "36"]
    assert run_miso.main(base + ["--exact-stats-file", "f"]) == 1                                   # not the exact mode
    assert run_miso.main(base + ["--exact", "--exact-stats-file", "f", "--paired-end", "250", "30"]) == 1
    assert run_miso.main(base + ["--exact", "--exact-stats-files", "f", "g"]) == 1                   # the comparison's flag
    out = capsys.readouterr().out
    assert out.count("--exact-stats-file goes with") == 2 and out.count("--exact-stats-files goes with") == 1


def _group_dirs(tmp_path, with_table):
    dirs = []
    for name in ("a", "b", "c"):
        d = tmp_path / name
        (d / "summary").mkdir(parents=True)
        if name in with_table:
            compare_py.write_exact_stats(str(d / "summary" / (name + ".miso_exact_stats")), [])
        dirs.append(str(d))
    return dirs


@pytest.mark.parametrize("argv,message", [
    (["--exact-delta-posterior"], "--exact-delta-posterior goes with --compare-groups"),
    (["--compare-samples", "d1", "d2", "o", "--exact-delta-posterior"], "--exact-delta-posterior goes with --compare-groups"),
    (["--compare-groups", "d1,d2", "d3", "o", "--group-names", "a", "b"], "--group-names goes with --compare-groups --delta-posterior"),
    (["--compare-groups", "d1", "d2", "o", "--delta-psi-thresholds", "0.3"], "--delta-psi-thresholds goes with"),
    (["--compare-groups", "d1", "d2", "o", "--exact-delta-posterior", "--delta-psi-thresholds", "1.0"], "outside"),
], ids=["alone", "with-samples", "names-alone", "thresholds-alone", "bad-threshold"])
def test_group_front_end_argument_errors(monkeypatch, capsys, argv, message):
    for name in ("output_samples_comparison", "output_group_comparisons", "output_group_exact_delta"):
        monkeypatch.setattr(samples_utils, name, _never)
    with pytest.raises(SystemExit) as e:
        samples_utils.main(argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_missing_table_names_its_directory_before_any_work(tmp_path, monkeypatch, capsys):
    for name in ("output_group_comparisons", "output_group_exact_delta"):
        monkeypatch.setattr(samples_utils, name, _never)
    a, b, c = _group_dirs(tmp_path, with_table=("a", "c"))
    with pytest.raises(SystemExit) as e:
        samples_utils.main(["--compare-groups", a + "," + b, c, str(tmp_path / "o"), "--exact-delta-posterior"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and b in err and ".miso_exact_stats" in err and a + " has no" not in err
    assert not (tmp_path / "o").exists()
    nine = ",".join(str(tmp_path / ("r%d" % i)) for i in range(9))
    with pytest.raises(SystemExit):
        samples_utils.main(["--compare-groups", nine, c, str(tmp_path / "o"), "--exact-delta-posterior"])
    assert "between 1 and 8 replicates" in capsys.readouterr().err


@pytest.mark.parametrize("flag", ["--delta-posterior", "--exact-delta-posterior"])
def test_group_names_go_with_either_flag(tmp_path, monkeypatch, flag):
    seen = {}
    monkeypatch.setattr(samples_utils, "output_group_comparisons", lambda *a, **kw: seen.update(kw) or [])
    monkeypatch.setattr(samples_utils, "output_group_exact_delta", lambda *a, **kw: seen.update(exact=kw) or ("f", 0))
    a, b, c = _group_dirs(tmp_path, with_table=("a", "b", "c"))
    samples_utils.main(["--compare-groups", a + "," + b, c, str(tmp_path / "o"), flag, "--group-names", "ctl", "kd",
                        "--delta-psi-thresholds", "0.3"])
    assert list(seen["group_names"]) == ["ctl", "kd"]
    if flag == "--exact-delta-posterior":
        assert list(seen["exact"]["group_names"]) == ["ctl", "kd"] and list(seen["exact"]["delta_thresholds"]) == [0.3]
        assert seen["delta_thresholds"] is None        # the sampled tables are not asked for
    else:
        assert "exact" not in seen and list(seen["delta_thresholds"]) == [0.3]


def test_group_front_end_pools_by_presence_pattern(tmp_path, monkeypatch, capsys):
    """the host side of the group front end with the device call replaced by the restatement's shape: which replicates an
    event is pooled over, one call per presence pattern, NA and one notice per cause"""
    a, b, c = _group_dirs(tmp_path, with_table=())
    st = [1.0, 2.0, 3.0, 100.0, 60.0, 1.0, 1.0]
    other = st[:3] + [101.0] + st[4:]
    tables = {a: [("e1", True, st), ("e2", True, st), ("e3", False, st), ("e4", True, st)],
              b: [("e1", True, st), ("e3", True, st), ("e4", True, other)],
              c: [("e1", True, st), ("e2", True, st), ("e4", True, st), ("e5", True, st)]}
    for d, rows in tables.items():
        compare_py.write_exact_stats(samples_utils.exact_stats_path(d), rows)
    calls = []

    class Res:
        def __init__(self, s1, s2):
            self.ok = [all(r[3:5] == s1[j][0][3:5] for r in s1[j] + s2[j]) for j in range(len(s1))]

        def row(self, j):
            return (0.5, 0.25, np.array([0.25, 0.1, 0.4]), 0.125, np.array([0.9, 0.2, 0.95, 0.1])) if self.ok[j] else None

    def fake(s1, s2, probs, z):
        calls.append((np.array(s1).shape, np.array(s2).shape, tuple(probs), tuple(z)))
        return Res(s1, s2)
    monkeypatch.setattr(samples_utils.capi, "exact_delta_groups", fake)
    out, n = samples_utils.output_group_exact_delta([a, b], [c], str(tmp_path / "o"), group_names=("ctl", "kd"))
    assert out == str(tmp_path / "o" / "ctl_vs_kd" / "delta-psi" / "ctl_vs_kd.miso_group_dpsi_exact") and n == 5
    rows = [ln.split("\t") for ln in open(out).read().splitlines()]
    got = {r[0]: dict(zip(rows[0], r)) for r in rows[1:]}
    assert [(got[e]["group1_replicates"], got[e]["group2_replicates"], got[e]["exact"]) for e in ("e1", "e2", "e3", "e4", "e5")] == \
        [("2", "1", "1"), ("1", "1", "1"), ("1", "0", "0"), ("2", "1", "0"), ("0", "1", "0")]
    assert got["e1"]["delta_psi_median"] == "0.2500" and got["e3"]["delta_psi_median"] == got["e4"]["delta_psi_median"] == "NA"
    # e1 and e4 share a pattern (both replicates of group 1), e2 has its own; e3 and e5 never reach the device
    assert sorted(c[0] for c in calls) == [(1, 1, 7), (2, 2, 7)]
    assert all(c[2] == (0.5, 0.025, 0.975) and c[3] == (0.1, -0.1, 0.2, -0.2) for c in calls)
    text = capsys.readouterr().out
    assert text.count("no replicate with an exact posterior") == 1 and "2 event(s) have no" in text
    assert text.count("differ in effective lengths") == 1 and "1 event(s) differ" in text
