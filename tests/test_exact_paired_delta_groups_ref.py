"""CPU: the restatement of the quantiles of delta psi between two groups of PAIRED-END replicates
(tests/_exact_paired_delta_groups_ref.py) against mpmath and against the pairwise restatements, then
the `.miso_exact_pairs` table and the front ends' argument errors.

Against mpmath by section 20's bracketing criterion, with the project's numbers only: with H_mp the mean over the pairs of
the pairwise reference (tests/test_exact_paired_compare_ref.py mp_H),
    H_mp(q - c) - eps_H <= p <= H_mp(q + c) + eps_H,    c = 5e-5, eps_H = TOL_H = 3e-6.
The mixture's error in H is at most the largest pairwise one, the last bracket is 2 / 9^5 = 3.4e-5 < c wide and q lies inside
it.  The two cases are the issue's, under both hyperparameter pairs, at p = 0.5, 0.025, 0.975.
"""
import numpy as np
import pytest

from miso_amd import compare as compare_py
from miso_amd import miso as miso_cli
from miso_amd import run_miso, samples_utils
from _exact_delta_ref import PROBS, ROUNDS, paired_delta_quantiles, search
from _exact_paired_compare_ref import HYPERS, PairedCompare
from _exact_paired_delta_groups_ref import GROUP_CASES, PairedMixtureCdf, _TablesOnce, case_stats, comparable, group_delta
from _exact_paired_ref import PairedStats
from test_exact_paired_compare_ref import TOL_H, MpSample, mp_H

C = 5e-5
INSIDE = 1.0 - 1e-9
assert TOL_H == 3e-6 and ROUNDS == 5
COMBOS = [(name, h) for h in HYPERS for name in GROUP_CASES]
_cache = {}


@pytest.fixture(scope="module")
def post(orc):
    return _TablesOnce(PairedCompare(orc))


def result(post, name, hyper, swapped=False):
    """(the restatement's [q ..., H0], the mixture) of a case, made once"""
    key = (name, hyper, swapped)
    if key not in _cache:
        if (name, hyper, "stats") not in _cache:
            _cache[name, hyper, "stats"] = case_stats(name, hyper)
        g1, g2 = _cache[name, hyper, "stats"]
        H = PairedMixtureCdf(post, g2, g1) if swapped else PairedMixtureCdf(post, g1, g2)
        _cache[key] = (search(H, PROBS), H)
    return _cache[key]


@pytest.mark.parametrize("name,hyper", COMBOS, ids=["%s-h%g_%g" % (n, h[0], h[1]) for n, h in COMBOS])
def test_quantiles_against_mpmath(post, name, hyper):
    res, H = result(post, name, hyper)
    s1, s2 = GROUP_CASES[name]
    zs = []
    for v in res[:3]:
        zs += [min(max(float(v) - C, -INSIDE), INSIDE), min(max(float(v) + C, -INSIDE), INSIDE)]
    zs.append(0.0)
    total = [0.0] * len(zs)
    k = 0
    for a in s1:
        for b in s2:
            pair = H.pairs[k]
            want = mp_H(MpSample(a, hyper, pair.tabs[0]), MpSample(b, hyper, pair.tabs[1]), pair.a_is_2, zs)
            total = [t + w for t, w in zip(total, want)]
            k += 1
    mix = [t / k for t in total]
    for j, p in enumerate(PROBS):
        below, above = mix[2 * j], mix[2 * j + 1]
        print("%s %s p %.3f: q %.9f, H_mp(q - c) %.9f, H_mp(q + c) %.9f, slack %.3g" %
              (name, hyper, p, res[j], below, above, min(p - below, above - p)))
        assert below - TOL_H <= p <= above + TOL_H, (name, hyper, p, res[j], below, above)
    print("%s %s H0 %.9f, H_mp(0) %.9f" % (name, hyper, res[3], float(mix[6])))
    assert abs(float(res[3]) - float(mix[6])) <= TOL_H


def test_the_two_mode_case_takes_both_outcomes_of_the_choice_of_A(post):
    _, H = result(post, "two-mode", HYPERS[0])
    assert [p.a_is_2 for p in H.pairs] == [True, True, True, False, False, True]


@pytest.mark.parametrize("hyper", HYPERS, ids=lambda h: "h%g_%g" % h)
def test_one_replicate_each_is_the_pairwise_result(post, hyper):
    for name in GROUP_CASES:
        g1, g2 = case_stats(name, hyper)
        zs = (0.1, -0.1)
        got = group_delta(post, g1[:1], g2[:1], PROBS, zs)
        assert np.array_equal(got[2:6], paired_delta_quantiles(post, g1[0], g2[0], PROBS)), name
        cmp_, _ = post.compare(g1[0], g2[0], zs)
        assert np.array_equal(got[6:], cmp_[5:]) and np.array_equal(got[:2], cmp_[:2]), name


@pytest.mark.parametrize("name", list(GROUP_CASES))
def test_cdf_is_the_a_major_mean_of_the_pairwise_cdfs(post, name):
    res, H = result(post, name, HYPERS[0])
    g1, g2 = _cache[name, HYPERS[0], "stats"]
    zs = (-0.2, 0.0, 0.05, 0.3)
    cols = [post.compare(p1, p2, zs)[0][5:] for p1 in g1 for p2 in g2]
    for j, z in enumerate(zs):
        s = np.float64(0.0)
        for c in cols:
            s = s + c[j]
        assert H(np.float64(z)) == s / np.float64(len(cols)), (name, z)


@pytest.mark.parametrize("name", list(GROUP_CASES))
def test_permutation_monotone_and_swap(post, name):
    hyper = HYPERS[0]
    res, H = result(post, name, hyper)
    g1, g2 = _cache[name, hyper, "stats"]
    # a reordered sum of N <= 64 terms in [0, 1] differs by at most N (N - 1) 2^-53 < 4.5e-13
    Hp = PairedMixtureCdf(post, g1[::-1], g2[1:] + g2[:1])
    for z in (-0.5, -0.1, 0.0, 0.1, 0.5) + tuple(res[:3]):
        assert abs(Hp(np.float64(z)) - H(np.float64(z))) <= 1e-12, (name, z)
    q = dict(zip(PROBS, res[:3]))
    assert q[0.025] <= q[0.5] <= q[0.975]
    swapped, _ = result(post, name, hyper, swapped=True)
    qs = dict(zip(PROBS, swapped[:3]))
    for p, other in ((0.5, 0.5), (0.025, 0.975), (0.975, 0.025)):
        assert abs(qs[p] + q[other]) <= 2 * C, (name, p, qs[p], q[other])
    assert 0.0 <= res[3] <= 1.0 and abs((1.0 - swapped[3]) - res[3]) <= 1e-5


def test_the_issues_figures(post):
    """h = (1, 1): the pooled figures the issue quotes, and the disagreeing case's pairwise medians"""
    res, _ = result(post, "disagreeing", HYPERS[0])
    g1, g2 = _cache["disagreeing", HYPERS[0], "stats"]
    med = [paired_delta_quantiles(post, p1, g2[0], [0.5])[0] for p1 in g1]
    print("disagreeing: pooled median %.4f interval [%.4f, %.4f]; pairwise medians %s" % (res[0], res[1], res[2], med))
    assert abs(res[0] - 0.4337) < 5e-4 and abs(res[1] + 0.0657) < 5e-4 and abs(res[2] - 0.6117) < 5e-4
    assert all(abs(m - w) < 1e-3 for m, w in zip(med, (0.003, 0.529, 0.443)))
    res, _ = result(post, "two-mode", HYPERS[0])
    print("two-mode: pooled median %.4f interval [%.4f, %.4f] H0 %.5f" % (res[0], res[1], res[2], res[3]))
    assert abs(res[0] + 0.2294) < 5e-4 and abs(res[1] + 0.7850) < 5e-4 and abs(res[2] - 0.3901) < 5e-4 and abs(res[3] - 0.74115) < 5e-5


def test_comparability():
    g1, g2 = case_stats("disagreeing", HYPERS[0])
    assert comparable(g1, g2)
    assert not comparable(g1, [PairedStats(3, 4, 60000.0, 43000.0, 0.5, 1.0, [])])
    assert not comparable([PairedStats(3, 4, 0.0, 43000.0, 1.0, 1.0, [])], g2)
    # (no equality of A0, A1 between the replicates is needed: the disagreeing case has two such pairs)
    assert g1[2].base.e0 != g1[0].base.e0


def test_exact_pairs_table_round_trip(tmp_path):
    path = str(tmp_path / "s.miso_exact_pairs")
    rng = np.random.default_rng(5)
    rows = []
    for i in range(12):
        pool = rng.uniform(2.0 ** -40, 0.02, size=5)
        m = pool[rng.integers(0, 5, size=(int(rng.integers(0, 40)), 2))]       # repeated probabilities, in any order
        rows.append(("ev%d" % i, i % 4 != 0, list(rng.random(6) * 10.0 ** rng.integers(-3, 6, 6)), m))
    rows.append(("nopairs", True, [3.0, 9.0, 60000.0, 43000.0, 1.0, 1.0], np.zeros((0, 2))))
    rows.append(("third", True, [1.0, 2.0, 1.0 / 3.0, np.nextafter(140.0, 141.0), 1.0, 1.0], [(1.0 / 3.0, 0.1), (0.1, 1.0 / 3.0), (0.1, 0.1)]))
    assert compare_py.write_exact_pairs(path, rows) == len(rows)
    text = open(path).read()
    assert text.count("event_name") == 1 and text.split("\n")[0].split("\t") == compare_py.EXACT_PAIRS_FIELDS
    back = compare_py.read_exact_pairs(path)
    assert list(back) == [r[0] for r in rows]
    for name, was, st, m in rows:
        assert back[name][0] == bool(was)
        assert np.array(back[name][1]).tobytes() == np.array(st, np.float64).tobytes(), name
        assert back[name][2].shape == (len(m), 2) and back[name][2].tobytes() == np.asarray(m, np.float64).reshape(-1, 2).tobytes(), name
    third = text.split("\n")[len(rows)].split("\t")
    assert third[9] == "%r,%r" % (1.0 / 3.0, 0.1) and third[10] == "0:1,1:0,1:1"        # distinct values in order of first use
    other = str(tmp_path / "not.txt")
    open(other, "w").write("event_name\tx\n")
    with pytest.raises(ValueError, match="no .miso_exact_pairs table"):
        compare_py.read_exact_pairs(other)


# ---- the front ends' argument errors, each raised before any work ----
def _never(*a, **kw):
    raise AssertionError("work was started")


@pytest.mark.parametrize("extra,message", [
    (["--exact-paired-stats"], "--exact-paired-stats needs the paired exact-posterior mode"),
    (["--paired-end", "250", "30", "--exact-paired-stats"], "--exact-paired-stats needs the paired exact-posterior mode"),
    (["--paired-end", "250", "30", "--exact-paired", "--exact-paired-stats", "--compare", "b.bam"], "--exact-paired-stats does not go with --compare"),
], ids=["single-end", "no-mode", "compare"])
def test_miso_exact_paired_stats_argument_errors(tmp_path, monkeypatch, capsys, extra, message):
    monkeypatch.setattr(miso_cli, "compute_all_genes_psi", _never)
    monkeypatch.setattr(miso_cli, "GenesDispatcher", _never)
    with pytest.raises(SystemExit) as e:
        miso_cli.main(["--run", str(tmp_path / "index"), str(tmp_path / "a.bam"), "--read-len", "36",
                       "--output-dir", str(tmp_path / "out")] + extra)
    assert e.value.code == 2
    assert message in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


def test_run_miso_exact_pairs_file_argument_errors(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(run_miso, "compute_gene_psi", _never)
    monkeypatch.setattr(run_miso, "compare_gene_psi", _never)
    genes = str(tmp_path / "genes.txt")
    base = ["--compute-genes-from-file", genes, "a.bam", str(tmp_path / "o"), "--read-len", "36"]
    assert run_miso.main(base + ["--exact-pairs-file", "f"]) == 1                                           # single-end
    assert run_miso.main(base + ["--paired-end", "250", "30", "--exact-pairs-file", "f"]) == 1              # not the mode
    assert run_miso.main(["--compare-genes-from-file", genes, "a.bam", "b.bam", str(tmp_path / "o1"), str(tmp_path / "o2"),
                          str(tmp_path / "bf"), "--read-len", "36",
                          "--paired-end", "250", "30", "--exact-paired", "--exact-pairs-file", "f"]) == 1   # a comparison
    assert capsys.readouterr().out.count("--exact-pairs-file goes with") == 3


def _group_dirs(tmp_path, with_table):
    dirs = []
    for name in ("a", "b", "c"):
        d = tmp_path / name
        (d / "summary").mkdir(parents=True)
        if name in with_table:
            compare_py.write_exact_pairs(str(d / "summary" / (name + ".miso_exact_pairs")), [])
        dirs.append(str(d))
    return dirs


@pytest.mark.parametrize("argv,message", [
    (["--exact-paired-delta-posterior"], "--exact-paired-delta-posterior goes with --compare-groups"),
    (["--compare-samples", "d1", "d2", "o", "--exact-paired-delta-posterior"], "--exact-paired-delta-posterior goes with --compare-groups"),
    (["--compare-groups", "d1", "d2", "o", "--exact-paired-delta-posterior", "--exact-delta-posterior"], "one of --exact-delta-posterior"),
    (["--compare-groups", "d1", "d2", "o", "--exact-paired-delta-posterior", "--delta-psi-thresholds", "1.0"], "outside"),
], ids=["alone", "with-samples", "both-exact", "bad-threshold"])
def test_group_front_end_argument_errors(monkeypatch, capsys, argv, message):
    for name in ("output_samples_comparison", "output_group_comparisons", "output_group_exact_delta", "output_group_exact_paired_delta"):
        monkeypatch.setattr(samples_utils, name, _never)
    with pytest.raises(SystemExit) as e:
        samples_utils.main(argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_missing_table_names_its_directory_before_any_work(tmp_path, monkeypatch, capsys):
    for name in ("output_group_comparisons", "output_group_exact_delta", "output_group_exact_paired_delta"):
        monkeypatch.setattr(samples_utils, name, _never)
    a, b, c = _group_dirs(tmp_path, with_table=("a", "c"))
    with pytest.raises(SystemExit) as e:
        samples_utils.main(["--compare-groups", a + "," + b, c, str(tmp_path / "o"), "--exact-paired-delta-posterior"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and b in err and ".miso_exact_pairs" in err and a + " has no" not in err
    assert not (tmp_path / "o").exists()
    nine = ",".join(str(tmp_path / ("r%d" % i)) for i in range(9))
    with pytest.raises(SystemExit):
        samples_utils.main(["--compare-groups", nine, c, str(tmp_path / "o"), "--exact-paired-delta-posterior"])
    assert "between 1 and 8 replicates" in capsys.readouterr().err


def test_group_front_end_pools_by_presence_pattern(tmp_path, monkeypatch, capsys):
    """the host side of the group front end with the device call replaced by a stand-in of its shape: which replicates an
    event is pooled over, one call per presence pattern, NA for the rest"""
    a, b, c = _group_dirs(tmp_path, with_table=())
    st = [1.0, 2.0, 100.0, 60.0, 1.0, 1.0]
    m = [(0.01, 0.002), (0.003, 0.01)]
    tables = {a: [("e1", True, st, m), ("e2", True, st, []), ("e3", False, st, []), ("e4", True, st, m)],
              b: [("e1", True, st, m), ("e3", True, st, m), ("e4", True, st, [])],
              c: [("e1", True, st, m), ("e2", True, st, m), ("e4", True, st, m), ("e5", True, st, m)]}
    for d, rows in tables.items():
        compare_py.write_exact_pairs(samples_utils.exact_pairs_path(d), rows)
    calls = []

    class Res:
        def row(self, j):
            return 0.5, 0.25, np.array([0.25, 0.1, 0.4]), 0.125, np.array([0.9, 0.2, 0.95, 0.1])

    def fake(g1, g2, probs, z):
        calls.append((len(g1), len(g2), len(g1[0][0]), [len(p) for p in g1[0][1]], tuple(probs), tuple(z)))
        return Res()
    monkeypatch.setattr(samples_utils.capi, "exact_paired_delta_groups", fake)
    out, n = samples_utils.output_group_exact_paired_delta([a, b], [c], str(tmp_path / "o"), group_names=("ctl", "kd"))
    assert out == str(tmp_path / "o" / "ctl_vs_kd" / "delta-psi" / "ctl_vs_kd.miso_group_dpsi_exact") and n == 5
    rows = [ln.split("\t") for ln in open(out).read().splitlines()]
    got = {r[0]: dict(zip(rows[0], r)) for r in rows[1:]}
    assert [(got[e]["group1_replicates"], got[e]["group2_replicates"], got[e]["exact"]) for e in ("e1", "e2", "e3", "e4", "e5")] == \
        [("2", "1", "1"), ("1", "1", "1"), ("1", "0", "0"), ("2", "1", "1"), ("0", "1", "0")]
    assert got["e1"]["delta_psi_median"] == "0.2500" and got["e3"]["delta_psi_median"] == got["e5"]["delta_psi_median"] == "NA"
    # e1 and e4 share a pattern (both replicates of group 1), e2 has its own; e3 and e5 never reach the device
    assert sorted(c[:4] for c in calls) == [(1, 1, 1, [0]), (2, 1, 2, [2, 2])]
    assert all(c[4] == (0.5, 0.025, 0.975) and c[5] == (0.1, -0.1, 0.2, -0.2) for c in calls)
    assert "2 event(s) have no" in capsys.readouterr().out
