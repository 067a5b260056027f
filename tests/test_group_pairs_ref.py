"""CPU: the pooled all-pairs comparison of two groups of replicates as tests/_group_pairs_ref.py restates it
-- tests/_pairs_ref.py on the concatenated columns --, what follows from the definition, the `.miso_group_dpsi` writer and
the argument errors of `samples_utils --compare-groups --delta-posterior`.  The GPU tests
(tests/test_gpu_compare_pairs_groups.py) hold the kernel to the restatement bit for bit."""
import itertools
import time

import numpy as np
import pytest

import _group_pairs_ref as GR
import _pairs_ref as PR
from miso_amd import compare, samples_utils

SHAPES = [(1, 1, 2), (2, 3, 3), (3, 3, 64), (2, 2, 255), (3, 2, 257)]
TAUS = (0.05, 0.2, 0.25, 0.5)


@pytest.mark.parametrize("kind", PR.KINDS)
@pytest.mark.parametrize("n1,n2,S", SHAPES)
def test_bisect_is_brute(kind, n1, n2, S):
    g1, g2 = GR.group_columns(kind, n1, n2, S)
    for level in (0.5, 0.95):
        x, y = GR.brute(g1, g2, level, TAUS), GR.bisect(g1, g2, level, TAUS)
        assert PR.same(x, y), (x, y)
        assert x[7] == n1 * S * n2 * S


@pytest.mark.parametrize("kind", PR.KINDS)
@pytest.mark.parametrize("n1,n2,S", SHAPES[1:])
def test_pooled_counts_are_the_sums_of_the_pairwise_ones(kind, n1, n2, S):
    g1, g2 = GR.group_columns(kind, n1, n2, S, seed=3)
    pooled = GR.bisect(g1, g2, 0.95, TAUS)
    pairs = [PR.bisect(a, b, 0.95, TAUS) for a in g1 for b in g2]
    assert pooled[3] == sum(p[3] for p in pairs) and pooled[4] == sum(p[4] for p in pairs)
    assert pooled[5] == [sum(p[5][j] for p in pairs) for j in range(len(TAUS))]
    assert pooled[7] == sum(p[7] for p in pairs)


def test_the_order_of_the_replicates_does_not_matter():
    g1, g2 = GR.group_columns("uniform", 3, 2, 65, seed=1)
    want = GR.brute(g1, g2, 0.9, TAUS)
    for p1 in itertools.permutations(range(3)):
        for p2 in itertools.permutations(range(2)):
            assert PR.same(GR.brute([g1[i] for i in p1], [g2[j] for j in p2], 0.9, TAUS), want)


def test_one_against_one_is_the_pairwise_comparison():
    a, b = PR.columns("ties", 130, 130)
    assert PR.same(GR.bisect([a], [b], 0.95, TAUS), PR.bisect(a, b, 0.95, TAUS))


def test_replicates_that_disagree():
    """One group-1 replicate near psi = 0.2, two near 0.8, against one group-2 replicate near 0.2: a third of the pooled
    differences lies around 0, two thirds around 0.6.  The pooled median is the lower quartile of the upper mode, about 0.56
    (with 2 700 draws a replicate: 0.5648, pairwise medians -0.0007, 0.6019, 0.6041, their mean 0.4018, pooled interval
    [-0.0808, 0.6969]) -- not the mean of the pairwise medians; the interval spans both modes, which no pairwise one does."""
    g1, g2 = GR.disagreeing(200)
    med, lo, hi = GR.brute(g1, g2, 0.95)[:3]
    pair = [PR.brute(a, g2[0], 0.95) for a in g1]
    mean_of_medians = sum(p[0] for p in pair) / 3
    assert abs(pair[0][0]) < 0.02 and abs(pair[1][0] - 0.6) < 0.02 and abs(pair[2][0] - 0.6) < 0.02
    assert abs(mean_of_medians - 0.4) < 0.02
    assert 0.54 < med < 0.59 and med - mean_of_medians > 0.12
    assert -0.12 < lo < -0.05 and 0.66 < hi < 0.73
    assert all(p[2] - p[1] < 0.5 * (hi - lo) for p in pair)


def test_the_limit():
    n1, n2, S = 2, 2, 8192
    M = (n1 * S) * (n2 * S)
    assert M == 268_435_456 and PR.ranks(M, 0.95) == (134_217_727, 6_710_885, 261_724_569)
    assert max(PR.ranks(M, 0.95)) < 2 ** 32 and M < 2 ** 32
    rng = np.random.default_rng(11)
    g1, g2 = [rng.random(S) for _ in range(n1)], [np.round(rng.beta(4, 4, S), 4) for _ in range(n2)]
    t0 = time.perf_counter()
    x = GR.bisect(g1, g2, 0.95, (0.2,))
    print("the restatement at the limit: %.2f s" % (time.perf_counter() - t0))
    assert x[6] and x[7] == M and x[3] + x[4] <= M and x[1] < x[0] < x[2]
    pairs = [PR.bisect(a, b, 0.95, (0.2,)) for a in g1 for b in g2]
    assert x[3] == sum(p[3] for p in pairs) and x[5] == [sum(p[5][0] for p in pairs)]


def test_not_finite():
    g1, g2 = GR.group_columns("uniform", 2, 3, 9)
    g2[1][4] = np.nan
    for f in (GR.brute, GR.bisect):
        x = f(g1, g2, 0.9, (0.2,))
        assert all(np.isnan(v) for v in x[:3]) and x[3:] == (0, 0, [0], False, 18 * 27)


def test_refusals():
    assert GR.refusal(2, 2, 8192, 0.95, (0.1, 0.2, 0.3, 0.4)) is None
    assert GR.refusal(6, 6, 2700, 0.95, ()) is None and GR.refusal(3, 3, 5000, 0.95, ()) is None
    assert GR.refusal(3, 2, 8192, 0.95, ()).startswith("group 1: Too many samples")
    assert GR.refusal(2, 3, 8192, 0.95, ()).startswith("group 2: Too many samples")
    assert GR.refusal(1, 1, 16385, 0.95, ()).startswith("group 1")
    assert "number of delta psi thresholds" in GR.refusal(1, 1, 10, 0.95, (0.1,) * 5)
    assert "threshold" in GR.refusal(1, 1, 10, 0.95, (1.0,)) and "confidence" in GR.refusal(1, 1, 10, 0.0, ())


# ---- the writer
HDR = {"isoforms": "'A_B','A'", "chrom": "chr7", "strand": "+", "mRNA_starts": "100,100", "mRNA_ends": "900,900"}


def _pairs(K, n_tau, M=400, finite=None):
    med = np.array([0.25, -0.125, 0.0625][:K] + [0.0] * max(0, K - 3))
    fin = np.ones(K, bool) if finite is None else np.asarray(finite)
    ge = np.array([[M // (2 + k + j) for j in range(n_tau)] for k in range(K)], np.int64).reshape(K, n_tau)
    return med, med - 0.5, med + 0.5, np.arange(K) * 10 + 100, np.arange(K) * 10 + 200, ge, fin, M


def test_group_dpsi_table(tmp_path):
    thr = (0.1, 0.25)
    two1 = [np.array([0.8, 0.2]), np.array([0.7, 0.3]), np.array([0.75, 0.25])]
    two2 = [np.array([0.2, 0.8])]
    three1 = [np.array([0.5, 0.3, 0.2]), np.array([0.25, 0.3, 0.45])]
    three2 = [np.array([0.25, 0.25, 0.5]), np.array([0.5, 0.25, 0.25])]
    rows = [("ev2", 3, 1, two1, two2, _pairs(2, 2), HDR),
            ("ev3", 2, 2, three1, three2, _pairs(3, 2), HDR),
            ("evbad", 2, 2, three1, three2, _pairs(3, 2, finite=[True, False, True]), HDR),
            ("evna", 1, 2, None, None, None, {"isoforms": "'X'"})]
    out = tmp_path / "g.miso_group_dpsi"
    assert compare.write_group_dpsi(str(out), rows, thr) == 4
    lines = [ln.split("\t") for ln in out.read_text().splitlines()]
    assert lines[0] == (["event_name", "group1_replicates", "group2_replicates", "group1_posterior_mean", "group2_posterior_mean",
                         "diff", "delta_psi_median", "delta_psi_ci_low", "delta_psi_ci_high", "prob_diff_gt_0", "prob_diff_lt_0",
                         "prob_abs_diff_ge_0.1", "prob_abs_diff_ge_0.25", "isoforms", "chrom", "strand", "mRNA_starts", "mRNA_ends"])
    assert all(len(ln) == len(lines[0]) for ln in lines)
    m1 = ((0.8 + 0.7) + 0.75) / 3
    assert lines[1] == (["ev2", "3", "1", "%.4f" % m1, "0.2000", "%.4f" % (m1 - 0.2), "0.2500", "-0.2500", "0.7500", "0.2500",
                         "0.5000", "0.5000", "0.3325"] + [HDR[k] for k in ("isoforms", "chrom", "strand", "mRNA_starts", "mRNA_ends")])
    assert lines[1][6:13] == compare.dpsi_fields(_pairs(2, 2), 2)
    assert lines[2][:6] == ["ev3", "2", "2", "0.3750,0.3000,0.3250", "0.3750,0.2500,0.3750", "0.0000,0.0500,-0.0500"]
    assert lines[2][6:13] == compare.dpsi_fields(_pairs(3, 2), 2) and lines[2][6] == "0.2500,-0.1250,0.0625"
    assert lines[3][6] == "0.2500,NA,0.0625" and lines[3][11] == "0.5000,NA,0.2500"
    assert lines[4] == ["evna", "1", "2"] + ["NA"] * 10 + ["'X'"] + ["NA"] * 4
    with pytest.raises(ValueError):
        compare.write_group_dpsi(str(out), rows, (0.1, 1.0))


def test_group_mean_is_summed_in_replicate_order():
    ms = [np.array([0.1]), np.array([0.7]), np.array([0.2])]
    assert compare.group_mean(ms) == [((0.1 + 0.7) + 0.2) / 3]
    assert compare.group_mean(ms[:1]) == [0.1]


# ---- the command line
def _never(*a, **kw):
    raise AssertionError("work was started")


@pytest.mark.parametrize("argv,message", [
    (["--delta-posterior"], "needs --compare-samples or --compare-groups"),
    (["--summarize-samples", "d", "o", "--delta-posterior"], "needs --compare-samples or --compare-groups"),
    (["--group-names", "a", "b"], "--group-names goes with --compare-groups --delta-posterior"),
    (["--compare-groups", "d1,d2", "d3", "o", "--group-names", "a", "b"], "--group-names goes with --compare-groups --delta-posterior"),
    (["--compare-samples", "d1", "d2", "o", "--delta-posterior", "--group-names", "a", "b"], "--group-names goes with"),
    (["--compare-groups", "d1,d2", "d3", "o", "--delta-posterior", "--delta-psi-thresholds", "0.1", "1.0"], "outside"),
    (["--compare-groups", "d1,d2", "d3", "o", "--delta-posterior", "--delta-psi-thresholds", "0.0"], "outside"),
    (["--compare-groups", "d1,d2", "d3", "o", "--delta-psi-thresholds", "0.1"], "goes with --delta-posterior"),
], ids=["alone", "summarize", "names-alone", "names-without-delta", "names-with-samples", "threshold-1", "threshold-0",
        "thresholds-alone"])
def test_argument_errors_before_any_work(monkeypatch, capsys, argv, message):
    for name in ("summarize_sampler_results", "output_samples_comparison", "output_group_comparisons"):
        monkeypatch.setattr(samples_utils, name, _never)
    with pytest.raises(SystemExit) as e:
        samples_utils.main(argv)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_main_hands_thresholds_and_names_on(monkeypatch):
    seen = {}
    monkeypatch.setattr(samples_utils, "output_group_comparisons", lambda *a, **kw: seen.update(kw) or [])
    samples_utils.main(["--compare-groups", "d1,d2", "d3", "o"])
    assert seen["delta_thresholds"] is None and seen["group_names"] is None
    samples_utils.main(["--compare-groups", "d1,d2", "d3", "o", "--delta-posterior"])
    assert tuple(seen["delta_thresholds"]) == (0.1, 0.2) and seen["group_names"] is None
    samples_utils.main(["--compare-groups", "d1,d2", "d3", "o", "--delta-posterior", "--delta-psi-thresholds", "0.3", "--group-names",
                        "ctl", "kd"])
    assert list(seen["delta_thresholds"]) == [0.3] and list(seen["group_names"]) == ["ctl", "kd"]
    assert samples_utils.DEFAULT_GROUP_NAMES == ("group1", "group2")
