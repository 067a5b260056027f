"""CPU: the front ends of the all-pairs comparison: the `.miso_dpsi` writer (miso_amd/compare.py), the
argument errors of the three command lines, and filter_events reading the table by column name."""
import numpy as np
import pytest

import _pairs_ref as PR
from miso_amd import compare, filter_events
from miso_amd import miso as miso_cli
from miso_amd import run_miso, samples_utils


def _pairs(K, n_tau, seed=0, not_finite=()):
    """a result tuple as capi.Batch.pair_comparison returns it, from the restatement on random columns"""
    rng = np.random.default_rng([seed, K])
    taus = (0.1, 0.2, 0.25, 0.5)[:n_tau]
    cols = []
    for k in range(K):
        a, b = np.round(rng.random(30), 4), np.round(rng.random(20), 4)
        if k in not_finite:
            a[3] = np.nan
        cols.append(PR.brute(a, b, 0.95, taus))
    return (np.array([c[0] for c in cols]), np.array([c[1] for c in cols]), np.array([c[2] for c in cols]),
            np.array([c[3] for c in cols], np.int64), np.array([c[4] for c in cols], np.int64),
            np.array([c[5] for c in cols], np.int64).reshape(K, n_tau), np.array([c[6] for c in cols]), 600)


def _row(name, K, pairs):
    s = (np.full(K, 0.5), np.full(K, 0.25), np.full(K, 0.75))
    iso = ",".join("'iso%d'" % k for k in range(K))
    h = {"isoforms": "[%s]" % iso, "counts": "(1,0):12,(0,1):34", "assigned_counts": "0:5,1:41", "chrom": "chr1", "strand": "+",
         "mRNA_starts": "1,2", "mRNA_ends": "3,4"}
    return (name, s, s, np.full(K, 2.5), h, h, pairs)


def test_header():
    f = compare.dpsi_header_fields([0.1, 0.25])
    assert f[:len(compare.HEADER_FIELDS)] == compare.HEADER_FIELDS
    assert f[len(compare.HEADER_FIELDS):] == ["delta_psi_median", "delta_psi_ci_low", "delta_psi_ci_high", "prob_diff_gt_0",
                                              "prob_diff_lt_0", "prob_abs_diff_ge_0.1", "prob_abs_diff_ge_0.25"]


@pytest.mark.parametrize("K", [2, 3, 5])
def test_rows(tmp_path, K):
    thresholds = [0.1, 0.2]
    rows = [_row("ev%d" % e, K, _pairs(K, 2, seed=e)) for e in range(3)]
    out, bf = tmp_path / "a_vs_b.miso_dpsi", tmp_path / "a_vs_b.miso_bf"
    assert compare.write_dpsi(str(out), rows, thresholds) == 3
    compare.write_comparison(str(bf), [r[:6] for r in rows])
    got, want = out.read_text().splitlines(), bf.read_text().splitlines()
    assert got[0].split("\t") == compare.dpsi_header_fields(thresholds)
    n_bf = len(compare.HEADER_FIELDS)
    for line, bf_line, row in zip(got[1:], want[1:], rows):
        assert line.startswith(bf_line + "\t")                    # the `.miso_bf` line verbatim
        f = line.split("\t")[n_bf:]
        med, lo, hi, gt, lt, ge, fin, M = row[6]
        ks = [0] if K == 2 else range(K)
        assert f == [",".join("%.4f" % v[k] for k in ks) for v in (med, lo, hi)] + \
            [",".join("%.4f" % (c[k] / 600.0) for k in ks) for c in (gt, lt, ge[:, 0], ge[:, 1])]


def test_not_finite_and_not_taken(tmp_path):
    rows = [_row("two", 2, _pairs(2, 1, not_finite=(0,))), _row("three", 3, _pairs(3, 1, not_finite=(1,))),
            _row("second_only", 2, _pairs(2, 1, not_finite=(1,))), _row("none", 3, None)]
    out = tmp_path / "t.miso_dpsi"
    compare.write_dpsi(str(out), rows, [0.2])
    n_bf = len(compare.HEADER_FIELDS)
    f = [ln.split("\t")[n_bf:] for ln in out.read_text().splitlines()[1:]]
    assert f[0] == ["NA"] * 6
    assert all(v.split(",")[1] == "NA" and "NA" not in (v.split(",")[0], v.split(",")[2]) for v in f[1])
    assert "NA" not in f[2]                                       # a two-isoform event prints isoform 0
    assert f[3] == ["NA"] * 6


def test_writer_checks_its_thresholds(tmp_path):
    for bad in ([], [0.0], [1.0], [0.1] * 5):
        with pytest.raises(ValueError):
            compare.write_dpsi(str(tmp_path / "x"), [], bad)


def test_filter_events_reads_the_table(tmp_path):
    rows = [_row("ev%d" % e, 2, _pairs(2, 2, seed=e)) for e in range(4)]
    out = tmp_path / "a_vs_b.miso_dpsi"
    compare.write_dpsi(str(out), rows, [0.1, 0.2])
    t = filter_events.Table(str(out))
    assert t.get(2, "event_name") == "ev2" and t.get(2, "prob_abs_diff_ge_0.2") == "%.4f" % (rows[2][6][5][0, 1] / 600.0)
    done = filter_events.multi_filter([str(out)], str(tmp_path / "filtered"), delta_psi_filter=0.0, bf_filter=1.0,
                                      out=open(str(tmp_path / "log"), "w"))
    assert done[0][1:] == (4, 4)
    assert (tmp_path / "filtered" / "a_vs_b.miso_dpsi.filtered").read_bytes() == out.read_bytes()


# ---- argument errors before any work
def _never(*a, **kw):
    raise AssertionError("work was started")


@pytest.mark.parametrize("extra,message", [
    (["--delta-posterior"], "goes with --compare"),
    (["--compare", "b.bam", "--delta-posterior", "--delta-psi-thresholds", "0.1", "1.0"], "outside"),
    (["--compare", "b.bam", "--delta-posterior", "--delta-psi-thresholds", "0.1", "0.2", "0.3", "0.4", "0.5"], "between 1 and 4"),
    (["--compare", "b.bam", "--delta-psi-thresholds", "0.1"], "goes with --exact-compare or --delta-posterior"),
], ids=["no-compare", "bad-threshold", "five-thresholds", "thresholds-alone"])
def test_miso_argument_errors(tmp_path, monkeypatch, capsys, extra, message):
    monkeypatch.setattr(miso_cli, "compute_all_genes_psi", _never)
    monkeypatch.setattr(miso_cli, "GenesDispatcher", _never)
    with pytest.raises(SystemExit) as e:
        miso_cli.main(["--run", str(tmp_path / "index"), str(tmp_path / "a.bam"), "--read-len", "36",
                       "--output-dir", str(tmp_path / "out")] + extra)
    assert e.value.code == 2
    assert message in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


def test_miso_hands_the_flag_on(tmp_path, monkeypatch):
    seen = {}
    monkeypatch.setattr(miso_cli, "compute_all_genes_psi", lambda *a, **kw: seen.update(kw) or 0)
    for extra, want in (([], False), (["--delta-posterior", "--delta-psi-thresholds", "0.3"], True)):
        assert miso_cli.main(["--run", str(tmp_path / "index"), str(tmp_path / "a.bam"), "--read-len", "36", "--output-dir",
                              str(tmp_path / "out"), "--compare", str(tmp_path / "b.bam")] + extra) == 0
        assert seen["delta_posterior"] is want and seen["delta_thresholds"] == ([0.3] if want else None)


@pytest.mark.parametrize("extra,message", [
    (["--summarize-samples", "d", "o", "--delta-posterior"], "goes with --compare-samples"),
    (["--compare-samples", "d1", "d2", "o", "--delta-psi-thresholds", "0.1"], "goes with --delta-posterior"),
    (["--compare-samples", "d1", "d2", "o", "--delta-posterior", "--delta-psi-thresholds", "1.5"], "outside"),
], ids=["no-compare", "thresholds-alone", "bad-threshold"])
def test_samples_utils_argument_errors(monkeypatch, capsys, extra, message):
    for name in ("summarize_sampler_results", "output_samples_comparison"):
        monkeypatch.setattr(samples_utils, name, _never)
    with pytest.raises(SystemExit) as e:
        samples_utils.main(extra)
    assert e.value.code == 2
    assert message in capsys.readouterr().err


def test_samples_utils_hands_the_thresholds_on(monkeypatch):
    seen = {}
    monkeypatch.setattr(samples_utils, "output_samples_comparison", lambda *a, **kw: seen.update(kw) or ("t", 0))
    samples_utils.main(["--compare-samples", "d1", "d2", "o"])
    assert seen["delta_thresholds"] is None
    samples_utils.main(["--compare-samples", "d1", "d2", "o", "--delta-posterior"])
    assert tuple(seen["delta_thresholds"]) == (0.1, 0.2)
    samples_utils.main(["--compare-samples", "d1", "d2", "o", "--delta-posterior", "--delta-psi-thresholds", "0.25", "0.5"])
    assert list(seen["delta_thresholds"]) == [0.25, 0.5]


def test_run_miso_argument_errors(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(run_miso, "compare_gene_psi", _never)
    monkeypatch.setattr(run_miso, "compute_gene_psi", _never)
    rc = run_miso.main(["--compute-genes-from-file", "g", "b", "o", "--read-len", "36", "--delta-posterior-file",
                        str(tmp_path / "t.miso_dpsi")])
    assert rc == 1 and "--delta-posterior-file goes with --compare-genes-from-file" in capsys.readouterr().out
    rc = run_miso.main(["--compare-genes-from-file", "g", "b1", "b2", "o1", "o2", "bf", "--read-len", "36",
                        "--delta-posterior-file", str(tmp_path / "t.miso_dpsi"), "--delta-psi-thresholds", "0.0"])
    assert rc == 1 and "outside" in capsys.readouterr().out
