"""CPU: the front ends of the exact delta psi table: `miso --run ... --exact-delta-posterior` and
`run_miso --exact-delta-file` -- their argument errors before any work, the flag on its way to the workers --, the sampler's
and pysplicing's keyword, and the `.miso_dpsi_exact` writer (compare.write_exact_dpsi).
"""
import os
import sys

import numpy as np
import pytest

from miso_amd import compare, filter_events, run_miso
from miso_amd import miso as miso_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "miso_amd"))

GFF = ("##gff-version 3\n"
       "chr1\tx\tgene\t1000\t1900\t.\t+\t.\tID=g0\n"
       "chr1\tx\tmRNA\t1000\t1900\t.\t+\t.\tID=g0.A;Parent=g0\n"
       "chr1\tx\texon\t1000\t1100\t.\t+\t.\tID=g0.A.1;Parent=g0.A\n"
       "chr1\tx\texon\t1800\t1900\t.\t+\t.\tID=g0.A.2;Parent=g0.A\n"
       "chr1\tx\tmRNA\t1000\t1900\t.\t+\t.\tID=g0.B;Parent=g0\n"
       "chr1\tx\texon\t1000\t1100\t.\t+\t.\tID=g0.B.1;Parent=g0.B\n"
       "chr1\tx\texon\t1400\t1500\t.\t+\t.\tID=g0.B.2;Parent=g0.B\n"
       "chr1\tx\texon\t1800\t1900\t.\t+\t.\tID=g0.B.3;Parent=g0.B\n")


@pytest.mark.parametrize("extra,message", [
    (["--compare", "b.bam", "--exact", "--exact-delta-posterior"], "goes with --exact-compare or --exact-paired-compare"),
    (["--compare", "b.bam", "--delta-posterior", "--exact-delta-posterior"], "goes with --exact-compare or --exact-paired-compare"),
    (["--exact", "--exact-compare", "--exact-delta-posterior"], "goes with --compare"),
    (["--compare", "b.bam", "--exact-compare", "--exact-delta-posterior"], "needs the exact-posterior mode"),
    (["--compare", "b.bam", "--paired-end", "250", "30", "--exact-paired-compare", "--exact-delta-posterior"],
     "needs the paired exact-posterior mode"),
], ids=["no-comparison-flag", "sampled-delta-only", "no-compare", "no-exact-mode", "no-paired-exact-mode"])
def test_miso_argument_errors(tmp_path, monkeypatch, capsys, extra, message):
    def never(*a, **kw):
        raise AssertionError("work was started")
    monkeypatch.setattr(miso_cli, "compute_all_genes_psi", never)
    monkeypatch.setattr(miso_cli, "GenesDispatcher", never)
    with pytest.raises(SystemExit) as e:
        miso_cli.main(["--run", str(tmp_path / "index"), str(tmp_path / "a.bam"), "--read-len", "36",
                       "--output-dir", str(tmp_path / "out")] + extra)
    assert e.value.code == 2
    assert message in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


def test_flag_reaches_the_workers(tmp_path, monkeypatch):
    from miso_amd import index_gff
    gff = tmp_path / "g.gff"
    gff.write_text(GFF)
    idx = str(tmp_path / "indexed")
    index_gff.index_gff(str(gff), idx)
    bam = tmp_path / "reads.bam"
    bam.write_text("")
    monkeypatch.setenv("MISO_DISPATCH", "subprocess")
    cmds = []
    monkeypatch.setattr(miso_cli.GenesDispatcher, "_run_subprocesses",
                        lambda self, jobs, parts, table: cmds.extend(cmd for _, cmd, _ in jobs) or [])
    base = ["--run", idx, str(bam), "--output-dir", str(tmp_path / "out"), "--read-len", "36", "-p", "1", "--compare", str(bam)]
    try:
        assert miso_cli.main(base + ["--exact", "--exact-compare"]) == 0
        assert miso_cli.main(base + ["--exact", "--exact-compare", "--exact-delta-posterior"]) == 0
        assert miso_cli.main(base + ["--paired-end", "250", "30", "--exact-paired", "--exact-paired-compare",
                                     "--exact-delta-posterior", "--delta-psi-thresholds", "0.05"]) == 0
    finally:
        miso_cli.Settings.load(None)
    assert len(cmds) == 3
    assert "--exact-delta-file" not in cmds[0]
    # without the flag the worker's command is what it is with it, less the flag's two words
    at = cmds[1].index("--exact-delta-file")
    assert cmds[1][:at] + cmds[1][at + 2:] == cmds[0]
    for c in cmds[1:]:
        part = c[c.index("--exact-delta-file") + 1]
        assert part.endswith("sample1_vs_sample2.miso_dpsi_exact.gpu0"), c
        assert os.path.dirname(part) == os.path.dirname(c[c.index("--exact-comparison-file") + 1])
    assert cmds[2][cmds[2].index("--delta-psi-thresholds") + 1] == "0.05" and "--paired-end" in cmds[2]


def test_worker_argument_errors(tmp_path, capsys):
    genes, bam = tmp_path / "genes.txt", tmp_path / "reads.bam"
    genes.write_text("g1\t/nowhere/g1.pickle\n")
    bam.write_text("")
    args = ["--compare-genes-from-file", str(genes), str(bam), str(bam), str(tmp_path / "o1"), str(tmp_path / "o2"),
            str(tmp_path / "t.miso_bf"), "--read-len", "36", "--exact", "--exact-delta-file", str(tmp_path / "t.miso_dpsi_exact")]
    try:
        assert run_miso.main(args) == 1
    finally:
        run_miso.Settings.load(None)
    assert "--exact-delta-file goes with --exact-comparison-file" in capsys.readouterr().out
    assert not (tmp_path / "o1").exists()
    with pytest.raises(ValueError, match="goes with the exact comparison"):
        run_miso.compare_gene_psi([], str(bam), str(bam), str(tmp_path / "o1"), str(tmp_path / "o2"), str(tmp_path / "t"),
                                  36, 1, exact=True, exact_delta_file=str(tmp_path / "x"))
    assert not (tmp_path / "o1").exists()


def test_sampler_asks_pysplicing_for_the_quantiles(tmp_path, monkeypatch):
    miso_sampler = run_miso.miso
    seen = []

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.append(kw)
        raise Stop()
    monkeypatch.setattr(miso_sampler.pysplicing, "MISOCompareBatch", fake)
    monkeypatch.setattr(miso_sampler.MISOSampler, "_prepare", lambda self, *a, **kw: ((), (), (), (), None))
    ev = [(None, None, "x.miso")]
    for dfile in (str(tmp_path / "d"), None):
        params = miso_sampler.get_single_end_sampler_params(2, 36, 1)
        params["exact"] = 1
        s = miso_sampler.MISOSampler(params, paired_end=False, log_dir=None)
        with pytest.raises(Stop):
            s.run_comparison_batch(100, ev, ev, str(tmp_path / "t"), num_chains=2, burn_in=10, lag=1, seed=1,
                                   exact_comparison_file=str(tmp_path / "x"), exact_delta_file=dfile)
    assert seen[0]["exact_delta"] == (0.5, 0.025, 0.975) == compare.EXACT_DPSI_PROBS
    assert seen[0]["exact_compare"] == compare.delta_points(compare.DEFAULT_DELTA_THRESHOLDS)
    assert "exact_delta" not in seen[1] and {k: v for k, v in seen[0].items() if k != "exact_delta"} == seen[1]
    with pytest.raises(ValueError, match="goes with the exact comparison"):
        s.run_comparison_batch(100, ev, ev, str(tmp_path / "t"), exact_delta_file=str(tmp_path / "d"))
    assert len(seen) == 2


def test_pysplicing_keyword_errors():
    pysplicing = run_miso.miso.pysplicing     # (the flat module the sampler itself drives)
    with pytest.raises(ValueError, match="requires exact_compare or exact_paired_compare"):
        pysplicing.MISOCompareBatch((), (), 36, exact=True, exact_delta=(0.5,))
    for bad in ((), (0.1, 0.2, 0.3, 0.4, 0.5), [0.5]):
        with pytest.raises(ValueError, match="1 to 4 probabilities"):
            pysplicing.MISOCompareBatch((), (), 36, exact=True, exact_compare=(0.1,), exact_delta=bad)


# ---- the `.miso_dpsi_exact` writer ----
H1 = {"isoforms": "'A_up_B_dn','A_up_dn'", "counts": "(0,1):5,(1,0):11,(1,1):17", "assigned_counts": "0:20,1:13",
      "chrom": "chr1", "strand": "+", "mRNA_starts": "100,100", "mRNA_ends": "900,900"}
H2 = dict(H1, counts="(0,1):9,(1,0):3,(1,1):20", assigned_counts="0:12,1:20")


def _rows(n_thresholds):
    s1 = (np.array([0.56, 0.44]), np.array([0.31, 0.2]), np.array([0.8, 0.69]))
    s2 = (np.array([0.2, 0.8]), np.array([0.07, 0.6]), np.array([0.4, 0.93]))
    grid1 = (np.array([0.5640391, 0.4359609]), np.array([0.30512, 0.2]), np.array([0.80004, 0.69]))
    grid2 = (np.array([0.1961334, 0.8038666]), np.array([0.06, 0.6]), np.array([0.39996, 0.93]))
    cdf = np.array([0.04, 0.001, 0.13, 0.0002])[:2 * n_thresholds]      # at (0.1, -0.1, 0.2, -0.2)
    exact = (0.5640391, 0.1961334, -1.88604, 3.2e13, 13.505, cdf, grid1, grid2)
    delta = (np.array([0.37223482, 0.06438668, 0.64535249]), 0.009374)   # at (0.5, 0.025, 0.975); H(0)
    return [("ev_exact", s1, s2, [6.4, 6.4], H1, H2, exact, delta), ("ev_sampled", s1, s2, [6.4, 6.4], H1, H2, None, None)]


def test_writer_one_threshold_and_filter(tmp_path):
    path = str(tmp_path / "a_vs_b.miso_dpsi_exact")
    assert compare.write_exact_dpsi(path, _rows(1), [0.1]) == 2
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) == 4
    header = lines[0].split("\t")
    assert header == compare.HEADER_FIELDS + ["exact"] + compare.DPSI_FIELDS + ["prob_abs_diff_ge_0.1"]
    # a comparable row: the `.miso_bf_exact` row's leading fields, 1, the quantiles, 1 - H(0), H(0), that table's probability
    xline = compare.exact_comparison_line(*_rows(1)[0][:7], thresholds=[0.1]).split("\t")
    n_head = len(compare.HEADER_FIELDS)
    got = lines[1].split("\t")
    assert got[:n_head] == xline[:n_head] and got[n_head] == "1"
    assert got[n_head + 1:] == ["0.3722", "0.0644", "0.6454", "0.9906", "0.0094", xline[-1]] and xline[-1] == "0.9610"
    # any other event: its `.miso_bf` line verbatim, then exact = 0 and NA in every further field
    plain = compare.comparison_line(*_rows(1)[1][:6])
    assert lines[2] == plain + "\t0" + "\tNA" * 6
    # filter_events reads the table by column name
    t = filter_events.Table(path)
    assert filter_events.filter_rows(t) == [0, 1]
    assert filter_events.filter_rows(t, bayes_factor=10.0) == [0]
    assert filter_events.filter_rows(t, delta_psi=0.365) == [0]


def test_writer_two_thresholds(tmp_path):
    path = str(tmp_path / "a_vs_b.miso_dpsi_exact")
    assert compare.write_exact_dpsi(path, _rows(2), [0.1, 0.2]) == 2
    lines = open(path).read().split("\n")
    assert lines[0].split("\t")[-2:] == ["prob_abs_diff_ge_0.1", "prob_abs_diff_ge_0.2"]
    assert lines[1].split("\t")[-7:] == ["0.3722", "0.0644", "0.6454", "0.9906", "0.0094", "0.9610", "0.8702"]
    assert lines[2].split("\t")[-8:] == ["0"] + ["NA"] * 7
    assert len(lines[1].split("\t")) == len(lines[2].split("\t")) == len(lines[0].split("\t"))
    for bad in ([], [0.0], [0.1, 0.2, 0.3, 0.4, 0.5]):
        with pytest.raises(ValueError):
            compare.write_exact_dpsi(path, _rows(1), bad)
