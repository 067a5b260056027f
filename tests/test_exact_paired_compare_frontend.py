"""CPU: the exact comparison of paired-end samples through the front ends -- `miso --run ... --compare ... --paired-end M SD
--exact-paired --exact-paired-compare` hands the table's name on to its workers, the three argument errors are raised before
any work, the sampler asks pysplicing for exact_paired_compare=, and without a device the calls fail with "no HIP device"
like every other (no CPU path)."""
import os
import sys

import numpy as np
import pytest

import miso_amd
from miso_amd import capi, compare, run_miso
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


def test_flag_reaches_the_workers_and_the_three_argument_errors(tmp_path, monkeypatch):
    from miso_amd import index_gff
    gff = tmp_path / "g.gff"
    gff.write_text(GFF)
    idx = str(tmp_path / "indexed")
    index_gff.index_gff(str(gff), idx)
    bam = tmp_path / "reads.bam"
    bam.write_text("")
    settings = tmp_path / "settings.txt"
    settings.write_text("[sampler]\nburn_in = 10\nlag = 2\nnum_iters = 100\nexact_paired = True\n")
    monkeypatch.setenv("MISO_DISPATCH", "subprocess")
    cmds = []
    monkeypatch.setattr(miso_cli.GenesDispatcher, "_run_subprocesses",
                        lambda self, jobs, parts, table: cmds.extend(cmd for _, cmd, _ in jobs) or [])
    base = ["--run", idx, str(bam), "--output-dir", str(tmp_path / "out"), "--read-len", "36", "-p", "1"]
    pe = ["--paired-end", "250", "30"]
    cmp_ = ["--compare", str(bam)]
    try:
        assert miso_cli.main(base + pe + cmp_ + ["--exact-paired"]) == 0
        assert miso_cli.main(base + pe + cmp_ + ["--exact-paired", "--exact-paired-compare"]) == 0
        assert miso_cli.main(base + pe + cmp_ + ["--exact-paired", "--exact-paired-compare", "--delta-psi-thresholds", "0.05"]) == 0
        # the settings key stands for the flag
        assert miso_cli.main(base + pe + cmp_ + ["--settings-filename", str(settings), "--exact-paired-compare"]) == 0
    finally:
        miso_cli.Settings.load(None)
    assert len(cmds) == 4
    assert "--exact-comparison-file" not in cmds[0]
    for c in cmds[1:]:
        assert c[c.index("--exact-comparison-file") + 1].endswith(".miso_bf_exact.gpu0"), c
        assert "--paired-end" in c
    assert "--exact-paired" in cmds[1] and "--delta-psi-thresholds" not in cmds[1]
    assert cmds[2][cmds[2].index("--delta-psi-thresholds") + 1] == "0.05"
    # argument errors, before any work
    for args in (base + pe + ["--exact-paired", "--exact-paired-compare"],              # without --compare
                 base + cmp_ + ["--exact-paired-compare"],                               # without --paired-end
                 base + pe + cmp_ + ["--exact-paired-compare"],                          # without the paired exact mode
                 base + pe + cmp_ + ["--exact-paired", "--exact-paired-compare", "--delta-psi-thresholds", "1.5"]):
        with pytest.raises(SystemExit):
            miso_cli.main(args)
    assert len(cmds) == 4


def test_worker_checks_the_mode(tmp_path, capsys):
    genes, bam = tmp_path / "genes.txt", tmp_path / "reads.bam"
    genes.write_text("g1\t/nowhere/g1.pickle\n")
    bam.write_text("")
    args = ["--compare-genes-from-file", str(genes), str(bam), str(bam), str(tmp_path / "o1"), str(tmp_path / "o2"),
            str(tmp_path / "t.miso_bf"), "--read-len", "36", "--paired-end", "250", "30",
            "--exact-comparison-file", str(tmp_path / "t.miso_bf_exact")]
    try:
        assert run_miso.main(args) == 1
    finally:
        run_miso.Settings.load(None)
    assert "needs the paired exact mode" in capsys.readouterr().out
    with pytest.raises(ValueError, match="paired exact-posterior mode"):
        run_miso.compare_gene_psi([], str(bam), str(bam), str(tmp_path / "o1"), str(tmp_path / "o2"), str(tmp_path / "t"),
                                  36, 1, paired_end=(250.0, 30.0), exact_paired=False,
                                  exact_comparison_file=str(tmp_path / "x"))


def test_sampler_asks_pysplicing_for_the_paired_comparison(tmp_path, monkeypatch):
    miso_sampler = run_miso.miso
    monkeypatch.delenv(miso_sampler.EXACT_PAIRED_ENV, raising=False)
    seen = []

    class Stop(Exception):
        pass

    def fake(*a, **kw):
        seen.append(kw)
        raise Stop()
    monkeypatch.setattr(miso_sampler.pysplicing, "MISOCompareBatch", fake)
    monkeypatch.setattr(miso_sampler.MISOSampler, "_prepare", lambda self, *a, **kw: ((), (), (), (), None))
    ev = [(None, None, "x.miso")]
    for extra, file in (({"exact_paired": 1}, str(tmp_path / "x")), ({"exact_paired": 1}, None)):
        params = miso_sampler.get_paired_end_sampler_params(2, 250, 900, 36, overhang_len=1)
        params.update(extra)
        s = miso_sampler.MISOSampler(params, paired_end=True, log_dir=None)
        with pytest.raises(Stop):
            s.run_comparison_batch(100, ev, ev, str(tmp_path / "t"), num_chains=2, burn_in=10, lag=1, seed=1,
                                   exact_comparison_file=file, delta_thresholds=[0.05])
    assert seen[0]["exact_paired"] is True and seen[0]["exact_paired_compare"] == compare.delta_points([0.05])
    assert "exact_compare" not in seen[0] and "exact_paired_compare" not in seen[1]
    params = miso_sampler.get_paired_end_sampler_params(2, 250, 900, 36, overhang_len=1)
    s = miso_sampler.MISOSampler(params, paired_end=True, log_dir=None)
    with pytest.raises(ValueError, match="paired exact-posterior mode"):
        s.run_comparison_batch(100, ev, ev, str(tmp_path / "t"), exact_comparison_file=str(tmp_path / "x"))


def test_pysplicing_keyword_errors():
    pysplicing = run_miso.miso.pysplicing     # (the flat module the sampler itself drives)
    with pytest.raises(ValueError, match="requires exact_paired=True"):
        pysplicing.MISOCompareBatch((), (), 36, paired=(250.0, 900.0, 4.0), exact_paired_compare=(0.1,))
    with pytest.raises(ValueError, match="at most 8"):
        pysplicing.MISOCompareBatch((), (), 36, paired=(250.0, 900.0, 4.0), exact_paired=True,
                                    exact_paired_compare=tuple(0.01 * k for k in range(9)))


def test_no_cpu_path():
    if capi.device_count() > 0:
        return      # (with a device the calls work: tests/test_gpu_exact_paired_compare.py)
    one = [[1.0, 1.0, 60000.0, 43000.0, 1.0, 1.0]]
    with pytest.raises(miso_amd.InternalError) as err:
        capi.selftest_exact_paired_compare(one, [[(0.01, 0.002)]], one, [[]], [0.1])
    assert "no HIP device" in str(err.value)
    # ... and the argument checks come after the device's, as everywhere
    bs = []
    for _ in range(2):
        b = miso_amd.Batch(36, iters=50, burn=10, lag=1, chains=1, paired=True, mean=250.0, var=900.0, exact_paired=True)
        b.add_problem(np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]), [1500, 1000], [3, 2],
                      fraglen=np.array([[250, 0], [0, 240], [260, 200]], np.int32))
        bs.append(b)
    with pytest.raises(miso_amd.InternalError):
        bs[0].compare_exact_paired(bs[1], [0.1])
