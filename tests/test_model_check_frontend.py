"""CPU: the model check's switches -- `miso --run ... --model-check`, `run_miso --model-check-file(s)` and
params["model_check"] end in capi.Batch(model_check=True); --paired-end is refused while the arguments are parsed -- and
the `.miso_fit` table's format (miso_amd/model_check.py), NA rows included."""
import os
import sys

import numpy as np
import pytest

from miso_amd import capi, model_check, run_miso
from miso_amd import miso as miso_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "miso_amd"))


class _Recorded(Exception):
    pass


@pytest.fixture
def batch_kwargs(monkeypatch):
    """capi.Batch replaced by a recorder: the keyword arguments of the batch a front end would have made"""
    seen = []

    def fake(*a, **kw):
        seen.append(kw)
        raise _Recorded()
    monkeypatch.setattr(run_miso.miso.capi, "Batch", fake)     # (miso_sampler's flat import of capi.py)
    return seen


def _prepare(params_extra, paired=False):
    miso_sampler = run_miso.miso
    if paired:
        params = miso_sampler.get_paired_end_sampler_params(2, 250, 900, 36, overhang_len=1)
    else:
        params = miso_sampler.get_single_end_sampler_params(2, 36, 1)
    params.update(params_extra)
    s = miso_sampler.MISOSampler(params, paired_end=paired, log_dir=None)
    with pytest.raises(_Recorded):
        s.prepare_batch(100, [], num_chains=2, burn_in=10, lag=1)


def test_the_parameter_reaches_the_batch(batch_kwargs):
    _prepare({})
    _prepare({"model_check": 1})
    _prepare({"model_check": 1}, paired=True)        # single-end only: a paired-end batch is never asked
    assert [kw["model_check"] for kw in batch_kwargs] == [False, True, False]


def test_paired_end_is_refused_at_parsing(tmp_path, capsys):
    for main, argv in ((miso_cli.main, ["--run", "idx", "reads.bam", "--output-dir", str(tmp_path), "--read-len", "36",
                                        "--paired-end", "250", "30", "--model-check"]),
                       (run_miso.main, ["--compute-genes-from-file", "g", "b", "o", "--read-len", "36", "--paired-end", "250", "30",
                                        "--model-check-file", str(tmp_path / "t")]),
                       (run_miso.main, ["--compare-genes-from-file", "g", "b1", "b2", "o1", "o2", "bf", "--read-len", "36",
                                        "--paired-end", "250", "30", "--model-check-files", "f1", "f2"])):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2
        assert "single-end only" in capsys.readouterr().err
    assert not os.listdir(str(tmp_path))               # before any work


def test_run_miso_hands_the_file_on(tmp_path, monkeypatch):
    calls = []
    monkeypatch.setattr(run_miso, "compute_gene_psi", lambda *a, **kw: calls.append(kw))
    genes, bam = tmp_path / "genes.txt", tmp_path / "reads.bam"
    genes.write_text("g1\t/nowhere/g1.pickle\n")
    bam.write_text("")
    base = ["--compute-genes-from-file", str(genes), str(bam), str(tmp_path / "out"), "--read-len", "36"]
    assert run_miso.main(base) == 0
    assert run_miso.main(base + ["--model-check-file", "fit.tsv"]) == 0
    assert [kw["model_check_file"] for kw in calls] == [None, "fit.tsv"]


def test_compute_gene_psi_hands_the_switch_to_the_sampler(tmp_path, monkeypatch):
    made = []

    class Stop(Exception):
        pass

    class FakeSampler(object):
        def __init__(self, params, **kw):
            made.append(dict(params))
            raise Stop()
    monkeypatch.setattr(run_miso.miso, "MISOSampler", FakeSampler)
    monkeypatch.setattr(run_miso, "collect_gene_events", lambda entries, *a, **kw: ([(None, None, None, None, 0)], {}))
    monkeypatch.setattr(run_miso, "preload_genes", lambda *a, **kw: None)
    for f in (str(tmp_path / "fit"), None):
        with pytest.raises(Stop):
            run_miso.compute_gene_psi(None, None, "reads.bam", str(tmp_path / "o"), 36, 1, gene_entries=[("g", "i")],
                                      bamfile=object(), model_check_file=f, verbose=False)
    assert ["model_check" in p for p in made] == [True, False]
    with pytest.raises(ValueError, match="single-end"):
        run_miso.compute_gene_psi(None, None, "reads.bam", str(tmp_path / "o"), 36, 1, gene_entries=[("g", "i")],
                                  bamfile=object(), model_check_file="f", paired_end=(250, 30), verbose=False)


def test_dispatcher_names_the_tables(tmp_path, monkeypatch):
    from miso_amd import index_gff
    gff = tmp_path / "g.gff"
    gff.write_text("##gff-version 3\n"
                   "chr1\tx\tgene\t1000\t1900\t.\t+\t.\tID=g0\n"
                   "chr1\tx\tmRNA\t1000\t1900\t.\t+\t.\tID=g0.A;Parent=g0\n"
                   "chr1\tx\texon\t1000\t1100\t.\t+\t.\tID=g0.A.1;Parent=g0.A\n"
                   "chr1\tx\texon\t1800\t1900\t.\t+\t.\tID=g0.A.2;Parent=g0.A\n"
                   "chr1\tx\tmRNA\t1000\t1900\t.\t+\t.\tID=g0.B;Parent=g0\n"
                   "chr1\tx\texon\t1000\t1100\t.\t+\t.\tID=g0.B.1;Parent=g0.B\n"
                   "chr1\tx\texon\t1400\t1500\t.\t+\t.\tID=g0.B.2;Parent=g0.B\n"
                   "chr1\tx\texon\t1800\t1900\t.\t+\t.\tID=g0.B.3;Parent=g0.B\n")
    idx = str(tmp_path / "indexed")
    index_gff.index_gff(str(gff), idx)
    bam = tmp_path / "reads.bam"
    bam.write_text("")
    monkeypatch.setenv("MISO_DISPATCH", "subprocess")
    cmds = []
    monkeypatch.setattr(miso_cli.GenesDispatcher, "_run_subprocesses",
                        lambda self, jobs, parts, table: cmds.extend(cmd for _, cmd, _ in jobs) or [])
    out = str(tmp_path / "out")
    base = ["--run", idx, str(bam), "--output-dir", out, "--read-len", "36", "-p", "1"]
    for flag in ([], ["--model-check"], ["--model-check", "--compare", str(bam), "--labels", "a", "b"]):
        assert miso_cli.main(base + flag) == 0
    assert len(cmds) == 3 and not any(c.startswith("--model-check") for c in cmds[0])
    one = cmds[1][cmds[1].index("--model-check-file") + 1]
    assert one == os.path.join(out, "summary", "out.miso_fit.gpu0")
    at = cmds[2].index("--model-check-files")
    assert cmds[2][at + 1:at + 3] == [os.path.join(out, l, "summary", l + ".miso_fit.gpu0") for l in ("a", "b")]


def _fit(status, **kw):
    d = dict(pattern=np.array([2, 1, 3], np.uint64), m=np.array([35, 85, 130]), n=np.array([12, 34, 154], np.int32), num_reads=200,
             num_off_model=1, rows=400, bad_rows=0, exceed=100, sum_obs=800.0, sum_rep=600.5, expected=np.array([11.96, 33.44, 154.6]),
             ge=np.array([200, 100, 399], np.int32), le=np.array([250, 320, 1], np.int32))
    d.update(kw)
    return capi.ModelFit(status, **d)


def test_table_format(tmp_path):
    f = tmp_path / "x.miso_fit"
    rows = [("ev1", _fit("ok"), 2), ("ev2", _fit("no_reads", num_reads=0), 2), ("ev3", _fit("too_many_classes"), 2),
            ("ev4", _fit("no_rows"), 2), ("ev5", _fit("no_gene"), 2)]
    assert model_check.write_model_fit(str(f), rows) == 5
    lines = f.read_text().split("\n")
    assert lines[-1] == "" and len(lines) == 7
    assert lines[0].split("\t") == ["event_name", "num_reads", "num_off_model", "num_classes", "num_rows", "fit_pvalue",
                                    "mean_disc_obs", "mean_disc_rep", "observed", "expected", "tail_ge", "tail_le"]
    assert lines[1].split("\t") == ["ev1", "200", "1", "3", "400", "0.2500", "2.0000", "1.5012",
                                    "(0,1):12,(1,0):34,(1,1):154", "(0,1):12.0,(1,0):33.4,(1,1):154.6",
                                    "(0,1):0.5000,(1,0):0.2500,(1,1):0.9975", "(0,1):0.6250,(1,0):0.8000,(1,1):0.0025"]
    for k in range(2, 6):
        assert lines[k].split("\t") == ["ev%d" % k] + ["NA"] * 11
    assert model_check.class_key(5, 3) == "(1,0,1)"
