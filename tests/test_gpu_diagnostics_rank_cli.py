"""GPU: the command lines of the rank-normalised chain diagnostics.

* `python -m miso_amd.samples_utils --diagnose-samples ... --rank-diagnostics`: six more columns, those of
  tests/_diag_rank_ref.py rank_fixed on the files' parsed four-decimal values, formatted as diagnostics.py says; the first
  seven columns byte-identical to a run without the flag; a group of events the pass refuses gets one notice and `nan`.
* `miso --run ... --diagnostics --rank-diagnostics`: the `.miso` files and the summary table byte-identical to a run without
  it, the six columns those of the run's full-precision samples (the checker's); with `--compare` one table per label;
  without `--diagnostics` an error.
"""
import gzip
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import _diag_rank_ref as RR
import _diag_ref as R
from _bam import sam_to_bam
from _libs import OrcLib
from _problems import flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "miso_amd"))
DATA = os.path.join(ROOT, "tests", "golden", "data")

pytestmark = pytest.mark.gpu


def _write_miso(path, samples, iters, burn, lag):
    K = samples.shape[1]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("#isoforms=[%s]\texon_lens=('a',100)\titers=%d\tburn_in=%d\tlag=%d\tpercent_accept=90.00\t"
                "proposal_type=drift\tcounts=(1,1):10\tassigned_counts=0:5,1:5\tchrom=chr1\tstrand=+\t"
                "mRNA_starts=1,1\tmRNA_ends=9,9\n" % (",".join("'i%d'" % k for k in range(K)), iters, burn, lag))
        f.write("sampled_psi\tlog_score\n")
        for row in samples:
            f.write("%s\t%.2f\n" % (",".join("%.4f" % v for v in row), -12.5))


def _f(fmt, v):
    return "nan" if math.isnan(v) else fmt % v


def _rank_columns(samples, C, qnorm):
    """The six columns of one event as the table prints them, from rank_fixed."""
    cols = [RR.rank_fixed(samples[:, k], C, 0.95, qnorm) for k in range(samples.shape[1])]
    rhat = [math.nan if math.isnan(c["rhat_bulk"]) or math.isnan(c["rhat_fold"]) else max(c["rhat_bulk"], c["rhat_fold"])
            for c in cols]
    tail = [math.nan if math.isnan(c["ess_ci_low"]) or math.isnan(c["ess_ci_high"]) else min(c["ess_ci_low"], c["ess_ci_high"])
            for c in cols]
    fields = [(rhat, "%.3f"), ([c["ess_bulk"] for c in cols], "%.1f"), (tail, "%.1f"),
              ([c["ess_ci_low"] for c in cols], "%.1f"), ([c["ess_ci_high"] for c in cols], "%.1f")]
    take = slice(None) if len(cols) > 2 else slice(0, 1)
    return [",".join(_f(f, v) for v in vals[take]) for vals, f in fields] + [",".join("%d" % c["distinct"] for c in cols[take])]


def test_diagnose_samples_with_rank_columns(tmp_path, capsys, orc):
    from miso_amd import diagnostics, samples_utils
    qnorm = orc.lib.orc_det_qnorm
    rng = np.random.default_rng(78)
    tree = tmp_path / "ctl"
    for e in range(6):
        K = 2 + e % 3
        cols = [R.ar1(rng, 0.2 * (e % 4), 2, 200, mean=(k + 1) / (K + 2.0), sd=0.03) for k in range(K)]
        samples = np.stack(cols, axis=1)
        if e == 5:
            samples[:, 1] = 0.3333                       # a constant column: nan, one distinct value
        _write_miso(str(tree / ("chr%d" % (e % 2)) / ("ev%02d.miso" % e)), samples, 1000, 200, 4)
    # 40 rows in 2 chains: N = 40 draws, too few for a 95 % interval (lo = 0): refused as a group, diagnosed classically
    short = np.stack([R.ar1(rng, 0.2, 2, 20, mean=0.4, sd=0.03), R.ar1(rng, 0.2, 2, 20, mean=0.6, sd=0.03)], axis=1)
    _write_miso(str(tree / "chr0" / "ev99.miso"), short, 180, 100, 4)
    assert RR.refusal(40, 2, 0.95) == "Too few samples for a credible interval" and RR.refusal(400, 2, 0.95) is None
    assert samples_utils.main(["--diagnose-samples", str(tree), str(tmp_path / "o0"), "--num-chains", "2"]) == 0
    assert "NOTICE" not in capsys.readouterr().out
    assert samples_utils.main(["--diagnose-samples", str(tree), str(tmp_path / "o1"), "--num-chains", "2",
                               "--rank-diagnostics"]) == 0
    out = capsys.readouterr().out
    notices = [l for l in out.splitlines() if l.startswith("NOTICE: no rank diagnostics")]
    assert len(notices) == 1 and "Too few samples for a credible interval" in notices[0], out
    plain = open(str(tmp_path / "o0" / "summary" / "ctl.miso_diag")).read().splitlines()
    got = [l.split("\t") for l in open(str(tmp_path / "o1" / "summary" / "ctl.miso_diag")).read().splitlines()]
    assert ["\t".join(r[:7]) for r in got] == plain and all(len(r) == 13 for r in got)
    assert got[0][7:] == diagnostics.RANK_FIELDS == ["rhat_rank", "ess_bulk", "ess_tail", "ess_ci_low", "ess_ci_high", "num_distinct"]
    rows = {r[0]: r[7:] for r in got[1:]}
    assert sorted(rows) == ["ev%02d" % e for e in range(6)] + ["ev99"]
    assert rows["ev99"] == ["nan"] * 6
    for dirpath, _, files in os.walk(str(tree)):
        for fn in files:
            name, samples, _ = samples_utils.parse_miso_file(os.path.join(dirpath, fn))
            if name != "ev99":
                assert rows[name] == _rank_columns(samples, 2, qnorm), name
    assert rows["ev05"][0].split(",")[1] == "nan" and rows["ev05"][5].split(",")[1] == "1"
    assert "," not in rows["ev00"][0] and rows["ev01"][0].count(",") == 2
    # the host decoder hands the pass the same doubles
    assert samples_utils.diagnose_sampler_results(str(tree), str(tmp_path / "h.miso_diag"), num_chains=2, decoder="host",
                                                  rank=True) == 7
    assert [l.split("\t") for l in open(str(tmp_path / "h.miso_diag")).read().splitlines()] == got
    with pytest.raises(SystemExit):
        samples_utils.main(["--summarize-samples", str(tree), str(tmp_path / "o2"), "--rank-diagnostics"])


def _run(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable] + args, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          text=True, timeout=600)


def test_miso_run_with_rank_diagnostics(tmp_path):
    import _golden
    from miso_amd import diagnostics, gene_utils
    with gzip.open(os.path.join(DATA, "c2c12.Atp2b1.sam.gz"), "rt") as f:
        sam_text = f.read()
    aln = str(tmp_path / "c2c12.Atp2b1.bam")
    sam_to_bam(sam_text, aln)
    idx = str(tmp_path / "indexed")
    settings = tmp_path / "settings.txt"
    settings.write_text("[data]\nfilter_results = True\nmin_event_reads = 20\n"
                        "[sampler]\nburn_in = 200\nlag = 4\nnum_iters = 1000\nnum_chains = 2\n")
    assert _run(["-m", "miso_amd.index_gff", "--index", os.path.join(DATA, "Atp2b1.mm9.gff"), idx]).returncode == 0
    common = ["--read-len", "36", "--settings-filename", str(settings), "-p", "1", "--seed", "31"]
    # an argument error, before any work
    r = _run(["-m", "miso_amd.miso", "--run", idx, aln, "--output-dir", str(tmp_path / "bad"), "--rank-diagnostics"] + common)
    assert r.returncode != 0 and "--rank-diagnostics goes with --diagnostics" in r.stdout
    assert not os.path.exists(str(tmp_path / "bad"))
    outs = {}
    for label, extra in (("diag", ["--summarize", "--diagnostics"]), ("rank", ["--summarize", "--diagnostics", "--rank-diagnostics"])):
        out = str(tmp_path / label / "run")
        r = _run(["-m", "miso_amd.miso", "--run", idx, aln, "--output-dir", out] + common + extra)
        logs = "".join(open(os.path.join(out, "batch-logs", f)).read() for f in os.listdir(os.path.join(out, "batch-logs")))
        assert r.returncode == 0, r.stdout + logs
        outs[label] = out
    rel = os.path.join("10", "ENSMUSG00000019943.miso")
    assert open(os.path.join(outs["diag"], rel), "rb").read() == open(os.path.join(outs["rank"], rel), "rb").read()
    assert open(os.path.join(outs["diag"], "summary", "run.miso_summary"), "rb").read() \
        == open(os.path.join(outs["rank"], "summary", "run.miso_summary"), "rb").read()
    classic = open(os.path.join(outs["diag"], "summary", "run.miso_diag")).read().splitlines()
    # the run's full-precision samples are the checker's in counter mode (tests/test_gpu_frontend.py)
    g = _golden.load("atp2b1")
    gene = gene_utils.load_genes_from_gff(os.path.join(DATA, "Atp2b1.mm9.gff"),
                                          suppress_warnings=True)["ENSMUSG00000019943"]["gene_object"]
    exons = [(p.start, p.end) for p in gene.parts]
    isoforms = [[gene.parts.index(p) for p in iso.parts] for iso in gene.isoforms]
    orc = OrcLib()
    qnorm = orc.lib.orc_det_qnorm

    def want(seed):
        cpu = orc.miso(orc.gene(flat(exons), isoforms), g["pos"], g["cigars"], 36, iters=1000, burn=200, lag=4, chains=2,
                       mode=OrcLib.COUNTER, seed=seed, event_id=0)
        assert cpu.rc == 0
        cols = [R.diag_fixed(cpu.samples[:, k], 2) for k in range(2)]
        line = diagnostics.diagnostics_line("ENSMUSG00000019943", *[[c[q] for c in cols] for q in range(4)], 400, 2)
        return ["\t".join(diagnostics.HEADER_FIELDS + diagnostics.RANK_FIELDS),
                line + "\t" + "\t".join(_rank_columns(cpu.samples, 2, qnorm))]

    got = open(os.path.join(outs["rank"], "summary", "run.miso_diag")).read().splitlines()
    assert got == want(31), (got, want(31))
    assert ["\t".join(l.split("\t")[:7]) for l in got] == classic
    assert "nan" not in got[1]
    # --compare: one table per label directory, sample 2 with the seed the comparison derives for it
    out = str(tmp_path / "cmp")
    r = _run(["-m", "miso_amd.miso", "--run", idx, aln, "--compare", aln, "--labels", "ctl", "kd", "--output-dir", out]
             + common + ["--diagnostics", "--rank-diagnostics"])
    logs = "".join(open(os.path.join(out, "batch-logs", f)).read() for f in os.listdir(os.path.join(out, "batch-logs")))
    assert r.returncode == 0, r.stdout + logs
    assert open(os.path.join(out, "ctl", rel), "rb").read() == open(os.path.join(outs["diag"], rel), "rb").read()
    assert open(os.path.join(out, "ctl", "summary", "ctl.miso_diag")).read().splitlines() == want(31), logs
    assert open(os.path.join(out, "kd", "summary", "kd.miso_diag")).read().splitlines() == want(31 ^ 0x5851F42D4C957F2D), logs
