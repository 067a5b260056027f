"""GPU: `miso --run ... --exact` end to end on the reference's own test data set (Atp2b1 GFF + c2c12 SAM, the inputs of
misopy/test_miso.py:131-171): the same file tree as a run without the flag, percent_accept=100 in the header, the same
read classes, and a posterior mean that agrees with the default run's."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "miso_amd"))
DATA = os.path.join(ROOT, "tests", "golden", "data")

pytestmark = pytest.mark.gpu


def run(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("MISO_EXACT", None)
    return subprocess.run([sys.executable] + args, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=600)


def tree(d):
    return sorted(os.path.relpath(os.path.join(b, f), d) for b, _, fs in os.walk(d) for f in fs
                  if "batch-logs" not in b and "batch-genes" not in b)


def test_miso_run_exact_on_reference_test_data(tmp_path):
    import miso_sampler
    with gzip.open(os.path.join(DATA, "c2c12.Atp2b1.sam.gz"), "rt") as f:
        sam_text = f.read()
    aln = str(tmp_path / "c2c12.Atp2b1.sam")
    open(aln, "w").write(sam_text)
    idx = str(tmp_path / "indexed")
    settings = tmp_path / "settings.txt"
    settings.write_text("[data]\nfilter_results = True\nmin_event_reads = 20\n"
                        "[sampler]\nburn_in = 3000\nlag = 10\nnum_iters = 13000\nnum_chains = 2\n")
    r = run(["-m", "miso_amd.index_gff", "--index", os.path.join(DATA, "Atp2b1.mm9.gff"), idx])
    assert r.returncode == 0, r.stdout
    outs = {}
    for name, flag in (("default", []), ("exact", ["--exact", "--diagnostics"])):
        out = str(tmp_path / name)
        r = run(["-m", "miso_amd.miso", "--run", idx, aln, "--output-dir", out, "--read-len", "36",
                 "--settings-filename", str(settings), "-p", "1", "--seed", "31"] + flag)
        logs = "".join(open(os.path.join(out, "batch-logs", f)).read() for f in os.listdir(os.path.join(out, "batch-logs")))
        assert r.returncode == 0, r.stdout + logs
        outs[name] = out
    diag = os.path.join("summary", "exact.miso_diag")
    assert [f for f in tree(outs["exact"]) if f != diag] == tree(outs["default"]) and diag in tree(outs["exact"])
    # --diagnostics on the exact run: independent draws -- split R-hat about 1, effective sample size about the row count
    # (the estimators' own noise at 2000 rows of 2 chains: a few per cent)
    rows = [ln.split("\t") for ln in open(os.path.join(outs["exact"], diag)).read().splitlines()]
    assert rows[0][:4] == ["event_name", "rhat", "ess", "mcse"] and len(rows) == 2 and rows[1][0] == "ENSMUSG00000019943"
    rhat, ess = float(rows[1][1]), float(rows[1][2])       # (two isoforms: the first isoform's scalars)
    assert abs(rhat - 1) < 0.01 and 0.7 * 2000 < ess < 1.4 * 2000 and rows[1][5:] == ["2000", "2"], rows[1]
    rel = os.path.join("10", "ENSMUSG00000019943.miso")
    assert rel in tree(outs["exact"])
    d_samples, d_hdr, _ = miso_sampler.load_samples(os.path.join(outs["default"], rel))
    e_samples, e_hdr, _ = miso_sampler.load_samples(os.path.join(outs["exact"], rel))
    assert e_samples.shape == d_samples.shape == (2000, 2)
    assert float(e_hdr["percent_accept"]) == 100.0 and float(d_hdr["percent_accept"]) < 100.0
    for key in ("counts", "iters", "burn_in", "lag", "chrom", "strand", "mRNA_starts", "mRNA_ends"):
        assert e_hdr[key] == d_hdr[key], key
    assert np.allclose(e_samples.sum(1), 1.0, atol=1.01e-4)
    # the rule of the statistical tests, 4 se + 2e-3, with the standard error of the DEFAULT run's mean taken from
    # the means of eight consecutive blocks of its 2000 rows (every block holds both chains; the exact rows are
    # independent draws and add their own, smaller, error: sd / sqrt(2000)).  The default run is a long one on purpose:
    # this event's mass sits at psi ~ 0.007 and its chains, started at 0.5, need more than the 200 iterations of burn-in
    # of the other command-line tests to get there (at burn_in = 200, num_iters = 1000 the default run's mean was still
    # 0.0215 against the posterior's 0.0069).
    blocks = d_samples[:, 0].reshape(8, 250).mean(1)
    se = np.sqrt(blocks.var(ddof=1) / 8 + e_samples[:, 0].var(ddof=1) / 2000)
    print("exact %.5f, default %.5f, se %.5f" % (e_samples[:, 0].mean(), d_samples[:, 0].mean(), se))
    assert abs(e_samples[:, 0].mean() - d_samples[:, 0].mean()) < 4 * se + 2e-3
