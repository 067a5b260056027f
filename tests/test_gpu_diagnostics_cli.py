"""GPU: the two command lines of the chain diagnostics.

* `python -m miso_amd.samples_utils --diagnose-samples`: the `.miso_diag` table of a directory of `.miso` files -- and of
  its miso_pack'ed copy -- equals the table made from parsing the files and tests/_diag_ref.py, line for line.
* `miso --run ... --diagnostics`: one row per written event, the values those of the run's full-precision samples (the
  checker's, which the run's samples equal bit for bit), the `.miso` files byte-identical to a run without the flag.
"""
import gzip
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

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


def _expected_table(tree, C):
    from miso_amd import diagnostics, samples_utils
    lines = []
    for dirpath, _, files in os.walk(tree):
        for fn in files:
            if fn.endswith(".miso"):
                name, samples, _ = samples_utils.parse_miso_file(os.path.join(dirpath, fn))
                cols = [R.diag_fixed(samples[:, k], C) for k in range(samples.shape[1])]
                lines.append(diagnostics.diagnostics_line(name, *[[c[q] for c in cols] for q in range(4)], samples.shape[0], C))
    return ["\t".join(diagnostics.HEADER_FIELDS)] + sorted(lines)


def test_diagnose_samples_on_files_and_on_their_packed_copy(tmp_path, capsys):
    from miso_amd import miso_pack, samples_utils
    rng = np.random.default_rng(77)
    tree = tmp_path / "ctl"
    for e in range(7):
        K = 2 + e % 3
        cols = [R.ar1(rng, 0.2 * (e % 4), 2, 200, mean=(k + 1) / (K + 2.0), sd=0.03) for k in range(K)]
        samples = np.stack(cols, axis=1)
        if e == 5:
            samples[:, 1] = 0.3333                       # a constant column: nan in the table
        # ev06's header speaks of 2 x 150 kept iterations, the file has 400 rows: named in a warning, diagnosed all the same
        _write_miso(str(tree / ("chr%d" % (e % 2)) / ("ev%02d.miso" % e)), samples, 1000, 200 if e != 6 else 400, 4)
    want = _expected_table(str(tree), 2)
    assert len(want) == 8 and want[6].startswith("ev05\t") and ",nan," in want[6]
    assert samples_utils.main(["--diagnose-samples", str(tree), str(tmp_path / "o1"), "--num-chains", "2"]) == 0
    out = capsys.readouterr().out
    warned = [l for l in out.splitlines() if l.startswith("WARNING: ev")]
    assert len(warned) == 1 and warned[0].startswith("WARNING: ev06:"), out
    got = open(str(tmp_path / "o1" / "summary" / "ctl.miso_diag")).read().splitlines()
    assert got == want
    # the default is the settings' six chains: every header disagrees, every event is still diagnosed
    assert samples_utils.main(["--diagnose-samples", str(tree), str(tmp_path / "o6")]) == 0
    assert len([l for l in capsys.readouterr().out.splitlines() if l.startswith("WARNING: ev")]) == 7
    assert open(str(tmp_path / "o6" / "summary" / "ctl.miso_diag")).read().splitlines() == _expected_table(str(tree), 6)
    # the host decoder reads the same doubles
    assert samples_utils.diagnose_sampler_results(str(tree), str(tmp_path / "h.miso_diag"), num_chains=2, decoder="host") == 7
    assert open(str(tmp_path / "h.miso_diag")).read().splitlines() == want
    packed = tmp_path / "packed" / "ctl"
    shutil.copytree(str(tree), str(packed))
    assert miso_pack.pack_dirs([str(packed)]) == 0
    assert not any(fn.endswith(".miso") for _, _, fs in os.walk(str(packed)) for fn in fs)
    capsys.readouterr()
    assert samples_utils.main(["--diagnose-samples", str(packed), str(tmp_path / "o2"), "--num-chains", "2"]) == 0
    assert open(str(tmp_path / "o2" / "summary" / "ctl.miso_diag")).read().splitlines() == want


def _run(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable] + args, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          text=True, timeout=600)


def test_miso_run_with_diagnostics(tmp_path):
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
    outs = {}
    for label, extra in (("plain", ["--summarize"]), ("diag", ["--summarize", "--diagnostics"]),
                         ("only", ["--summary-only", "--diagnostics"])):
        out = str(tmp_path / label / "run")
        r = _run(["-m", "miso_amd.miso", "--run", idx, aln, "--output-dir", out, "--read-len", "36",
                  "--settings-filename", str(settings), "-p", "1", "--seed", "31"] + extra)
        logs = "".join(open(os.path.join(out, "batch-logs", f)).read() for f in os.listdir(os.path.join(out, "batch-logs")))
        assert r.returncode == 0, r.stdout + logs
        outs[label] = out
    rel = os.path.join("10", "ENSMUSG00000019943.miso")
    assert open(os.path.join(outs["plain"], rel), "rb").read() == open(os.path.join(outs["diag"], rel), "rb").read()
    assert open(os.path.join(outs["plain"], "summary", "run.miso_summary"), "rb").read() \
        == open(os.path.join(outs["diag"], "summary", "run.miso_summary"), "rb").read()
    assert not os.path.exists(os.path.join(outs["plain"], "summary", "run.miso_diag"))
    assert not os.path.exists(os.path.join(outs["only"], rel))
    # the run's full-precision samples are the checker's in counter mode (tests/test_gpu_frontend.py): diagnose those
    g = _golden.load("atp2b1")
    gene = gene_utils.load_genes_from_gff(os.path.join(DATA, "Atp2b1.mm9.gff"),
                                          suppress_warnings=True)["ENSMUSG00000019943"]["gene_object"]
    exons = [(p.start, p.end) for p in gene.parts]
    isoforms = [[gene.parts.index(p) for p in iso.parts] for iso in gene.isoforms]
    orc = OrcLib()
    cpu = orc.miso(orc.gene(flat(exons), isoforms), g["pos"], g["cigars"], 36, iters=1000, burn=200, lag=4, chains=2,
                   mode=OrcLib.COUNTER, seed=31, event_id=0)
    assert cpu.rc == 0
    cols = [R.diag_fixed(cpu.samples[:, k], 2) for k in range(2)]
    want = ["\t".join(diagnostics.HEADER_FIELDS),
            diagnostics.diagnostics_line("ENSMUSG00000019943", *[[c[q] for c in cols] for q in range(4)], 400, 2)]
    for label in ("diag", "only"):
        got = open(os.path.join(outs[label], "summary", "run.miso_diag")).read().splitlines()
        assert got == want, (label, got, want)
    # one row per written event
    written = [fn for _, _, fs in os.walk(outs["diag"]) for fn in fs if fn.endswith(".miso")]
    assert len(written) == len(want) - 1
    # --compare: one table per label directory.  Sample 1 draws with the run's seed, sample 2 with the seed the
    # comparison derives for it, both with the event's own number: the checker gives either sample's full-precision draws
    out = str(tmp_path / "cmp")
    r = _run(["-m", "miso_amd.miso", "--run", idx, aln, "--compare", aln, "--labels", "ctl", "kd", "--output-dir", out,
              "--read-len", "36", "--settings-filename", str(settings), "-p", "1", "--seed", "31", "--diagnostics"])
    logs = "".join(open(os.path.join(out, "batch-logs", f)).read() for f in os.listdir(os.path.join(out, "batch-logs")))
    assert r.returncode == 0, r.stdout + logs
    assert open(os.path.join(out, "ctl", rel), "rb").read() == open(os.path.join(outs["plain"], rel), "rb").read()
    assert open(os.path.join(out, "ctl", "summary", "ctl.miso_diag")).read().splitlines() == want, logs
    cpu2 = orc.miso(orc.gene(flat(exons), isoforms), g["pos"], g["cigars"], 36, iters=1000, burn=200, lag=4, chains=2,
                    mode=OrcLib.COUNTER, seed=31 ^ 0x5851F42D4C957F2D, event_id=0)
    assert cpu2.rc == 0
    cols2 = [R.diag_fixed(cpu2.samples[:, k], 2) for k in range(2)]
    want2 = [want[0], diagnostics.diagnostics_line("ENSMUSG00000019943", *[[c[q] for c in cols2] for q in range(4)], 400, 2)]
    assert open(os.path.join(out, "kd", "summary", "kd.miso_diag")).read().splitlines() == want2, logs
