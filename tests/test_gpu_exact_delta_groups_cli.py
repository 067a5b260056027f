"""GPU: replicates of separate runs meet -- four `miso --run ... --exact --exact-stats` runs of the reference's own test data
set (Atp2b1 GFF + c2c12 SAM), its reads cut into four differing replicates (tests/_bam.py), then
`samples_utils --compare-groups a,b c,d OUT --exact-delta-posterior`: the `.miso_exact_stats` tables,
the pooled `.miso_group_dpsi_exact` table against the restatement on the statistics read back from the four tables, an event
dropped from one replicate's table pooled over the rest, and a run without the new flag byte-identical but for the table."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from _bam import sam_to_bam
from _exact_delta_groups_ref import group_delta
from _exact_ref import Posterior

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
EVENT = "ENSMUSG00000019943"
KEEP = {"a": 1.0, "b": 0.8, "c": 0.6, "d": 0.45}       # the share of the reads a replicate keeps
THRESHOLDS = (0.1, 0.25)

pytestmark = pytest.mark.gpu


def run(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("MISO_EXACT", None)
    return subprocess.run([sys.executable] + args, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=600)


def all_files(top):
    out = {}
    for d, subdirs, names in os.walk(top):
        subdirs[:] = [s for s in subdirs if s not in ("batch-logs", "batch-genes")]      # (time stamps in names and text)
        for f in names:
            out[os.path.relpath(os.path.join(d, f), top)] = open(os.path.join(d, f), "rb").read()
    return out


def read_table(path):
    rows = [ln.split("\t") for ln in open(path).read().splitlines()]
    return rows[0], {r[0]: dict(zip(rows[0], r)) for r in rows[1:]}


def test_four_runs_then_the_pooled_exact_table(tmp_path, orc):
    from miso_amd import compare
    with gzip.open(os.path.join(DATA, "c2c12.Atp2b1.sam.gz"), "rt") as f:
        lines = f.read().splitlines()
    head = [ln for ln in lines if ln.startswith("@")]
    body = [ln for ln in lines if not ln.startswith("@")]
    rng = np.random.default_rng(11)
    settings = tmp_path / "settings.txt"
    settings.write_text("[data]\nmin_event_reads = 5\n[sampler]\nburn_in = 100\nlag = 5\nnum_iters = 600\nnum_chains = 2\n")
    idx = str(tmp_path / "indexed")
    r = run(["-m", "miso_amd.index_gff", "--index", os.path.join(DATA, "Atp2b1.mm9.gff"), idx])
    assert r.returncode == 0, r.stdout
    outs = {}
    for name, share in KEEP.items():
        keep = [ln for ln in body if rng.random() < share]
        bam = str(tmp_path / (name + ".bam"))
        sam_to_bam("\n".join(head + keep) + "\n", bam)
        for flags in ((["--exact-stats"],) if name != "a" else (["--exact-stats"], [])):
            out = str(tmp_path / (name if flags else name + "_plain"))
            r = run(["-m", "miso_amd.miso", "--run", idx, bam, "--output-dir", out, "--read-len", "36",
                     "--settings-filename", str(settings), "-p", "1", "--seed", "31", "--exact"] + flags)
            logs = "".join(open(os.path.join(out, "batch-logs", f)).read() for f in os.listdir(os.path.join(out, "batch-logs")))
            assert r.returncode == 0, r.stdout + logs
            outs[os.path.basename(out)] = out
    # the flag adds one file and changes no other byte
    with_, without = all_files(outs["a"]), all_files(outs["a_plain"])
    table = os.path.join("summary", "a.miso_exact_stats")
    assert sorted(with_) == sorted(list(without) + [table])
    assert all(with_[f] == data for f, data in without.items()) and any(f.endswith(".miso") for f in without)
    stats = {n: compare.read_exact_stats(os.path.join(outs[n], table.replace("a.", n + "."))) for n in KEEP}
    for n in KEEP:
        assert list(stats[n]) == [EVENT] and stats[n][EVENT][0] is True, n
    rows = {n: stats[n][EVENT][1] for n in KEEP}
    assert len({tuple(r[:3]) for r in rows.values()}) == 4          # differing replicates ...
    assert len({tuple(r[3:]) for r in rows.values()}) == 1          # ... of one event

    def pooled(tag, g1, g2):
        out = str(tmp_path / ("cmp_" + tag))
        r = run(["-m", "miso_amd.samples_utils", "--compare-groups", ",".join(outs[n] for n in g1), ",".join(outs[n] for n in g2), out,
                 "--exact-delta-posterior", "--group-names", "ctl", "kd", "--delta-psi-thresholds"] + ["%g" % t for t in THRESHOLDS])
        assert r.returncode == 0, r.stdout
        path = os.path.join(out, "ctl_vs_kd", "delta-psi", "ctl_vs_kd.miso_group_dpsi_exact")
        assert os.path.isfile(os.path.join(out, "a_vs_c", "bayes-factors", "a_vs_c.miso_bf"))     # beside what the run writes today
        return read_table(path), r.stdout
    post = Posterior(orc)
    z = compare.delta_points(THRESHOLDS)

    def want_row(g1, g2):
        w = group_delta(post, [rows[n] for n in g1], [rows[n] for n in g2], compare.EXACT_DPSI_PROBS, z)
        return {"group1_replicates": "%d" % len(g1), "group2_replicates": "%d" % len(g2), "exact": "1",
                "group1_posterior_mean": "%.4f" % w[0], "group2_posterior_mean": "%.4f" % w[1], "diff": "%.4f" % (w[0] - w[1]),
                "delta_psi_median": "%.4f" % w[2], "delta_psi_ci_low": "%.4f" % w[3], "delta_psi_ci_high": "%.4f" % w[4],
                "prob_diff_gt_0": "%.4f" % (1.0 - w[5]), "prob_diff_lt_0": "%.4f" % w[5],
                "prob_abs_diff_ge_0.1": "%.4f" % ((1.0 - w[6]) + w[7]), "prob_abs_diff_ge_0.25": "%.4f" % ((1.0 - w[8]) + w[9])}
    (header, got), _ = pooled("all", ("a", "b"), ("c", "d"))
    assert header == compare.group_dpsi_exact_header_fields(list(THRESHOLDS)) and list(got) == [EVENT]
    want = want_row(("a", "b"), ("c", "d"))
    assert {k: got[EVENT][k] for k in want} == want
    # the event dropped from replicate b's table: pooled over a alone against c and d
    tb = os.path.join(outs["b"], "summary", "b.miso_exact_stats")
    kept = open(tb).read()
    compare.write_exact_stats(tb, [])
    (_, got), text = pooled("dropped", ("a", "b"), ("c", "d"))
    want = want_row(("a",), ("c", "d"))
    assert {k: got[EVENT][k] for k in want} == want and "Notice" not in text
    # ... and marked not exact in both replicates of group 2: NA, the counts, one notice
    open(tb, "w").write(kept)
    for n in ("c", "d"):
        compare.write_exact_stats(os.path.join(outs[n], "summary", n + ".miso_exact_stats"), [(EVENT, False, rows[n])])
    (_, got), text = pooled("none", ("a", "b"), ("c", "d"))
    assert (got[EVENT]["group1_replicates"], got[EVENT]["group2_replicates"], got[EVENT]["exact"]) == ("2", "0", "0")
    assert got[EVENT]["delta_psi_median"] == "NA" and text.count("no replicate with an exact posterior") == 1
    # a missing table is an error that names the directory
    os.remove(tb)
    r = run(["-m", "miso_amd.samples_utils", "--compare-groups", outs["a"] + "," + outs["b"], outs["c"], str(tmp_path / "never"),
             "--exact-delta-posterior"])
    assert r.returncode == 2 and outs["b"] in r.stdout and not (tmp_path / "never").exists()
