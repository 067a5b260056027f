"""GPU: paired-end replicates of separate runs meet -- four `miso --run ... --paired-end 250 30 --exact-paired
--exact-paired-stats` runs on one four-gene index and a synthetic paired SAM file per replicate (the recipe of
tests/test_gpu_exact_paired_cli.py make_inputs, other seeds and expression per replicate), then
`samples_utils --compare-groups a,b c,d OUT --exact-paired-delta-posterior`: the `.miso_exact_pairs`
tables, the pooled `.miso_group_dpsi_exact` table against the restatement on the tables read back, an event dropped from one
replicate's table pooled over the rest, the three-isoform gene NA, and a run without the new flag byte-identical but for the
table."""
import os
import subprocess
import sys

import numpy as np
import pytest

from _exact_paired_compare_ref import PairedCompare
from _exact_paired_delta_groups_ref import group_delta
from _exact_paired_ref import PairedStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "miso_amd"))

pytestmark = pytest.mark.gpu

N_GENES = 4
K3 = 2                  # a three-isoform gene: never the mode's
SETTINGS = "[data]\nmin_event_reads = 20\n[sampler]\nburn_in = 100\nlag = 5\nnum_iters = 600\nnum_chains = 2\n"
REPLICATES = {"a": (11, False), "b": (12, False), "c": (13, True), "d": (14, True)}      # seed, expression reversed
THRESHOLDS = (0.1, 0.25)


def run(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    import miso_sampler
    env.pop(miso_sampler.EXACT_PAIRED_ENV, None)
    env.pop("MISO_EXACT", None)
    return subprocess.run([sys.executable] + args, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=600)


def make_inputs(tmp_path):
    """one GFF of four genes, and per replicate a SAM file of its own read pairs"""
    from miso_amd import capi, workload
    lines, genes = ["##gff-version 3"], []
    for e in range(N_GENES):
        K = 3 if e == K3 else 2
        off = 10000 + e * 9000
        exons, isoforms, expr = workload.event_gene(e, K, min_len=400, max_len=800, gap=300)
        ex = [(s + off, t + off) for s, t in exons]
        gid = "gene%d" % e
        lines.append("chr1\tx\tgene\t%d\t%d\t.\t+\t.\tID=%s" % (ex[0][0], ex[-1][1], gid))
        for m, iso in enumerate(isoforms):
            tid = "%s.t%d" % (gid, m)
            lines.append("chr1\tx\tmRNA\t%d\t%d\t.\t+\t.\tID=%s;Parent=%s" % (ex[iso[0]][0], ex[iso[-1]][1], tid, gid))
            lines += ["chr1\tx\texon\t%d\t%d\t.\t+\t.\tID=%s.e%d;Parent=%s" % (ex[x][0], ex[x][1], tid, x, tid) for x in iso]
        genes.append((capi.Gene(exons, isoforms), list(expr), off))
    gff = tmp_path / "g.gff"
    gff.write_text("\n".join(lines) + "\n")
    sams = {}
    for name, (seed, reverse) in REPLICATES.items():
        rng = np.random.default_rng(seed)
        recs = []
        for e, (g, expr, off) in enumerate(genes):
            n = int(rng.integers(150, 320))
            _, pos, cig = capi.simulate_reads(g, expr[::-1] if reverse else expr, n, 36, 100 * seed + e, 250.0, 900.0)
            for i in range(n):
                a, b = int(pos[2 * i]) + off, int(pos[2 * i + 1]) + off
                recs.append("p%d_%d\t99\tchr1\t%d\t255\t%s\t=\t%d\t0\t%s\t%s" % (e, i, a, cig[2 * i].decode(), b, "A" * 36, "I" * 36))
                recs.append("p%d_%d\t147\tchr1\t%d\t255\t%s\t=\t%d\t0\t%s\t%s" % (e, i, b, cig[2 * i + 1].decode(), a, "A" * 36, "I" * 36))
        sam = tmp_path / (name + ".sam")
        sam.write_text("@SQ\tSN:chr1\tLN:250000\n" + "\n".join(recs) + "\n")
        sams[name] = str(sam)
    return str(gff), sams


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
    gff, sams = make_inputs(tmp_path)
    idx = str(tmp_path / "idx")
    assert run(["-m", "miso_amd.index_gff", "--index", gff, idx]).returncode == 0
    settings = tmp_path / "s.txt"
    settings.write_text(SETTINGS)
    outs = {}
    for name in REPLICATES:
        for flags in ((["--exact-paired-stats"],) if name != "a" else (["--exact-paired-stats"], [])):
            out = str(tmp_path / (name if flags else name + "_plain"))
            r = run(["-m", "miso_amd.miso", "--run", idx, sams[name], "--output-dir", out, "--read-len", "36", "--paired-end", "250", "30",
                     "--settings-filename", str(settings), "-p", "1", "--seed", "19", "--exact-paired"] + flags)
            logs = "".join(open(os.path.join(out, "batch-logs", f)).read() for f in os.listdir(os.path.join(out, "batch-logs")))
            assert r.returncode == 0, r.stdout + logs
            outs[os.path.basename(out)] = out
    # the flag adds one file and changes no other byte
    with_, without = all_files(outs["a"]), all_files(outs["a_plain"])
    table = os.path.join("summary", "a.miso_exact_pairs")
    assert sorted(with_) == sorted(list(without) + [table])
    assert all(with_[f] == data for f, data in without.items()) and any(f.endswith(".miso") for f in without)
    tabs = {n: compare.read_exact_pairs(os.path.join(outs[n], table.replace("a.", n + "."))) for n in REPLICATES}
    events = ["gene%d" % e for e in range(N_GENES)]
    two = [ev for ev in events if ev != "gene%d" % K3]
    for n in REPLICATES:
        assert sorted(tabs[n]) == events, n
        assert [tabs[n][ev][0] for ev in events] == [ev in two for ev in events], n
        assert all(len(tabs[n][ev][2]) > 0 for ev in two), n
    assert len({tabs[n]["gene0"][2].tobytes() for n in REPLICATES}) == 4          # differing replicates

    def pooled(tag, g1, g2):
        out = str(tmp_path / ("cmp_" + tag))
        r = run(["-m", "miso_amd.samples_utils", "--compare-groups", ",".join(outs[n] for n in g1), ",".join(outs[n] for n in g2), out,
                 "--exact-paired-delta-posterior", "--group-names", "ctl", "kd", "--delta-psi-thresholds"] + ["%g" % t for t in THRESHOLDS])
        assert r.returncode == 0, r.stdout
        return read_table(os.path.join(out, "ctl_vs_kd", "delta-psi", "ctl_vs_kd.miso_group_dpsi_exact")), r.stdout
    post = PairedCompare(orc)
    z = compare.delta_points(THRESHOLDS)

    def want_row(ev, g1, g2):
        ps = [[PairedStats(*(tabs[n][ev][1] + [tabs[n][ev][2]])) for n in g] for g in (g1, g2)]
        w = group_delta(post, ps[0], ps[1], compare.EXACT_DPSI_PROBS, z)
        return {"group1_replicates": "%d" % len(g1), "group2_replicates": "%d" % len(g2), "exact": "1",
                "group1_posterior_mean": "%.4f" % w[0], "group2_posterior_mean": "%.4f" % w[1], "diff": "%.4f" % (w[0] - w[1]),
                "delta_psi_median": "%.4f" % w[2], "delta_psi_ci_low": "%.4f" % w[3], "delta_psi_ci_high": "%.4f" % w[4],
                "prob_diff_gt_0": "%.4f" % (1.0 - w[5]), "prob_diff_lt_0": "%.4f" % w[5],
                "prob_abs_diff_ge_0.1": "%.4f" % ((1.0 - w[6]) + w[7]), "prob_abs_diff_ge_0.25": "%.4f" % ((1.0 - w[8]) + w[9])}
    (header, got), _ = pooled("all", ("a", "b"), ("c", "d"))
    assert header == compare.group_dpsi_exact_header_fields(list(THRESHOLDS)) and sorted(got) == events
    for ev in two:
        want = want_row(ev, ("a", "b"), ("c", "d"))
        assert {k: got[ev][k] for k in want} == want, ev
    # the three-isoform gene: in every table, never exact
    k3 = got["gene%d" % K3]
    assert (k3["group1_replicates"], k3["group2_replicates"], k3["exact"], k3["delta_psi_median"]) == ("0", "0", "0", "NA")
    # an event dropped from replicate b's table: pooled over a alone against c and d
    tb = os.path.join(outs["b"], "summary", "b.miso_exact_pairs")
    compare.write_exact_pairs(tb, [(ev,) + tabs["b"][ev] for ev in events if ev != "gene1"])
    (_, got), _ = pooled("dropped", ("a", "b"), ("c", "d"))
    want = want_row("gene1", ("a",), ("c", "d"))
    assert {k: got["gene1"][k] for k in want} == want
    want = want_row("gene0", ("a", "b"), ("c", "d"))
    assert {k: got["gene0"][k] for k in want} == want
    # a missing table is an error that names the directory
    os.remove(tb)
    r = run(["-m", "miso_amd.samples_utils", "--compare-groups", outs["a"] + "," + outs["b"], outs["c"], str(tmp_path / "never"),
             "--exact-paired-delta-posterior"])
    assert r.returncode == 2 and outs["b"] in r.stdout and not (tmp_path / "never").exists()
