"""GPU: `miso --run INDEX SAM --compare SAM2 --paired-end 250 30 --exact-paired --exact-paired-compare` end to end on a
six-gene index and two synthetic paired SAM files: the `.miso_bf_exact` table beside the `.miso_bf`, its comparable rows
against capi's own numbers for the same read pairs (no seed enters them), every other output byte-identical to a run
without the flag, and filter_events on the new table."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "miso_amd"))

pytestmark = pytest.mark.gpu

N_GENES = 6
K3 = (2,)               # a three-isoform gene: sampled, never exact-comparable
THRESHOLDS = (0.1, 0.25)
SETTINGS = "[data]\nmin_event_reads = 20\n[sampler]\nburn_in = 100\nlag = 5\nnum_iters = 600\nnum_chains = 2\n"


def run(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    import miso_sampler
    env.pop(miso_sampler.EXACT_PAIRED_ENV, None)
    env.pop("MISO_EXACT", None)
    return subprocess.run([sys.executable] + args, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=600)


def make_inputs(tmp_path):
    """GFF3 of six synthetic genes and one paired SAM per sample (another expression in sample 2); returns per gene and
    sample (exons, isoforms, pos, cigars) in the gene's own coordinates"""
    from miso_amd import capi, workload
    rng = np.random.default_rng(4)
    lines, recs, events = ["##gff-version 3"], ([], []), []
    for e in range(N_GENES):
        K = 3 if e in K3 else 2
        off = 10000 + e * 9000
        exons, isoforms, expr = workload.event_gene(e, K, min_len=400, max_len=800, gap=300)
        g = capi.Gene(exons, isoforms)
        ex = [(s + off, t + off) for s, t in exons]
        gid = "gene%d" % e
        lines.append("chr1\tx\tgene\t%d\t%d\t.\t+\t.\tID=%s" % (ex[0][0], ex[-1][1], gid))
        for m, iso in enumerate(isoforms):
            tid = "%s.t%d" % (gid, m)
            lines.append("chr1\tx\tmRNA\t%d\t%d\t.\t+\t.\tID=%s;Parent=%s" % (ex[iso[0]][0], ex[iso[-1]][1], tid, gid))
            lines += ["chr1\tx\texon\t%d\t%d\t.\t+\t.\tID=%s.e%d;Parent=%s" % (ex[x][0], ex[x][1], tid, x, tid) for x in iso]
        per_sample = []
        for s in (0, 1):
            n = int(rng.integers(60, 200))
            _, pos, cig = capi.simulate_reads(g, expr if s == 0 else expr[::-1].copy(), n, 36, 7000 + 2 * e + s, 250.0, 900.0)
            assert len(pos) == 2 * n
            for i in range(n):
                a, b = int(pos[2 * i]) + off, int(pos[2 * i + 1]) + off
                recs[s].append("p%d_%d\t99\tchr1\t%d\t255\t%s\t=\t%d\t0\t%s\t%s" % (e, i, a, cig[2 * i].decode(), b, "A" * 36, "I" * 36))
                recs[s].append("p%d_%d\t147\tchr1\t%d\t255\t%s\t=\t%d\t0\t%s\t%s" % (e, i, b, cig[2 * i + 1].decode(), a, "A" * 36, "I" * 36))
            per_sample.append((exons, isoforms, pos, cig))
        events.append(per_sample)
    gff = tmp_path / "g.gff"
    gff.write_text("\n".join(lines) + "\n")
    sams = []
    for s in (0, 1):
        sam = tmp_path / ("r%d.sam" % s)
        sam.write_text("@SQ\tSN:chr1\tLN:250000\n" + "\n".join(recs[s]) + "\n")
        sams.append(str(sam))
    return str(gff), sams, events


def read_table(path):
    rows = [ln.split("\t") for ln in open(path).read().splitlines()]
    return rows[0], {r[0]: dict(zip(rows[0], r)) for r in rows[1:]}


def test_exact_paired_compare_table_end_to_end(tmp_path):
    import miso_amd
    from miso_amd import compare, filter_events
    gff, sams, events = make_inputs(tmp_path)
    settings = tmp_path / "s.txt"
    settings.write_text(SETTINGS)
    idx = str(tmp_path / "idx")
    assert run(["-m", "miso_amd.index_gff", "--index", gff, idx]).returncode == 0
    outs = {}
    for name, extra in (("plain", []), ("xc", ["--exact-paired-compare", "--delta-psi-thresholds"] + ["%g" % t for t in THRESHOLDS])):
        out = str(tmp_path / name)
        r = run(["-m", "miso_amd.miso", "--run", idx, sams[0], "--compare", sams[1], "--labels", "a", "b", "--paired-end", "250", "30",
                 "--exact-paired", "--output-dir", out, "--read-len", "36", "--settings-filename", str(settings), "-p", "1",
                 "--seed", "77"] + extra)
        logs = "".join(open(os.path.join(out, "batch-logs", f)).read() for f in os.listdir(os.path.join(out, "batch-logs")))
        assert r.returncode == 0, r.stdout + logs
        files = {}
        for lab in ("a", "b"):
            d = os.path.join(out, lab, "chr1")
            files.update({lab + "/" + f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))})
        bf_dir = os.path.join(out, "a_vs_b", "bayes-factors")
        files["bf"] = open(os.path.join(bf_dir, "a_vs_b.miso_bf"), "rb").read()
        outs[name] = (files, sorted(os.listdir(bf_dir)))
    # the flag adds one file and changes no other byte
    assert outs["plain"][0] == outs["xc"][0]
    assert outs["plain"][1] == ["a_vs_b.miso_bf"] and outs["xc"][1] == ["a_vs_b.miso_bf", "a_vs_b.miso_bf_exact"]
    table = os.path.join(str(tmp_path / "xc"), "a_vs_b", "bayes-factors", "a_vs_b.miso_bf_exact")
    header, rows = read_table(table)
    _, bf_rows = read_table(table[:-len("_exact")])
    assert header == compare.HEADER_FIELDS + ["exact", "log10_bayes_factor"] + ["prob_abs_diff_ge_%g" % t for t in THRESHOLDS]
    assert sorted(rows) == sorted(bf_rows) == sorted("gene%d" % e for e in range(N_GENES))
    # capi's numbers for the same read pairs: whatever the seed
    two = [e for e in range(N_GENES) if e not in K3]
    bs = []
    for s in (0, 1):
        b = miso_amd.Batch(36, paired=True, mean=250.0, var=900.0, exact_paired=True, chains=2, iters=600, burn=100, lag=5)
        for e in two:
            exons, isoforms, pos, cig = events[e][s]
            b.add_event(miso_amd.Gene(exons, isoforms), pos, cig)
        b.run(seed=1 + s, first_event_id=0)
        bs.append(b)
    z = [v for t in THRESHOLDS for v in (t, -t)]
    bs[0].compare_exact_paired(bs[1], z)
    for j, e in enumerate(two):
        row = rows["gene%d" % e]
        got = bs[0].exact_comparison(j)
        assert got is not None, e
        m1, m2, _, bf, l10, H = got
        s1, s2 = bs[0].exact_summary(j, 0.95), bs[1].exact_summary(j, 0.95)
        want = {"sample1_posterior_mean": "%.4f" % s1[0][0], "sample1_ci_low": "%.4f" % s1[1][0], "sample1_ci_high": "%.4f" % s1[2][0],
                "sample2_posterior_mean": "%.4f" % s2[0][0], "sample2_ci_low": "%.4f" % s2[1][0], "sample2_ci_high": "%.4f" % s2[2][0],
                "diff": "%.4f" % (m1 - m2), "bayes_factor": "%.2f" % min(bf, 1e12), "exact": "1", "log10_bayes_factor": "%.4f" % l10}
        for k, t in enumerate(THRESHOLDS):
            want["prob_abs_diff_ge_%g" % t] = "%.4f" % ((1.0 - H[2 * k]) + H[2 * k + 1])
        assert {k: row[k] for k in want} == want, e
        for k in ("isoforms", "sample1_counts", "sample2_counts", "sample1_assigned_counts", "chrom", "strand", "mRNA_starts"):
            assert row[k] == bf_rows["gene%d" % e][k], (e, k)
    # the three-isoform event: its `.miso_bf` fields verbatim, exact = 0 and NA
    for e in K3:
        row, plain = rows["gene%d" % e], bf_rows["gene%d" % e]
        assert all(row[k] == plain[k] for k in plain) and row["exact"] == "0", e
        assert [row[k] for k in header[len(compare.HEADER_FIELDS) + 1:]] == ["NA"] * (1 + len(THRESHOLDS)), e
    # filter_events takes the table (it is defined for two-isoform events: their rows)
    two_table = str(tmp_path / "two.miso_bf_exact")
    text = open(table).read().splitlines(keepends=True)
    open(two_table, "w").write("".join(ln for ln in text if ln.split("\t")[0] not in ["gene%d" % e for e in K3]))
    fdir = str(tmp_path / "filtered")
    assert filter_events.main(["--filter", two_table, "--output-dir", fdir, "--bayes-factor", "5", "--delta-psi", "0.1"]) == 0
    lines = open(os.path.join(fdir, "two.miso_bf_exact.filtered")).read().splitlines()
    want = [r for r in text[1:] if r.split("\t")[0] in ["gene%d" % e for e in two]
            and abs(float(rows[r.split("\t")[0]]["diff"])) >= 0.1 and float(rows[r.split("\t")[0]]["bayes_factor"]) >= 5]
    assert lines[0].split("\t") == header and lines[1:] == [r.rstrip("\n") for r in want]
