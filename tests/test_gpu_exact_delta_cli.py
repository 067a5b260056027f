"""GPU: `miso --run INDEX SAM --compare SAM2 ... --exact-compare | --exact-paired-compare --exact-delta-posterior` end to end,
single-end on a 30-event index and paired-end on a six-gene one (the sizes of tests/test_gpu_exact_compare_cli.py and
tests/test_gpu_exact_paired_compare_cli.py): the `.miso_dpsi_exact` table beside the `.miso_bf_exact`, its comparable rows
against capi's own numbers for the same reads (no seed enters them), the other rows with their `.miso_bf` line and NA, and
every other output file byte-identical to a run without the flag."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "miso_amd"))

pytestmark = pytest.mark.gpu

THRESHOLDS = (0.1, 0.25)
SETTINGS = "[data]\nmin_event_reads = 20\n[sampler]\nburn_in = 100\nlag = 5\nnum_iters = 600\nnum_chains = 2\n"
# kind: genes, three-isoform genes (sampled, never exact-comparable), genes below min_event_reads in sample 2 (in no table)
KINDS = {"single": dict(n_genes=30, k3=(7, 19), few=(12,), paired=False),
         "paired": dict(n_genes=6, k3=(2,), few=(), paired=True)}


def run(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    import miso_sampler
    env.pop(miso_sampler.EXACT_PAIRED_ENV, None)
    env.pop("MISO_EXACT", None)
    return subprocess.run([sys.executable] + args, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=600)


def make_inputs(tmp_path, n_genes, k3, few, paired):
    """GFF3 of synthetic genes and one SAM per sample (another expression in sample 2); returns per gene and sample
    (exons, isoforms, pos, cigars) in the gene's own coordinates"""
    from miso_amd import capi, workload
    rng = np.random.default_rng(6 if paired else 5)
    lines, recs, events = ["##gff-version 3"], ([], []), []
    for e in range(n_genes):
        K = 3 if e in k3 else 2
        off = 10000 + e * (9000 if paired else 6000)
        exons, isoforms, expr = workload.event_gene(e, K, min_len=400, max_len=800, gap=300) if paired else workload.event_gene(e, K)
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
            ex_s = expr if s == 0 else expr[::-1].copy()
            if paired:
                n = int(rng.integers(60, 200))
                _, pos, cig = capi.simulate_reads(g, ex_s, n, 36, 8000 + 2 * e + s, 250.0, 900.0)
                assert len(pos) == 2 * n
                for i in range(n):
                    a, b = int(pos[2 * i]) + off, int(pos[2 * i + 1]) + off
                    recs[s].append("p%d_%d\t99\tchr1\t%d\t255\t%s\t=\t%d\t0\t%s\t%s" % (e, i, a, cig[2 * i].decode(), b, "A" * 36, "I" * 36))
                    recs[s].append("p%d_%d\t147\tchr1\t%d\t255\t%s\t=\t%d\t0\t%s\t%s" % (e, i, b, cig[2 * i + 1].decode(), a, "A" * 36, "I" * 36))
            else:
                n = 15 if (s == 1 and e in few) else int(rng.integers(40, 160))
                _, pos, cig = capi.simulate_reads(g, ex_s, n, 36, 6000 + 2 * e + s)
                recs[s].extend("r%d_%d\t0\tchr1\t%d\t255\t%s\t*\t0\t0\t%s\t%s" % (e, i, pos[i] + off, cig[i].decode(), "A" * 36, "I" * 36)
                               for i in range(len(pos)))
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


def all_files(top):
    out = {}
    for d, subdirs, names in os.walk(top):
        subdirs[:] = [s for s in subdirs if s not in ("batch-logs", "batch-genes")]      # (time stamps in names and text)
        for f in names:
            out[os.path.relpath(os.path.join(d, f), top)] = open(os.path.join(d, f), "rb").read()
    return out


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_exact_delta_table_end_to_end(tmp_path, kind):
    import miso_amd
    from miso_amd import compare
    n_genes, k3, few, paired = (KINDS[kind][k] for k in ("n_genes", "k3", "few", "paired"))
    gff, sams, events = make_inputs(tmp_path, n_genes, k3, few, paired)
    settings = tmp_path / "s.txt"
    settings.write_text(SETTINGS)
    idx = str(tmp_path / "idx")
    assert run(["-m", "miso_amd.index_gff", "--index", gff, idx]).returncode == 0
    mode = (["--paired-end", "250", "30", "--exact-paired", "--exact-paired-compare"] if paired else ["--exact", "--exact-compare"])
    outs = {}
    for name, extra in (("without", []), ("with", ["--exact-delta-posterior"])):
        out = str(tmp_path / name)
        r = run(["-m", "miso_amd.miso", "--run", idx, sams[0], "--compare", sams[1], "--labels", "a", "b", "--output-dir", out,
                 "--read-len", "36", "--settings-filename", str(settings), "-p", "1", "--seed", "77", "--delta-psi-thresholds"]
                + ["%g" % t for t in THRESHOLDS] + mode + extra)
        logs = "".join(open(os.path.join(out, "batch-logs", f)).read() for f in os.listdir(os.path.join(out, "batch-logs")))
        assert r.returncode == 0, r.stdout + logs
        outs[name] = all_files(out)
    # the flag adds one file and changes no other byte
    new = os.path.join("a_vs_b", "bayes-factors", "a_vs_b.miso_dpsi_exact")
    assert sorted(outs["with"]) == sorted(list(outs["without"]) + [new])
    assert all(outs["with"][f] == data for f, data in outs["without"].items())
    assert any(f.endswith(".miso_bf_exact") for f in outs["without"]) and any(f.endswith(".miso") for f in outs["without"])
    table = os.path.join(str(tmp_path / "with"), new)
    header, rows = read_table(table)
    _, bf_rows = read_table(table[:-len(".miso_dpsi_exact")] + ".miso_bf")
    _, x_rows = read_table(table[:-len(".miso_dpsi_exact")] + ".miso_bf_exact")
    assert header == compare.HEADER_FIELDS + ["exact"] + compare.DPSI_FIELDS + ["prob_abs_diff_ge_%g" % t for t in THRESHOLDS]
    kept = [e for e in range(n_genes) if e not in few]
    assert sorted(rows) == sorted(bf_rows) == sorted("gene%d" % e for e in kept)
    # capi's numbers for the same reads: whatever the seed
    two = [e for e in kept if e not in k3]
    bs = []
    for s in (0, 1):
        shape = dict(chains=2, iters=600, burn=100, lag=5)
        b = (miso_amd.Batch(36, paired=True, mean=250.0, var=900.0, exact_paired=True, **shape) if paired
             else miso_amd.Batch(36, exact=True, **shape))
        for e in two:
            exons, isoforms, pos, cig = events[e][s]
            b.add_event(miso_amd.Gene(exons, isoforms), pos, cig)
        b.run(seed=1 + s, first_event_id=0)
        bs.append(b)
    z = [v for t in THRESHOLDS for v in (t, -t)]
    (bs[0].compare_exact_paired if paired else bs[0].compare_exact)(bs[1], z)
    bs[0].exact_delta_quantiles(bs[1], (0.5, 0.025, 0.975))
    for j, e in enumerate(two):
        row = rows["gene%d" % e]
        got = bs[0].exact_delta(j)
        assert got is not None, e
        q, h0 = got
        want = {"exact": "1", "delta_psi_median": "%.4f" % q[0], "delta_psi_ci_low": "%.4f" % q[1], "delta_psi_ci_high": "%.4f" % q[2],
                "prob_diff_gt_0": "%.4f" % (1.0 - h0), "prob_diff_lt_0": "%.4f" % h0}
        assert {k: row[k] for k in want} == want, e
        # the rest of the row is the `.miso_bf_exact` row's
        for k in compare.HEADER_FIELDS + ["prob_abs_diff_ge_%g" % t for t in THRESHOLDS]:
            assert row[k] == x_rows["gene%d" % e][k], (e, k)
        assert float(row["delta_psi_ci_low"]) <= float(row["delta_psi_median"]) <= float(row["delta_psi_ci_high"])
    # every other event: its `.miso_bf` fields verbatim, exact = 0 and NA
    for e in k3:
        row, plain = rows["gene%d" % e], bf_rows["gene%d" % e]
        assert all(row[k] == plain[k] for k in plain) and row["exact"] == "0", e
        assert [row[k] for k in header[len(compare.HEADER_FIELDS) + 1:]] == ["NA"] * (5 + len(THRESHOLDS)), e
