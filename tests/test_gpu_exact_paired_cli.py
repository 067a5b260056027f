"""GPU: `miso --run INDEX SAM --paired-end 250 30 [--exact-paired]` end to end on a four-gene index and a synthetic paired
SAM file: the same file tree with and without the flag; without it the chains run as always (and a settings file that
spells the key out as False changes no byte); with it the two-isoform events' `.miso` files parse, carry
percent_accept=100 and a mean within the sampler run's Monte-Carlo bound, and the three-isoform gene's file is the same
bytes as without the flag."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "miso_amd"))

pytestmark = pytest.mark.gpu

N_GENES = 4
K3 = (2,)               # a three-isoform gene: sampled in both runs
SETTINGS = "[data]\nmin_event_reads = 20\n[sampler]\nburn_in = 500\nlag = 5\nnum_iters = 2500\nnum_chains = 2\n"
ROWS = 2 * (2500 - 500) // 5


def run(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    import miso_sampler
    env.pop(miso_sampler.EXACT_PAIRED_ENV, None)
    env.pop("MISO_EXACT", None)
    return subprocess.run([sys.executable] + args, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=600)


def make_inputs(tmp_path):
    from miso_amd import capi, workload
    rng = np.random.default_rng(4)
    lines, recs = ["##gff-version 3"], []
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
        n = int(rng.integers(150, 320))
        _, pos, cig = capi.simulate_reads(g, expr, n, 36, 7000 + e, 250.0, 900.0)
        assert len(pos) == 2 * n
        for i in range(n):
            a, b = int(pos[2 * i]) + off, int(pos[2 * i + 1]) + off
            recs.append("p%d_%d\t99\tchr1\t%d\t255\t%s\t=\t%d\t0\t%s\t%s" % (e, i, a, cig[2 * i].decode(), b, "A" * 36, "I" * 36))
            recs.append("p%d_%d\t147\tchr1\t%d\t255\t%s\t=\t%d\t0\t%s\t%s" % (e, i, b, cig[2 * i + 1].decode(), a, "A" * 36, "I" * 36))
    gff, sam = tmp_path / "g.gff", tmp_path / "r.sam"
    gff.write_text("\n".join(lines) + "\n")
    sam.write_text("@SQ\tSN:chr1\tLN:250000\n" + "\n".join(recs) + "\n")
    return str(gff), str(sam)


def test_miso_run_exact_paired_end_to_end(tmp_path):
    import miso_sampler
    gff, sam = make_inputs(tmp_path)
    idx = str(tmp_path / "idx")
    assert run(["-m", "miso_amd.index_gff", "--index", gff, idx]).returncode == 0
    plain_settings, off_settings = tmp_path / "s.txt", tmp_path / "s_off.txt"
    plain_settings.write_text(SETTINGS)
    off_settings.write_text(SETTINGS + "exact_paired = False\n")
    outs = {}
    for name, settings, flag in (("default", plain_settings, []), ("off", off_settings, []), ("exact", plain_settings, ["--exact-paired"])):
        out = str(tmp_path / name)
        r = run(["-m", "miso_amd.miso", "--run", idx, sam, "--output-dir", out, "--read-len", "36", "--paired-end", "250", "30",
                 "--settings-filename", str(settings), "-p", "1", "--seed", "19"] + flag)
        logs = "".join(open(os.path.join(out, "batch-logs", f)).read() for f in os.listdir(os.path.join(out, "batch-logs")))
        assert r.returncode == 0, r.stdout + logs
        d = os.path.join(out, "chr1")
        outs[name] = {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}
    want = ["gene%d.miso" % e for e in range(N_GENES)]
    assert sorted(outs["default"]) == sorted(outs["exact"]) == sorted(outs["off"]) == want
    # without the flag: the run of always, whatever way the switch is left off
    assert outs["default"] == outs["off"]
    for e in range(N_GENES):
        f = "gene%d.miso" % e
        d_samples, d_hdr, _ = miso_sampler.load_samples(os.path.join(str(tmp_path / "default"), "chr1", f))
        e_samples, e_hdr, _ = miso_sampler.load_samples(os.path.join(str(tmp_path / "exact"), "chr1", f))
        if e in K3:
            assert outs["exact"][f] == outs["default"][f]          # not the mode's event: the same bytes
            continue
        assert e_samples.shape == d_samples.shape == (ROWS, 2)
        assert float(e_hdr["percent_accept"]) == 100.0 and float(d_hdr["percent_accept"]) < 100.0
        for key in ("counts", "iters", "burn_in", "lag", "chrom", "strand", "mRNA_starts", "mRNA_ends"):
            assert e_hdr[key] == d_hdr[key], key
        assert np.allclose(e_samples.sum(1), 1.0, atol=1.01e-4) and (e_samples >= 0).all()
        # 4 se + 2e-3, the standard error of the sampler run's mean from eight consecutive blocks of its rows (each holds
        # both chains), the exact rows' own from their variance
        blocks = d_samples[:, 0].reshape(8, ROWS // 8).mean(1)
        se = np.sqrt(blocks.var(ddof=1) / 8 + e_samples[:, 0].var(ddof=1) / ROWS)
        print("gene%d: exact %.5f, default %.5f, se %.5f" % (e, e_samples[:, 0].mean(), d_samples[:, 0].mean(), se))
        assert abs(e_samples[:, 0].mean() - d_samples[:, 0].mean()) < 4 * se + 2e-3
