"""GPU: `miso --run --prefilter` -- the coverage pass (csrc/kernels_coverage.hip) against the restatement in
tests/_coverage_ref.py for SAM, BAM and unsorted input at several chunk sizes, and the run end to end: filtered batch
files, kept events byte-identical to a run without the prefilter, table reuse, no passing event, --compare and an
index without genes.gff."""
import os
import random
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _coverage_ref as ref
from _bam import sam_to_bam
from miso_amd import capi, exon_utils, sam_utils

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible")


def run(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable] + args, env=env, cwd=ROOT, stdout=subprocess.PIPE,
                          stderr=subprocess.STDOUT, text=True, timeout=600)


# ---- the device pass against the checker ----
@pytest.fixture(scope="module")
def random_case(tmp_path_factory):
    """~10^5 records over 300 genes on three references (GFF "chr2" is the file's "2"), long, nested and duplicate
    genes among them; flags and CIGARs of every kind the rules name."""
    rng = random.Random(5)
    d = tmp_path_factory.mktemp("coverage")
    refs = ["chr1", "2", "chr3"]
    genes = []
    for g in range(300):
        seqid = rng.choice(["chr1", "chr2", "chr3"])
        r = rng.random()
        if r < 0.1 and genes:                               # nested in an earlier gene of any reference
            seqid, s, e = genes[rng.randrange(len(genes))]
            start = rng.randint(s, e)
            end = rng.randint(start, e)
        elif r < 0.15 and genes:                            # a duplicate
            seqid, start, end = genes[rng.randrange(len(genes))][:3]
        else:
            start = rng.randint(1, 2000000)
            end = start + (rng.randint(100000, 400000) if r > 0.97 else rng.randint(300, 20000))
        genes.append((seqid, start, end))
    genes.append(("chr9", 1, 3000000))                      # a reference the file lacks
    genes.append(("chr1", 5000, 4000))                      # start > end
    gff = "##gff-version 3\n" + "".join("%s\tt\tgene\t%d\t%d\t.\t+\t.\tID=gene%03d\n" % (s, a, b, k)
                                        for k, (s, a, b) in enumerate(genes))
    recs = []
    for i in range(100000):
        if rng.random() < 0.6:                              # near a gene
            seqid, s, e = genes[rng.randrange(300)]
            name = "2" if seqid == "chr2" else seqid
            pos0 = max(0, rng.randint(s - 200, e + 50) - 1)
        else:
            name, pos0 = rng.choice(refs), rng.randint(0, 2400000)
        u = rng.random()
        cigar = "50M" if u < 0.6 else "20M%dN30M" % rng.randint(10, 3000) if u < 0.8 else \
            "10S40M" if u < 0.9 else "*" if u < 0.93 else "30M5D20M"
        flag = rng.choice([0, 0, 0, 16, 256, 1024, 512, 4, 99, 147])
        if flag & 4 and rng.random() < 0.5:
            name, pos0, cigar = "*", -1, "*"
        recs.append("q%d\t%d\t%s\t%d\t50\t%s\t*\t0\t0\t*\t*" % (i, flag, name, pos0 + 1, cigar))
    head = "".join("@SQ\tSN:%s\tLN:3000000\n" % r for r in refs)
    sam = head + "\n".join(recs) + "\n"
    recs_shuffled = list(recs)
    rng.shuffle(recs_shuffled)
    shuffled = head + "\n".join(recs_shuffled) + "\n"
    paths = {"sam": str(d / "reads.sam"), "bam": str(d / "reads.bam"), "shuffled": str(d / "shuffled.sam")}
    open(paths["sam"], "w").write(sam)
    open(paths["shuffled"], "w").write(shuffled)
    sam_to_bam(sam, paths["bam"], block=60000)
    gff_path = str(d / "genes.gff")
    open(gff_path, "w").write(gff)
    return paths, gff_path, gff, ref.counts(sam, gff), ref.table(sam, gff)


@pytest.mark.parametrize("which", ["sam", "bam", "shuffled"])
def test_region_counts_equal_the_checker(random_case, which, tmp_path):
    paths, gff_path, gff, want, want_table = random_case
    f = sam_utils.Samfile(paths[which])
    intervals = exon_utils.read_coverage_intervals(gff_path)
    seen = []
    for chunk in (1000, 4096, 0):
        got, st = exon_utils.coverage_counts(f, intervals, chunk_records=chunk)
        assert got.dtype == np.int64 and list(got) == want, chunk
        assert st["chunks"] == (len(f) + (chunk or 1 << 22) - 1) // (chunk or 1 << 22)
        seen.append(st["kept"])
    assert len(set(seen)) == 1 and 0 < seen[0] < len(f)
    assert sum(1 for c in want if c > 0) > 150
    # the table: the checker's, line for line
    out = str(tmp_path / which)
    os.makedirs(out)
    table = exon_utils.get_bam_gff_coverage(paths[which], gff_path, out)
    assert table == exon_utils.coverage_filename(paths[which], out)
    assert open(table).read().splitlines() == want_table.splitlines()


def test_region_counts_raw_names_and_empty(random_case):
    paths, _, _, _, _ = random_case
    f = sam_utils.Samfile(paths["sam"])
    got, st = capi.region_counts(f, [], [], [])
    assert len(got) == 0 and st["kept"] == 0
    # the C ABI matches names exactly: "chr2" is not the file's "2" (exon_utils resolves it first)
    got, _ = capi.region_counts(f, ["chr2", "2"], [1, 1], [3000000, 3000000])
    assert got[0] == 0 and got[1] > 0


# ---- end to end ----
def _seven_genes(tmp_path, tag, small=(2, 5), seqid="chr1"):
    """GFF3 + SAM of 7 synthetic genes; the genes in `small` get 15 reads (below min_event_reads = 20)."""
    from miso_amd import workload
    gff, sam = tmp_path / ("g%s.gff" % tag), tmp_path / ("r%s.sam" % tag)
    lines, recs = ["##gff-version 3"], []
    for e in range(7):
        off = 10000 + e * 6000
        exons, isoforms, pos, cig = workload.event_reads(e, 2 + (e % 3), 15 if e in small else 300)
        ex = [(s + off, t + off) for s, t in exons]
        gid = "gene%d" % e
        lines.append("%s\tx\tgene\t%d\t%d\t.\t+\t.\tID=%s" % (seqid, ex[0][0], ex[-1][1], gid))
        for m, iso in enumerate(isoforms):
            tid = "%s.t%d" % (gid, m)
            lines.append("%s\tx\tmRNA\t%d\t%d\t.\t+\t.\tID=%s;Parent=%s" % (seqid, ex[iso[0]][0], ex[iso[-1]][1], tid, gid))
            lines += ["%s\tx\texon\t%d\t%d\t.\t+\t.\tID=%s.e%d;Parent=%s" % (seqid, ex[x][0], ex[x][1], tid, x, tid)
                      for x in iso]
        recs += ["r%d_%d\t0\tchr1\t%d\t255\t%s\t*\t0\t0\t%s\t%s" % (e, i, pos[i] + off, cig[i].decode(), "A" * 36, "I" * 36)
                 for i in range(len(pos))]
    gff.write_text("\n".join(lines) + "\n")
    sam.write_text("@SQ\tSN:chr1\tLN:100000\n" + "\n".join(recs) + "\n")
    return gff, sam


def _setup(tmp_path, **kw):
    gff, sam = _seven_genes(tmp_path, "", **kw)
    settings = tmp_path / "s.txt"
    settings.write_text("[data]\nmin_event_reads = 20\n[sampler]\nburn_in = 100\nlag = 5\nnum_iters = 600\nnum_chains = 2\n")
    idx = str(tmp_path / "idx")
    assert run(["-m", "miso_amd.index_gff", "--index", str(gff), idx]).returncode == 0
    return idx, str(sam), str(settings)


def _miso(idx, sam, settings, out, nproc, *extra):
    return run(["-m", "miso_amd.miso", "--run", idx, sam, "--output-dir", out, "--read-len", "36",
                "--settings-filename", settings, "-p", str(nproc), "--seed", "77"] + list(extra))


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))} if os.path.isdir(d) else {}


def _batch_genes(out):
    d = os.path.join(out, "batch-genes")
    return sorted(l.split("\t")[0] for f in os.listdir(d) for l in open(os.path.join(d, f)).read().splitlines())


def test_prefilter_end_to_end(tmp_path):
    idx, sam, settings = _setup(tmp_path)
    plain = str(tmp_path / "plain")
    r = _miso(idx, sam, settings, plain, 1)
    assert r.returncode == 0, r.stdout
    want = _files(os.path.join(plain, "chr1"))
    kept = ["gene%d" % e for e in (0, 1, 3, 4, 6)]
    assert sorted(want) == [g + ".miso" for g in kept]
    for nproc in (1, 3):
        out = str(tmp_path / ("pre%d" % nproc))
        r = _miso(idx, sam, settings, out, nproc, "--prefilter")
        assert r.returncode == 0, r.stdout
        assert "Total of 5 events pass coverage filter." in r.stdout
        assert _batch_genes(out) == kept                                  # gene2, gene5 never dispatched
        assert _files(os.path.join(out, "chr1")) == want, nproc
        table = os.path.join(out, "r.sam.bed")
        assert open(table).read() == ref.table(open(sam).read(), open(os.path.join(idx, "genes.gff")).read())
    # a second run into a fresh directory that holds an edited copy of the table: reused, gene0 not run
    lines = open(table).read().splitlines()
    lines = [l.rsplit("\t", 1)[0] + "\t0" if "ID=gene0" in l else l for l in lines]
    again = str(tmp_path / "again")
    os.makedirs(again)
    open(os.path.join(again, "r.sam.bed"), "w").write("\n".join(lines) + "\n")
    r = _miso(idx, sam, settings, again, 2, "--prefilter")
    assert r.returncode == 0, r.stdout
    assert "File exists. Skipping..." in r.stdout and "Total of 4 events pass coverage filter." in r.stdout
    assert _batch_genes(again) == kept[1:]
    assert _files(os.path.join(again, "chr1")) == {k: v for k, v in want.items() if k != "gene0.miso"}


def test_prefilter_no_event_passes(tmp_path):
    idx, sam, settings = _setup(tmp_path, seqid="scaffold7")      # no reference of the file, even after "chr"
    out = str(tmp_path / "out")
    r = _miso(idx, sam, settings, out, 1, "--prefilter")
    assert r.returncode == 1, r.stdout
    assert "None of the events in %s appear to meet the read coverage filter" % idx in r.stdout
    assert os.listdir(os.path.join(out, "batch-logs")) == []
    assert not [f for _, _, fs in os.walk(out) for f in fs if f.endswith(".miso")]


def test_prefilter_compare(tmp_path):
    """gene5 passes the coverage filter in sample 1 only and gene2 in sample 2 only: each is sampled in that sample's
    directory alone and left out of the .miso_bf table; every other file is the one the run without --prefilter
    writes, and each sample's table is the one a run on that file alone writes."""
    gff, sam1 = _seven_genes(tmp_path, "1", small=(2,))
    _, sam2 = _seven_genes(tmp_path, "2", small=(5,))
    settings = tmp_path / "s.txt"
    settings.write_text("[data]\nmin_event_reads = 20\n[sampler]\nburn_in = 100\nlag = 5\nnum_iters = 600\nnum_chains = 2\n")
    idx = str(tmp_path / "idx")
    assert run(["-m", "miso_amd.index_gff", "--index", str(gff), idx]).returncode == 0
    outs = {}
    for name, extra in (("plain", []), ("pre", ["--prefilter"])):
        out = str(tmp_path / name)
        r = _miso(idx, str(sam1), str(settings), out, 2, "--compare", str(sam2), "--labels", "a", "b", *extra)
        assert r.returncode == 0, r.stdout
        files = {}
        for lab in ("a", "b"):
            files.update({lab + "/" + f: v for f, v in _files(os.path.join(out, lab, "chr1")).items()})
        files["bf"] = open(os.path.join(out, "a_vs_b", "bayes-factors", "a_vs_b.miso_bf"), "rb").read()
        outs[name] = files
    both = [e for e in range(7) if e not in (2, 5)]
    assert sorted(outs["plain"]) == sorted(["a/gene%d.miso" % e for e in both] + ["b/gene%d.miso" % e for e in both]
                                           + ["bf"])
    assert sorted(set(outs["pre"]) - set(outs["plain"])) == ["a/gene5.miso", "b/gene2.miso"]
    assert {k: v for k, v in outs["pre"].items() if k in outs["plain"]} == outs["plain"]
    assert b"gene5" not in outs["pre"]["bf"] and b"gene2" not in outs["pre"]["bf"]
    # sample 1 alone with --prefilter: the same table, the same gene5
    alone = str(tmp_path / "alone")
    r = _miso(idx, str(sam1), str(settings), alone, 1, "--prefilter")
    assert r.returncode == 0, r.stdout
    pre = str(tmp_path / "pre")
    assert open(os.path.join(pre, "a", "r1.sam.bed")).read() == open(os.path.join(alone, "r1.sam.bed")).read()
    assert os.path.isfile(os.path.join(pre, "b", "r2.sam.bed"))
    assert open(os.path.join(alone, "chr1", "gene5.miso"), "rb").read() == outs["pre"]["a/gene5.miso"]


def test_prefilter_without_genes_gff(tmp_path):
    idx, sam, settings = _setup(tmp_path)
    os.remove(os.path.join(idx, "genes.gff"))
    plain, pre = str(tmp_path / "plain"), str(tmp_path / "pre")
    r = _miso(idx, sam, settings, plain, 1)
    assert r.returncode == 0, r.stdout
    r = _miso(idx, sam, settings, pre, 1, "--prefilter")
    assert r.returncode == 0, r.stdout
    assert "WARNING: Could not find 'genes.gff'" in r.stdout
    assert _files(os.path.join(pre, "chr1")) == _files(os.path.join(plain, "chr1")) != {}
    assert not os.path.exists(os.path.join(pre, "r.sam.bed"))
    shutil.rmtree(plain)
