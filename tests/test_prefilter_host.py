"""CPU: the semantics of `miso --run --prefilter` -- the checker (tests/_coverage_ref.py) on hand-built cases with their
counts written out, the coverage table's text, its filter and its reuse, and the dispatcher's batch files."""
import os
import subprocess
import sys

import pytest

import _coverage_ref as ref
from miso_amd import exon_utils
from miso_amd.settings import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sam(refs, recs):
    head = "".join("@SQ\tSN:%s\tLN:100000\n" % r for r in refs)
    body = "".join("r%d\t%d\t%s\t%d\t50\t%s\t*\t0\t0\t*\t*\n" % (k, flag, rname, pos0 + 1, cigar)
                   for k, (flag, rname, pos0, cigar) in enumerate(recs))
    return head + body


def _gene(seqid, start, end, gid):
    attrs = "ID=%s" % gid if gid else "Name=none"
    return "%s\tt\tgene\t%d\t%d\t.\t+\t.\t%s" % (seqid, start, end, attrs)


GENES = [("chr1", 101, 200, "g0"),     # outer
         ("chr1", 121, 160, "g1"),     # nested in g0
         ("chr1", 151, 260, "g2"),     # overlaps g0
         ("chr1", 121, 160, "g3"),     # duplicate of g1
         ("chr1", 1001, 1100, "g4"),
         ("chr1", 1201, 1300, "g5"),
         ("chr10", 1, 100, "g6"),      # the file calls it "10"
         ("chrZ", 1, 1000, "g7"),      # a reference the file lacks
         ("chr1", 300, 250, "g8")]     # start > end

RECORDS = [(0, "chr1", 125, "10M"),             # [125,135): inside g0, g1, g3
           (0, "chr1", 165, "20M"),             # [165,185): inside g0, g2
           (0, "chr1", 205, "20M"),             # [205,225): inside g2 only
           (0, "chr1", 110, "10M"),             # [110,120): ends at g1's start - 1: not g1's
           (0, "chr1", 160, "5M"),              # [160,165): begins at g1's end: not g1's
           (0, "chr1", 1010, "10M50N10M"),      # spliced [1010,1080): inside g4
           (0, "chr1", 1050, "20M150N20M"),     # spliced [1050,1240): its gap spans g4's end and g5's start: dropped
           (0, "chr1", 1200, "100M"),           # exactly g5
           (0, "chr1", 1199, "10M"),            # one before g5
           (0, "chr1", 1291, "10M"),            # one past g5
           (4, "chr1", 125, "10M"),             # unmapped with a position
           (4, "*", -1, "*"),                   # unmapped
           (0, "chr1", 130, "*"),               # no reference-consuming operation: span [130,131)
           (256, "chr1", 180, "10M"),           # secondary: counted
           (1024, "chr1", 230, "10M"),          # duplicate: counted
           (0, "10", 5, "20M"),                 # inside g6 once "chr10" resolves to "10"
           (0, "chrX", 5, "20M"),               # a reference no gene names
           (0, "chr1", 250, "20M")]             # overlaps g2 but lies inside no gene: not kept

WANT = {"g0": 6, "g1": 2, "g2": 5, "g3": 2, "g4": 1, "g5": 1, "g6": 1, "g7": 0, "g8": 0}


def _gff_text(genes=GENES):
    return "##gff-version 3\n" + "".join(_gene(*g) + "\n" for g in genes)


def test_checker_on_hand_built_cases():
    sam = _sam(["chr1", "10", "chrX"], RECORDS)
    assert ref.counts(sam, _gff_text()) == [WANT[g[3]] for g in GENES]


def test_checker_chr_prefix_only_where_the_file_lacks_the_name():
    recs = [(0, "chr10", 5, "20M"), (0, "10", 5, "20M"), (0, "10", 7, "20M")]
    # both names in the file: "chr10" stays itself
    assert ref.counts(_sam(["chr10", "10"], recs), _gff_text([("chr10", 1, 100, "a")])) == [1]
    assert ref.counts(_sam(["10"], recs[1:]), _gff_text([("chr10", 1, 100, "a")])) == [2]
    assert ref.counts(_sam(["10"], recs[1:]), _gff_text([("chr11", 1, 100, "a")])) == [0]


def test_checker_kept_record_counts_in_every_overlapping_interval():
    # [95,115) lies inside "wide" only; it overlaps "narrow" [104,110) too, which holds no record whole
    genes = [("chr1", 51, 200, "wide"), ("chr1", 105, 110, "narrow"), ("chr1", 300, 400, "far")]
    sam = _sam(["chr1"], [(0, "chr1", 95, "20M"), (0, "chr1", 100, "3M"), (0, "chr1", 250, "10M")])
    assert ref.counts(sam, _gff_text(genes)) == [2, 1, 0]


def test_table_text_and_lines_that_are_intervals(tmp_path):
    gff = tmp_path / "genes.gff"
    text = _gff_text() + "# a comment\nchr1\tshort\tline\n" + _gene("chr1", 101, 200, "g9") + "\textra\n"
    gff.write_text(text)
    fields = exon_utils.read_coverage_intervals(str(gff))
    assert [f[8] for f in fields] == ["ID=%s" % g[3] for g in GENES] + ["ID=g9"]
    assert fields[-1][9] == "extra"
    sam = _sam(["chr1", "10", "chrX"], RECORDS)
    want = ref.table(sam, text)
    assert exon_utils.format_coverage(fields, ref.counts(sam, text)) == want
    assert want.splitlines()[0] == "chr1\tt\tgene\t101\t200\t.\t+\t.\tID=g0\t6"
    assert want.splitlines()[-1] == "chr1\tt\tgene\t101\t200\t.\t+\t.\tID=g9\textra\t6"


def test_coverage_filename():
    assert exon_utils.coverage_filename("/d/Sample.A.BAM", "/o") == "/o/Sample.A.bed"
    assert exon_utils.coverage_filename("/d/reads.sam", "/o") == "/o/reads.sam.bed"


def test_filter_ids_edges_and_missing_id(tmp_path, capsys):
    lines = [_gene("chr1", 1, 10, "a") + "\t20",
             _gene("chr1", 1, 10, "b") + "\t19",
             _gene("chr1", 1, 10, None) + "\t50",                              # no ID: warned, skipped
             _gene("chr1", 1, 10, None) + "\t3",                               # no ID, too few: silently dropped
             "chr1\tt\tgene\t1\t10\t.\t+\t.\tName=x;ID=c%2Cd,e \t21",           # escaped, first value, trailing blank
             "# comment\t99",
             _gene("chr2", 5, 90, "f") + "\t0"]
    table = tmp_path / "t.bed"
    table.write_text("\n".join(lines) + "\n")
    got = exon_utils.get_ids_passing_filter(str(table), 20)
    want, no_id = ref.passing_ids(table.read_text(), 20)
    assert got == want == ["a", "c,d"]
    assert len(no_id) == 1
    out = capsys.readouterr().out
    assert out.count("WARNING: No ID= found for line:") == 1 and "Name=none\t50" in out
    assert exon_utils.get_ids_passing_filter(str(table), 21) == ref.passing_ids(table.read_text(), 21)[0] == ["c,d"]
    assert exon_utils.get_ids_passing_filter(str(table), 0) == ref.passing_ids(table.read_text(), 0)[0] \
        == ["a", "b", "c,d", "f"]


def test_existing_table_is_reused(tmp_path, capsys):
    bam, gff = tmp_path / "x.bam", tmp_path / "genes.gff"
    bam.write_bytes(b"not read")
    gff.write_text(_gff_text())
    out = tmp_path / "out"
    out.mkdir()
    (out / "x.bed").write_text("kept as it is\n")

    def compute(*args):
        raise AssertionError("an existing table must be reused")
    assert exon_utils.get_bam_gff_coverage(str(bam), str(gff), str(out), compute=compute) == str(out / "x.bed")
    assert "  - File exists. Skipping..." in capsys.readouterr().out
    assert (out / "x.bed").read_text() == "kept as it is\n"
    calls = []
    fresh = tmp_path / "fresh"
    path = exon_utils.get_bam_gff_coverage(str(bam), str(gff), str(fresh), compute=lambda *a: calls.append(a))
    assert path == str(fresh / "x.bed") and calls == [(str(bam), str(gff), path)]


def test_help_lists_prefilter():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "miso_amd.miso", "--help"], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "--prefilter" in r.stdout and "bedtools" not in r.stdout


# ---- the dispatcher, over a table that exists (nothing runs on the device) ----
def _index(tmp_path, n=6):
    from miso_amd import index_gff
    lines = ["##gff-version 3"]
    for g in range(n):
        s = 1000 + 10000 * g
        lines += ["chr1\tx\tgene\t%d\t%d\t.\t+\t.\tID=g%d" % (s, s + 900, g),
                  "chr1\tx\tmRNA\t%d\t%d\t.\t+\t.\tID=g%d.A;Parent=g%d" % (s, s + 900, g, g),
                  "chr1\tx\texon\t%d\t%d\t.\t+\t.\tID=g%d.A.1;Parent=g%d.A" % (s, s + 100, g, g),
                  "chr1\tx\texon\t%d\t%d\t.\t+\t.\tID=g%d.A.2;Parent=g%d.A" % (s + 800, s + 900, g, g)]
    gff = tmp_path / "many.gff"
    gff.write_text("\n".join(lines) + "\n")
    idx = str(tmp_path / "indexed")
    index_gff.index_gff(str(gff), idx)
    return idx


def _table(idx, counts):
    lines = open(os.path.join(idx, "genes.gff")).read().splitlines()
    return "".join("%s\t%d\n" % (l, c) for l, c in zip(lines, counts))


@pytest.fixture
def min_reads_20(tmp_path):
    p = tmp_path / "s.txt"
    p.write_text("[data]\nmin_event_reads = 20\n")
    Settings.load(str(p))
    yield
    Settings.load(None)


def test_dispatcher_keeps_global_numbers(tmp_path, min_reads_20, capsys):
    from miso_amd import miso as miso_cli, run_miso
    idx = _index(tmp_path)
    bam = tmp_path / "reads.bam"
    bam.write_bytes(b"")
    out = tmp_path / "out"
    out.mkdir()
    (out / "reads.bed").write_text(_table(idx, [30, 5, 20, 19, 100, 0]))
    d = miso_cli.GenesDispatcher(idx, str(bam), str(out), 36, 1, num_proc=2, prefilter=True)
    d.apply_prefilter()
    assert "Total of 3 events pass coverage filter." in capsys.readouterr().out
    batches = d.output_batch_files()
    assert [(n, first) for _, n, first in batches] == [(1, 0), (2, 1)]
    cols = [run_miso.read_genes_file_columns(f) for f, _, _ in batches]
    assert [[g for g, _ in e] for e, _, _ in cols] == [["g0"], ["g2", "g4"]]
    assert [numbers for _, numbers, _ in cols] == [[0], [2, 4]]
    assert all(samples is None for _, _, samples in cols)
    assert run_miso.read_genes_file(batches[1][0]) == cols[1][0]
    # without --prefilter the batch files keep their two columns
    plain = miso_cli.GenesDispatcher(idx, str(bam), str(tmp_path / "plain"), 36, 1, num_proc=2)
    for f, _, _ in plain.output_batch_files():
        assert all(len(l.split("\t")) == 2 for l in open(f).read().splitlines())
        assert run_miso.read_genes_file_columns(f)[1:] == (None, None)


def test_dispatcher_compare_marks_the_samples(tmp_path, min_reads_20):
    from miso_amd import miso as miso_cli, run_miso
    idx = _index(tmp_path, n=4)
    b1, b2 = tmp_path / "a.bam", tmp_path / "b.bam"
    b1.write_bytes(b"")
    b2.write_bytes(b"")
    out = tmp_path / "out"
    for lab, counts in (("s1", [30, 5, 40, 0]), ("s2", [25, 0, 3, 0])):
        (out / lab).mkdir(parents=True)
        (out / lab / ("%s.bed" % ("a" if lab == "s1" else "b"))).write_text(_table(idx, counts))
    d = miso_cli.GenesDispatcher(idx, str(b1), str(out), 36, 1, num_proc=1, compare_bam=str(b2), labels=("s1", "s2"),
                                 prefilter=True)
    d.apply_prefilter()
    (f, n, first), = d.output_batch_files()
    entries, numbers, samples = run_miso.read_genes_file_columns(f)
    assert [g for g, _ in entries] == ["g0", "g2"] and numbers == [0, 2] and samples == ["1,2", "1"]


def test_dispatcher_no_event_passes(tmp_path, min_reads_20):
    from miso_amd import miso as miso_cli
    idx = _index(tmp_path, n=3)
    bam = tmp_path / "reads.bam"
    bam.write_bytes(b"")
    out = tmp_path / "out"
    out.mkdir()
    (out / "reads.bed").write_text(_table(idx, [19, 0, 2]))
    d = miso_cli.GenesDispatcher(idx, str(bam), str(out), 36, 1, num_proc=1, prefilter=True)
    with pytest.raises(miso_cli.PrefilterError, match="None of the events in .* appear to meet the read coverage"):
        d.apply_prefilter()


def test_dispatcher_without_genes_gff(tmp_path, min_reads_20, capsys):
    from miso_amd import miso as miso_cli
    idx = _index(tmp_path, n=3)
    os.remove(os.path.join(idx, "genes.gff"))
    bam = tmp_path / "reads.bam"
    bam.write_bytes(b"")
    d = miso_cli.GenesDispatcher(idx, str(bam), str(tmp_path / "out"), 36, 1, num_proc=1, prefilter=True)
    d.apply_prefilter()
    assert "WARNING: Could not find 'genes.gff'" in capsys.readouterr().out
    assert d.gene_ids == ["g0", "g1", "g2"] and d.event_numbers is None


def test_genes_file_columns_must_be_complete(tmp_path):
    from miso_amd import run_miso
    f = tmp_path / "batch.txt"
    f.write_text("a\tx.pickle\t3\nb\ty.pickle\n")
    with pytest.raises(ValueError):
        run_miso.read_genes_file_columns(str(f))
