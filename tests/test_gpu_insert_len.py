"""GPU: `pe_utils --compute-insert-len` (csrc/kernels_insert.hip) against the restatement in tests/_insert_len_ref.py --
the record codes, the pair counts, every region's inserts and the file's text, SAM and BAM, across chunk boundaries,
and the statistics of a million records of known fragment length distribution."""
import gzip
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import _insert_len_ref as ref
from _bam import sam_to_bam
from miso_amd import capi, exon_utils, pe_utils, sam_utils

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
ATP2B1_GFF = os.path.join(DATA, "Atp2b1.mm9.gff")
COUNTS = ("kept", "skipped", "unpaired", "same_strand", "nonpositive", "tagged")


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible")


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def _sam_line(name, flag, rname, pos0, cigar, seq_len=None):
    seq = "A" * seq_len if seq_len else "*"
    return "%s\t%d\t%s\t%d\t50\t%s\t=\t1\t0\t%s\t*" % (name, flag, rname, pos0 + 1, cigar, seq)


def _header(refs):
    return "".join("@SQ\tSN:%s\tLN:100000000\n" % r for r in refs)


def _gff(intervals):
    return "##gff-version 3\n" + "".join("%s\tt\texon\t%d\t%d\t.\t%s\t.\tID=x%d\n" % (s, a, b, st, k)
                                         for k, (s, a, b, st) in enumerate(intervals))


def _check_end_to_end(path, sam_text, gff_path, filter_reads=True, chunk_records=0, tmp_path=None):
    """Counts, regions and (when anything is kept) the file text of the GPU pass == the checker's."""
    intervals = pe_utils.read_intervals(gff_path)
    check_iv = ref.gff_intervals(open(gff_path).read())
    f = sam_utils.Samfile(path)
    got, st = pe_utils.insert_lengths(f, intervals, filter_reads=filter_reads, chunk_records=chunk_records)
    want, counts = ref.insert_len(ref.parse_sam(sam_text), check_iv, filter_reads=filter_reads)
    assert {k: st[k] for k in COUNTS} == counts
    assert list(got) == [check_iv[k].name() for k in want]
    assert [list(map(int, v)) for v in got.values()] == list(want.values())
    text = None
    if counts["kept"]:
        out = str(tmp_path / ("o%d.insert_len" % chunk_records))
        stats = pe_utils.summarize_insert_len_dist(got, out, sd_max=2)
        want_text, want_stats = ref.summarize(want, check_iv)
        text = open(out).read()
        assert text.splitlines()[0] == want_text.splitlines()[0]
        assert text == want_text
        assert stats[3] == want_stats[3]
    return counts, text


# ---- record codes ----
def _tagging_case():
    ivs = [("chr1", 101, 200, "+"),     # 0: outer
           ("chr1", 121, 160, "-"),     # 1: nested in 0
           ("chr1", 151, 260, "+"),     # 2: overlaps 0
           ("chr1", 121, 160, "-"),     # 3: duplicate of 1
           ("chr1", 1001, 1100, "+"),   # 4: alone
           ("chr2", 1, 50, "+"),        # 5
           ("chrZ", 1, 1000, "+")]      # 6: a reference the file does not name
    lines = []
    k = 0

    def rec(rname, pos0, cigar, flag=99):
        nonlocal k
        lines.append(_sam_line("r%d" % k, flag, rname, pos0, cigar))
        k += 1
    for pos0, n in ((100, 100), (99, 100), (100, 101), (101, 100), (100, 99), (101, 99)):
        rec("chr1", pos0, "%dM" % n)                            # both boundaries of interval 0, one past each
    for pos0, n in ((1000, 100), (999, 10), (1090, 10), (1090, 11), (1000, 1)):
        rec("chr1", pos0, "%dM" % n)                            # interval 4's boundaries
    rec("chr1", 125, "10M")                                     # inside 0, 1 and 3
    rec("chr1", 165, "20M")                                     # inside 0 and 2
    rec("chr1", 205, "20M")                                     # inside 2 only
    rec("chr1", 110, "10M30N10M")                               # spliced span 110-160: 0 only
    rec("chr1", 110, "5S10M")                                   # soft clip: reference span only
    rec("chr1", 120, "20M", flag=99 | 0x4)                      # unmapped with a position
    rec("*", -1, "*", flag=77)                                  # unmapped, no reference
    rec("chr1", 130, "*", flag=99)                              # no CIGAR: span pos + 1
    rec("chr2", 0, "50M")                                       # exactly interval 5
    rec("chr2", 0, "51M")
    rec("chrX", 100, "20M")                                     # a reference no interval names
    rec("chr1", 120, "20M", flag=0x200 | 99)                    # QC fail: tagged, filtered
    rec("chr1", 120, "20M", flag=99 | 0x8)                      # mate unmapped
    rec("chr1", 120, "20M", flag=0)                             # not paired
    sam = _header(["chr1", "chr2", "chrX"]) + "\n".join(lines) + "\n"
    return ivs, sam


@pytest.mark.parametrize("as_bam", [False, True])
def test_record_codes(tmp_path, as_bam):
    ivs, sam = _tagging_case()
    gff = _write(tmp_path, "iv.gff", _gff(ivs))
    path = _write(tmp_path, "t.sam", sam)
    if as_bam:
        path = str(tmp_path / "t.bam")
        sam_to_bam(sam, path, block=300)
    f = sam_utils.Samfile(path)
    intervals = pe_utils.read_intervals(gff)
    recs = ref.parse_sam(sam)
    for filter_reads in (True, False):
        want = ref.record_codes(recs, ref.gff_intervals(open(gff).read()), filter_reads=filter_reads)
        for chunk in (0, 1, 4, 7):
            got = capi.insert_tag_records(f, [r.seqid for r in intervals], [r.start for r in intervals],
                                          [r.end for r in intervals], filter_reads=filter_reads, chunk_records=chunk)
            assert [int(c) for c in got] == want, (filter_reads, chunk)
    tags = [c & capi.MISO_INSERT_TAG_MASK for c in want]
    assert tags[0] == 0 and tags[1] == tags[2] == capi.MISO_INSERT_TAG_NONE
    assert ref.TAG_MULTI in tags and 4 in tags and 5 in tags


# ---- end to end ----
@pytest.fixture(scope="module")
def atp2b1(tmp_path_factory):
    d = tmp_path_factory.mktemp("atp2b1")
    with gzip.open(os.path.join(DATA, "c2c12.Atp2b1.sam.gz"), "rt") as fh:
        sam = fh.read()
    sam_path = str(d / "c2c12.Atp2b1.sam")
    open(sam_path, "w").write(sam)
    bam_path = str(d / "c2c12.Atp2b1.bam")
    sam_to_bam(sam, bam_path, block=20000)
    _, gff = exon_utils.get_const_exons_by_gene(ATP2B1_GFF, str(d), min_size=20)
    return sam, sam_path, bam_path, gff


@pytest.mark.parametrize("which", ["sam", "bam"])
def test_atp2b1_end_to_end(atp2b1, which, tmp_path):
    sam, sam_path, bam_path, gff = atp2b1
    counts, text = _check_end_to_end(sam_path if which == "sam" else bam_path, sam, gff, tmp_path=tmp_path)
    assert len(pe_utils.read_intervals(gff)) == 5
    assert counts["kept"] >= 100, counts          # not an empty case
    assert text.startswith("#mean=")


def _pairs_case():
    """Spliced and soft-clipped mates, same strand, groups of 1 and 3, /1 /2 names, QC-fail and mate-unmapped flags, a
    pair across two intervals and one in nested intervals, and a name-sorted stretch (right mate first: insert <= 0)."""
    ivs = [("chr1", 1001, 3000, "+"), ("chr1", 5001, 7000, "-"), ("chr1", 5101, 5300, "-"), ("chr2", 1, 4000, ".")]
    L = []
    pair = lambda n, a, b, ca="50M", cb="50M", fa=99, fb=147, r="chr1": L.extend(
        [_sam_line(n, fa, r, a, ca), _sam_line(n, fb, r, b, cb)])
    pair("ok1", 1100, 1300)
    pair("ok2/1", 1200, 1500)                                    # /1 /2: one name
    L[-1] = _sam_line("ok2/2", 147, "chr1", 1500, "50M")
    pair("ok3", 100, 400, r="chr2")
    pair("ok4", 5400, 5600)
    pair("splice", 1100, 1300, cb="20M100N30M")
    pair("clip", 1100, 1300, ca="5S45M")
    pair("same", 1100, 1300, fa=99, fb=131)                     # both forward
    pair("across", 2900, 5050)                                   # left in 0, right in 1 (left ends past 0? no: 2900+50)
    pair("nested", 5150, 5600)                                   # left in 1 and 2: two tags
    pair("qc", 1100, 1300, fa=99 | 0x200)
    pair("mu", 1100, 1300, fb=147 | 0x8)
    pair("unp", 1100, 1300, fa=97 & ~0x1, fb=145 & ~0x1)         # not flagged paired
    L.append(_sam_line("single", 99, "chr1", 1700, "50M"))
    pair("three", 1800, 1900)
    L.append(_sam_line("three", 147, "chr1", 2000, "50M"))
    pair("outside", 100, 300)                                    # no interval on chr1 there
    pair("ok5", 2100, 2200)
    for k in range(4):                                           # name-sorted: the right mate comes first
        pair("neg%d" % k, 1500 + 40 * k, 1400, fa=147, fb=99)
    pair("zero", 1450, 1400, ca="50M", cb="50M", fa=147, fb=99)  # insert 1400 + 50 - 1450 = 0
    return ivs, _header(["chr1", "chr2"]) + "\n".join(L) + "\n"


@pytest.mark.parametrize("filter_reads", [True, False])
@pytest.mark.parametrize("as_bam", [False, True])
def test_synthetic_pairs(tmp_path, filter_reads, as_bam):
    ivs, sam = _pairs_case()
    gff = _write(tmp_path, "p.gff", _gff(ivs))
    path = _write(tmp_path, "p.sam", sam)
    if as_bam:
        path = str(tmp_path / "p.bam")
        sam_to_bam(sam, path, block=500)
    counts, _ = _check_end_to_end(path, sam, gff, filter_reads=filter_reads, tmp_path=tmp_path)
    assert counts["kept"] == 5 + (3 if not filter_reads else 0)  # qc, mu, unp pair when the filter is off
    assert counts["nonpositive"] == 5 and counts["same_strand"] == 1 and counts["skipped"] >= 4
    assert counts["unpaired"] >= 2


def test_chunk_boundaries(tmp_path):
    """Mates split across chunks, a mate at every chunk's first and last index."""
    ivs = [("chr1", 1, 100000, "+"), ("chr1", 200001, 300000, "+")]
    lines = [_sam_line("lone", 99, "chr1", 50, "50M")]
    rng = np.random.default_rng(3)
    for k in range(40):
        base = 200000 * (k % 2) + int(rng.integers(100, 90000))
        lines += [_sam_line("m%d" % k, 99, "chr1", base, "50M"),
                  _sam_line("m%d" % k, 147, "chr1", base + int(rng.integers(60, 400)), "50M")]
    lines.append(_sam_line("lone2", 99, "chr1", 500, "50M"))
    sam = _header(["chr1"]) + "\n".join(lines) + "\n"
    gff = _write(tmp_path, "c.gff", _gff(ivs))
    path = _write(tmp_path, "c.sam", sam)
    texts = set()
    for chunk in (1, 2, 3, 4, 5, 16, 0):
        counts, text = _check_end_to_end(path, sam, gff, chunk_records=chunk, tmp_path=tmp_path)
        assert counts["kept"] == 40 and counts["unpaired"] == 2
        texts.add(text)
    assert len(texts) == 1


def test_statistics_million_records(tmp_path):
    """Fragments ~ N(250, 30^2) inside exons of 6 kb, 5 * 10^5 pairs: the filter at 2 sd leaves the normal truncated at
    +-2 sigma, sd 30 * sqrt(1 - 4 phi(2) / (2 Phi(2) - 1)) = 26.4."""
    rng = np.random.default_rng(11)
    n_pairs, read, exon = 500000, 50, 6000
    ivs = [("chr1", 1 + 20000 * k, 20000 * k + exon, "+") for k in range(8)]
    frag = np.maximum(np.rint(rng.normal(250.0, 30.0, n_pairs)).astype(np.int64), read + 10)
    which = rng.integers(0, len(ivs), n_pairs)
    left = 20000 * which + (rng.random(n_pairs) * (exon - frag)).astype(np.int64)
    right = left + frag - read
    out = [_header(["chr1"])]
    for k in range(n_pairs):
        out.append("f%d\t99\tchr1\t%d\t50\t50M\t=\t1\t0\t*\t*\nf%d\t147\tchr1\t%d\t50\t50M\t=\t1\t0\t*\t*\n"
                   % (k, left[k] + 1, k, right[k] + 1))
    sam = "".join(out)
    gff = _write(tmp_path, "s.gff", _gff(ivs))
    path = _write(tmp_path, "s.sam", sam)
    counts, text = _check_end_to_end(path, sam, gff, tmp_path=tmp_path)
    assert counts["kept"] == n_pairs
    params = pe_utils.parse_insert_len_params(text.splitlines()[0])
    phi2 = math.exp(-2.0) / math.sqrt(2 * math.pi)
    trunc_sd = 30.0 * math.sqrt(1 - 4 * phi2 / math.erf(2 / math.sqrt(2)))
    assert abs(trunc_sd - 26.4) < 0.05
    assert abs(float(params["mean"]) - 250.0) <= 1.0
    assert abs(float(params["sdev"]) - trunc_sd) <= 1.0


def test_cli_child_process(atp2b1, tmp_path):
    sam, sam_path, bam_path, _ = atp2b1
    gff_dir, out_dir = tmp_path / "gff", tmp_path / "out"
    r = subprocess.run([sys.executable, "-m", "miso_amd.exon_utils", "--get-const-exons", ATP2B1_GFF,
                        "--output-dir", str(gff_dir)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    gff = str(gff_dir / "Atp2b1.mm9.min_20.const_exons.gff")
    r = subprocess.run([sys.executable, "-m", "miso_amd.pe_utils", "--compute-insert-len", sam_path + "," + bam_path,
                        gff, "--output-dir", str(out_dir)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for stage in ("decode", "record pass", "grouping", "pair pass", "write"):
        assert stage in r.stderr
    want, _ = ref.insert_len(ref.parse_sam(sam), ref.gff_intervals(open(gff).read()))
    want_text, _ = ref.summarize(want, ref.gff_intervals(open(gff).read()))
    for p in (sam_path, bam_path):
        assert open(str(out_dir / (os.path.basename(p) + ".insert_len"))).read() == want_text
    # a GFF that names no reference of the file: no pairs, a warning, exit 0 and no file
    empty = _write(tmp_path, "none.gff", _gff([("chrQ", 1, 100, "+")]))
    r = subprocess.run([sys.executable, "-m", "miso_amd.pe_utils", "--compute-insert-len", sam_path, empty,
                        "--output-dir", str(tmp_path / "none")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "no paired mates" in r.stderr
    assert not os.path.exists(str(tmp_path / "none" / "c2c12.Atp2b1.sam.insert_len"))
