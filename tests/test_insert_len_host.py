"""CPU: `exon_utils --get-const-exons`, the statistics and the file of `pe_utils --compute-insert-len`, against the
restatement in tests/_insert_len_ref.py; without a GPU the native pass refuses (there is no CPU path)."""
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest

import _insert_len_ref as ref
from miso_amd import capi, exon_utils, pe_utils, sam_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
ATP2B1_GFF = os.path.join(DATA, "Atp2b1.mm9.gff")

# two genes on chr1 and one on chr2:
#   g1: t1 = e1 e2 e3 e4, t2 = e1 e3' e4 (e2 skipped, e3' = e3 on the other strand), t3 = e1 e3 e4
#   g2: one transcript, exons of 9 / 10 / 11 bp around min_size 10
#   g3: a gene whose first transcript has no exons
MULTI_GFF = """##gff-version 3
chr1\tsrc\tgene\t100\t2000\t.\t+\t.\tID=g1
chr1\tsrc\tmRNA\t100\t2000\t.\t+\t.\tID=t1;Parent=g1
chr1\tsrc\texon\t100\t200\t.\t+\t.\tID=e1;Parent=t1
chr1\tsrc\texon\t500\t600\t.\t+\t.\tID=e2;Parent=t1
chr1\tsrc\texon\t900\t1000\t.\t+\t.\tID=e3;Parent=t1
chr1\tsrc\texon\t1900\t2000\t.\t+\t.\tID=e4;Parent=t1
chr1\tsrc\tmRNA\t100\t2000\t.\t+\t.\tID=t2;Parent=g1
chr1\tsrc\texon\t100\t200\t.\t+\t.\tID=e1b;Parent=t2
chr1\tsrc\texon\t900\t1000\t.\t-\t.\tID=e3b;Parent=t2
chr1\tsrc\texon\t1900\t2000\t.\t+\t.\tID=e4b;Parent=t2
chr1\tsrc\tmRNA\t100\t2000\t.\t+\t.\tID=t3;Parent=g1
chr1\tsrc\texon\t100\t200\t.\t+\t.\tID=e1c;Parent=t3
chr1\tsrc\texon\t900\t1000\t.\t+\t.\tID=e3c;Parent=t3
chr1\tsrc\texon\t1900\t2000\t.\t+\t.\tID=e4c;Parent=t3
chr2\tsrc\tgene\t10\t100\t.\t-\t.\tID=g2
chr2\tsrc\tmRNA\t10\t100\t.\t-\t.\tID=t4;Parent=g2
chr2\tsrc\texon\t10\t18\t.\t-\t.\tID=s9;Parent=t4
chr2\tsrc\texon\t30\t39\t.\t-\t.\tID=s10;Parent=t4
chr2\tsrc\texon\t50\t60\t.\t-\t.\tID=s11;Parent=t4
chr3\tsrc\tgene\t10\t100\t.\t+\t.\tID=g3
chr3\tsrc\tmRNA\t10\t100\t.\t+\t.\tID=t5;Parent=g3
"""


@pytest.fixture
def multi_gff(tmp_path):
    p = tmp_path / "multi.gff3"
    p.write_text(MULTI_GFF)
    return str(p)


def _triples(recs):
    return [(r.seqid, r.start, r.end, r.strand, r.get_value("GeneParent")) for r in recs]


def test_const_exons_atp2b1():
    got = exon_utils.get_const_exons(ATP2B1_GFF, min_size=20)
    want = ref.const_exons(open(ATP2B1_GFF).read(), min_size=20)
    assert _triples(got) == want
    assert len(want) == 5


@pytest.mark.parametrize("min_size", [0, 10, 11, 101, 102])
def test_const_exons_hand_made(multi_gff, min_size):
    got = _triples(exon_utils.get_const_exons(multi_gff, min_size=min_size))
    assert got == ref.const_exons(MULTI_GFF, min_size=min_size)
    g1 = [("chr1", 100, 200, "+", "g1"), ("chr1", 1900, 2000, "+", "g1")]   # e2 skipped, e3 strand mismatch
    g2 = [("chr2", 10, 18, "-", "g2"), ("chr2", 30, 39, "-", "g2"), ("chr2", 50, 60, "-", "g2")]
    want = {0: g1 + g2, 10: g1 + g2[1:], 11: g1 + g2[2:], 101: g1, 102: []}[min_size]
    assert got == want


def test_const_exons_file(multi_gff, tmp_path):
    out_dir = str(tmp_path / "out")
    recs, path = exon_utils.get_const_exons_by_gene(multi_gff, out_dir, min_size=10)
    assert path == os.path.join(out_dir, "multi.min_10.const_exons.gff")
    assert open(path).read() == (
        "##gff-version 3\n"
        "chr1\tsrc\texon\t100\t200\t.\t+\t.\tID=e1;Parent=t1;GeneParent=g1\n"
        "chr1\tsrc\texon\t1900\t2000\t.\t+\t.\tID=e4;Parent=t1;GeneParent=g1\n"
        "chr2\tsrc\texon\t30\t39\t.\t-\t.\tID=s10;Parent=t4;GeneParent=g2\n"
        "chr2\tsrc\texon\t50\t60\t.\t-\t.\tID=s11;Parent=t4;GeneParent=g2\n")
    # the file reads back as the same records
    assert _triples(pe_utils.read_intervals(path)) == _triples(recs)
    assert os.path.basename(exon_utils.const_exons_filename("/x/a.b.gff3", "/o", 20)) == "a.b.min_20.const_exons.gff"


def test_const_exons_cli(tmp_path):
    out_dir = tmp_path / "cli"
    r = subprocess.run([sys.executable, "-m", "miso_amd.exon_utils", "--get-const-exons", ATP2B1_GFF,
                        "--output-dir", str(out_dir)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    path = out_dir / "Atp2b1.mm9.min_20.const_exons.gff"
    recs = pe_utils.read_intervals(str(path))
    assert _triples(recs) == ref.const_exons(open(ATP2B1_GFF).read(), min_size=20)


def _intervals(n):
    class R(object):
        def __init__(self, k):
            self.seqid, self.start, self.end, self.strand = "chr1", 1000 * k + 1, 1000 * k + 900, "+"
    return [R(k) for k in range(n)]


def test_statistics_and_writer(tmp_path):
    rng = np.random.default_rng(7)
    regions = OrderedDict()
    ivs = _intervals(4)
    for k, iv in enumerate(ivs[:3]):
        v = np.round(rng.normal(300, 20, 400 + 50 * k)).astype(np.int64)
        v[:3] = [150, 160, 170]         # low outliers
        v[-3:] = [430, 450, 470]        # high outliers
        rng.shuffle(v)
        regions[pe_utils.interval_name(iv)] = v
    regions[pe_utils.interval_name(ivs[3])] = np.array([500, 520])   # a region that loses everything
    out = str(tmp_path / "x.insert_len")
    mu, sd, disp, n = pe_utils.summarize_insert_len_dist(regions, out, sd_max=2)
    every = np.concatenate(list(regions.values())).astype(np.float64)
    m0, s0 = every.mean(), every.std()
    left = every[(every >= m0 - 2 * s0) & (every <= m0 + 2 * s0)]
    assert n == len(left) and mu == left.mean() and sd == left.std() and disp == left.std() / np.sqrt(left.mean())
    assert left.min() > 170 and left.max() < 430 and n < len(every) - 8
    text = open(out).read()
    lines = text.splitlines()
    assert lines[0] == "#mean=%.1f,sdev=%.1f,dispersion=%.1f,num_pairs=%d" % (mu, sd, disp, n)
    assert lines[1] == "#region\tinsert_len"
    assert [l.split("\t")[0] for l in lines[2:]] == [pe_utils.interval_name(iv) for iv in ivs[:3]]
    for line, (region, v) in zip(lines[2:], regions.items()):
        vals = [int(x) for x in line.split("\t")[1].split(",")]
        assert vals == [int(x) for x in v if m0 - 2 * s0 <= x <= m0 + 2 * s0]   # order kept, by value
    # the checker's restatement writes the same text
    by_iv = {k: list(map(int, v)) for k, v in enumerate(regions.values())}
    want, _ = ref.summarize(by_iv, [ref.Interval(iv.seqid, iv.start, iv.end, iv.strand) for iv in ivs])
    assert text == want


def test_round_trip(tmp_path):
    ivs = _intervals(2)
    regions = OrderedDict([(pe_utils.interval_name(ivs[0]), np.array([200, 210, 190])),
                           (pe_utils.interval_name(ivs[1]), np.array([205, 195]))])
    out = str(tmp_path / "r.insert_len")
    mu, sd, disp, n = pe_utils.summarize_insert_len_dist(regions, out, sd_max=2)
    values, params = pe_utils.load_insert_len(out)
    assert list(values) == [200, 210, 190, 205, 195]
    assert params == {"mean": "%.1f" % mu, "sdev": "%.1f" % sd, "dispersion": "%.1f" % disp, "num_pairs": "5"}
    assert pe_utils.parse_insert_len_params("#mean=1.0,sdev=2.5\n") == {"mean": "1.0", "sdev": "2.5"}


def test_nothing_left_is_an_error(tmp_path):
    with pytest.raises(pe_utils.InsertLenError):
        pe_utils.summarize_insert_len_dist(OrderedDict(), str(tmp_path / "e.insert_len"))


def test_no_cpu_fallback_without_device(tmp_path):
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    p = tmp_path / "t.sam"
    p.write_text("@SQ\tSN:chr1\tLN:1000\nr1\t67\tchr1\t10\t50\t20M\t=\t60\t70\t*\t*\n")
    f = sam_utils.Samfile(str(p))
    with pytest.raises(capi.InternalError, match="no HIP device"):
        capi.insert_len(f, ["chr1"], [1], [500])
    with pytest.raises(capi.InternalError, match="no HIP device"):
        capi.insert_tag_records(f, ["chr1"], [1], [500])
    import ctypes
    n = ctypes.c_int64(0)
    rc = capi.lib().miso_insert_len(f._h, 0, 1, 0, None, None, None, 0, None, None, 0, ctypes.byref(n), None)
    assert rc == capi.MISO_ENODEVICE
