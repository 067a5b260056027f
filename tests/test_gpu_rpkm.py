"""GPU: `sam_rpkm --compute-rpkm` -- the fetch-count pass (csrc/kernels_rpkm.hip) against the brute-force counts of
tests/_rpkm_ref.py and against the host index (Samfile.fetch_indices) for SAM, BAM and shuffled input at several chunk
sizes, the empty cases, exact name matching, the tool end to end, and the coverage pass (which shares
csrc/record_pass.hpp with it) against its own checker on the same file."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import _bam
import _coverage_ref as coverage_ref
import _rpkm_case as case
import _rpkm_ref as ref
from miso_amd import capi, exon_utils, sam_rpkm, sam_utils

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 2 ** 31 - 1                     # length of the third reference: the largest an int32 coordinate reaches
CIGARS = ["50M", "20M%dN30M", "10S40M", "*", "30M5D20M"]
FLAGS = [0, 4, 16, 256, 512, 1024, 99, 147]


@pytest.fixture(scope="module", autouse=True)
def device():
    if capi.device_count() < 1:
        pytest.fail("no HIP device visible")


def sam_to_bam(sam_text, path):
    """_bam.sam_to_bam; the bin of the record at the far end of the 2^31 - 1 reference does not fit the 16-bit field
    (BAM bins stop at 2^29) and is stored truncated, as htslib stores it.  The reader does not use bins."""
    orig = _bam._reg2bin
    _bam._reg2bin = lambda beg, end: orig(beg, end) & 0xFFFF
    try:
        _bam.sam_to_bam(sam_text, path, block=60000)
    finally:
        _bam._reg2bin = orig


def build_case(rng):
    """(intervals as (GFF seqid, start, end), records as (file's reference name, pos0, flag, cigar), planted: name ->
    (interval index, expected count))."""
    file_name = {"chr1": "chr1", "chr2": "2", "chrBig": "chrBig"}
    ivs, recs, planted = [], [], {}
    # random intervals in the first 300 kb of each reference: nested, duplicate and start == end among them
    for _ in range(190):
        r = rng.random()
        if r < 0.12 and ivs:
            seqid, s, e = ivs[rng.randrange(len(ivs))]
            start = rng.randint(s, e)
            end = rng.randint(start, e)
        elif r < 0.2 and ivs:
            seqid, start, end = ivs[rng.randrange(len(ivs))]
        elif r < 0.26:
            seqid = rng.choice(["chr1", "chr2", "chrBig"])
            start = end = rng.randint(1, 300000)
        else:
            seqid = rng.choice(["chr1", "chr2", "chrBig"])
            start = rng.randint(1, 300000)
            end = start + rng.randint(40, 3000)
        ivs.append((seqid, start, end))
    n_random = len(ivs)
    for i in range(19000):
        if rng.random() < 0.6:
            seqid, s, e = ivs[rng.randrange(n_random)]
            name, pos0 = file_name[seqid], max(0, rng.randint(s - 200, e + 50) - 1)
        else:
            name, pos0 = rng.choice(["chr1", "2", "chrBig"]), rng.randint(0, 320000)
        cigar = rng.choices(CIGARS, [60, 20, 10, 3, 7])[0]
        if "%d" in cigar:
            cigar = cigar % rng.randint(10, 3000)
        flag = rng.choice([0, 0, 0] + FLAGS)
        if flag & 4:                       # unmapped: a third without a reference, a third without a CIGAR
            u = rng.random()
            if u < 0.33:
                name, pos0, cigar = "*", -1, "*"
            elif u < 0.66:
                cigar = "*"
        recs.append((name, pos0, flag, cigar))
    # every boundary of one isolated interval [S, E): bam_endpos == S out, S + 1 in; pos == E - 1 in, E out
    S, E = 500000, 500100
    planted["boundary"] = (len(ivs), 2)
    ivs.append(("chr1", S, E))
    recs += [("chr1", S - 50, 0, "50M"), ("chr1", S - 49, 0, "50M"), ("chr1", E - 1, 16, "50M"), ("chr1", E, 0, "50M")]
    # ... and of a start == end interval: only a record over the position counts (pos < S2 < bam_endpos)
    S2 = 510000
    planted["point"] = (len(ivs), 1)
    ivs.append(("chr2", S2, S2))
    recs += [("2", S2 - 50, 0, "50M"), ("2", S2 - 25, 0, "50M"), ("2", S2, 0, "50M")]
    # 100 consecutive records of a sorted file in one bin
    planted["one_bin"] = (len(ivs), 100)
    ivs.append(("chr1", 599990, 600100))
    recs += [("chr1", 600000, rng.choice(FLAGS), "50M") for _ in range(100)]
    # 200 consecutive records, each in a bin of its own: 200 small intervals with one record inside each
    for k in range(200):
        base = 700000 + 10 * k
        ivs.append(("chr2", base, base + 5))
        recs.append(("2", base + 1, 0, "3M"))
    planted["own_bins"] = (len(ivs) - 1, 1)
    # the far end of the 2^31 - 1 reference: a record ending on its last base, intervals over it and beyond int32
    recs.append(("chrBig", BIG - 50, 0, "50M"))
    planted["far_end"] = (len(ivs), 1)
    ivs.append(("chrBig", BIG - 30, BIG))
    planted["past_int32"] = (len(ivs), 1)
    ivs.append(("chrBig", BIG - 1, 2 ** 33))
    planted["beyond"] = (len(ivs), 0)
    ivs.append(("chrBig", BIG, 2 ** 40))
    # start > end, and a reference the file lacks
    planted["reversed"] = (len(ivs), 0)
    ivs.append(("chr1", 5000, 4000))
    planted["absent"] = (len(ivs), 0)
    ivs.append(("chr9", 1, 3000000))
    return ivs, recs, planted


@pytest.fixture(scope="module")
def counts_case(tmp_path_factory):
    rng = random.Random(21)
    d = tmp_path_factory.mktemp("rpkm")
    ivs, recs, planted = build_case(rng)
    refs = [("chr1", 3000000), ("2", 3000000), ("chrBig", BIG)]
    order = {n: k for k, (n, _) in enumerate(refs)}
    lines = ["q%d\t%d\t%s\t%d\t50\t%s\t*\t0\t0\t*\t*" % (i, flag, name, pos0 + 1, cigar)
             for i, (name, pos0, flag, cigar) in enumerate(recs)]
    by_pos = sorted(range(len(recs)), key=lambda i: (order.get(recs[i][0], len(order)), recs[i][1]))
    head = "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    sam = head + "\n".join(lines[i] for i in by_pos) + "\n"
    shuffled_lines = list(lines)
    rng.shuffle(shuffled_lines)
    paths = {"sam": str(d / "reads.sam"), "bam": str(d / "reads.bam"), "shuffled": str(d / "shuffled.sam")}
    open(paths["sam"], "w").write(sam)
    open(paths["shuffled"], "w").write(head + "\n".join(shuffled_lines) + "\n")
    sam_to_bam(sam, paths["bam"])
    names = [r[0] for r in refs]
    resolved = [(ref.resolve(names, seqid) or "9", s, e) for seqid, s, e in ivs]
    want = ref.fetch_counts(sam, resolved)
    return paths, sam, ivs, planted, want


def test_case_holds_what_it_must(counts_case):
    """The shape of the case itself, so that the comparison below is of what the issue lists."""
    _, sam, ivs, planted, want = counts_case
    recs = [l.split("\t") for l in sam.splitlines() if not l.startswith("@")]
    assert 19000 < len(recs) < 21000 and 380 < len(ivs) < 420
    assert {int(r[1]) for r in recs} >= set(FLAGS)
    kinds = {"N" if "N" in r[5] else r[5] for r in recs}
    assert kinds >= {"50M", "N", "10S40M", "*", "30M5D20M"}
    assert any(int(r[1]) & 4 and r[2] == "*" for r in recs) and any(int(r[1]) & 4 and r[2] != "*" for r in recs)
    assert any(s == e for _, s, e in ivs) and len(set(ivs)) < len(ivs)
    assert any(a[0] == b[0] and b[1] <= a[1] and a[2] <= b[2] and a != b for a in ivs[:190] for b in ivs[:190])
    for name, (at, n) in planted.items():
        assert want[at] == n, name
    assert all(c == 1 for c in want[planted["own_bins"][0] - 199:planted["own_bins"][0] + 1])
    assert sum(1 for c in want if c > 0) > len(want) // 2


@pytest.mark.parametrize("which", ["sam", "bam", "shuffled"])
def test_fetch_counts_equal_both_checkers(counts_case, which):
    paths, _, ivs, planted, want = counts_case
    f = sam_utils.Samfile(paths[which])
    seqids = [sam_utils.resolve_chrom(f, s) for s, _, _ in ivs]
    starts, ends = [s for _, s, _ in ivs], [e for _, _, e in ivs]
    assert "chr2" not in f.references and seqids.count("2") > 200
    # the host index, one look-up per interval: what the device pass replaces
    host = [len(f.fetch_indices(n, s, e)) if n in f.references and s <= e else 0 for n, s, e in zip(seqids, starts, ends)]
    assert host == want
    for chunk in (1000, 4096, 0):
        got, st = capi.fetch_counts(f, seqids, starts, ends, chunk_records=chunk)
        assert got.dtype == np.int64 and len(got) == len(ivs)
        assert list(got) == want, chunk
        assert st["chunks"] == (len(f) + (chunk or 1 << 22) - 1) // (chunk or 1 << 22)
    assert sum(1 for c in got if c > 0) > len(ivs) // 2
    assert got[planted["boundary"][0]] == 2 and got[planted["one_bin"][0]] == 100 and got[planted["far_end"][0]] == 1


def test_fetch_counts_empty_cases(counts_case, tmp_path):
    paths = counts_case[0]
    f = sam_utils.Samfile(paths["sam"])
    got, st = capi.fetch_counts(f, [], [], [])
    assert len(got) == 0 and got.dtype == np.int64 and st["chunks"] == 1
    empty = tmp_path / "empty.sam"
    empty.write_text("@SQ\tSN:chr1\tLN:1000\n")
    e = sam_utils.Samfile(str(empty))
    assert len(e) == 0
    got, st = capi.fetch_counts(e, ["chr1", "chr1", "chr7"], [1, 5, 1], [1000, 5, 10])
    assert list(got) == [0, 0, 0] and st["chunks"] == 0
    got, st = capi.fetch_counts(e, [], [], [])
    assert len(got) == 0 and st["chunks"] == 0


def test_fetch_counts_matches_names_exactly(counts_case):
    """The C ABI does not resolve names: "chr2" is not the file's "2" (sam_rpkm resolves it first)."""
    f = sam_utils.Samfile(counts_case[0]["sam"])
    got, _ = capi.fetch_counts(f, ["chr2", "2", "CHR1", "chr1"], [1, 1, 1, 1], [3000000] * 4)
    assert got[0] == 0 and got[2] == 0
    assert got[1] == int(np.sum(f.ref_id == f.gettid("2"))) > 0
    assert got[3] == int(np.sum(f.ref_id == f.gettid("chr1"))) > 0


def test_coverage_pass_unchanged_on_this_file(counts_case, tmp_path):
    """The coverage pass shares its keys, histogram add and chunk loop with the fetch counts: on this file it still
    gives its own checker's counts (the full yardstick is test_gpu_prefilter.py)."""
    paths, sam, ivs, _, _ = counts_case
    ivs = ivs[:190:3] + ivs[190:193] + ivs[-10:]       # the checker is quadratic: a sixth of the intervals, every kind
    gff_text = "##gff-version 3\n" + "".join("%s\tt\tgene\t%d\t%d\t.\t+\t.\tID=g%03d\n" % (s, a, b, k)
                                             for k, (s, a, b) in enumerate(ivs))
    gff = tmp_path / "ivs.gff"
    gff.write_text(gff_text)
    want = coverage_ref.counts(sam, gff_text)
    f = sam_utils.Samfile(paths["bam"])
    intervals = exon_utils.read_coverage_intervals(str(gff))
    for chunk in (1000, 0):
        got, st = exon_utils.coverage_counts(f, intervals, chunk_records=chunk)
        assert list(got) == want and 0 < st["kept"] < len(f)
    assert sum(1 for c in want if c > 0) > len(want) // 2


# ---- end to end ----
def run_tool(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "miso_amd.sam_rpkm"] + args, env=env, cwd=ROOT,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)


def test_compute_rpkm_end_to_end(tmp_path, capsys):
    gff_text, sam_text = case.gff_text(), case.sam_text()
    gff, sam, bam = tmp_path / "genes.gff", tmp_path / "reads.sam", tmp_path / "reads.bam"
    gff.write_text(gff_text)
    sam.write_text(sam_text)
    _bam.sam_to_bam(sam_text, str(bam))
    want_rows, want_text, want_lines = ref.compute(sam_text, gff_text, case.READ_LEN)
    assert len(want_rows) == 4 and all(float(r["rpkm"]) > 0 for r in want_rows)
    for reads in (sam, bam):
        out = tmp_path / ("out_" + reads.suffix[1:])
        r = run_tool(["--compute-rpkm", str(gff), str(reads), str(out), "--read-len", str(case.READ_LEN)])
        assert r.returncode == 0, r.stdout
        assert (out / (reads.name + ".rpkm")).read_bytes() == want_text.encode()
        printed = r.stdout.splitlines()
        at = printed.index("Computed RPKMs for 4 genes.")
        assert printed[at:] == want_lines[-len(printed[at:]):] and len(printed[at:]) == 3 + 2 * 2
        assert "  - Total of 1 genes cannot be used because they lack const. regions." in printed
        assert "  - Total of 2 genes cannot be used since their exons are too small." in printed
        assert "    * absent\t0" in printed and any(l.startswith("    * small\t") and not l.endswith("\t0") for l in printed)
        for line in want_lines:
            assert line in printed, line
        assert "Number of total reads in BAM file: 3000" in printed
    # in process: the returned rows
    capsys.readouterr()
    rows = sam_rpkm.compute_rpkm(str(gff), str(bam), case.READ_LEN, str(tmp_path / "again"))
    assert rows == want_rows
    assert (tmp_path / "again" / "reads.bam.rpkm").read_bytes() == want_text.encode()
