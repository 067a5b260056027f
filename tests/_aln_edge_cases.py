"""Test helper: the inputs of tests/test_aln_edge_cases.py (the checkers alone, no GPU) and tests/test_gpu_aln_edges.py
(the device passes): alignment files that reach the branches of csrc/kernels_density.hip and csrc/kernels_insert.hip the
seeded random files of tests/test_gpu_density.py and tests/test_gpu_insert_len.py never enter.  Pure Python: SAM text,
region / interval lists, nothing of the package.

Density cases are (sam text, [(seqid, tx_start, tx_end)]); insert cases are ([(seqid, start, end, strand)], sam text).
"""
import random

BIG = 2 ** 31 - 1                 # the longest reference an int32 coordinate reaches
COORD_LIMIT = 2 ** 40             # kCoordLimit of kernels_density.hip: region coordinates beyond +-2^40 are refused
FIRST_JXN_CAP = 1 << 20           # kFirstJxnCap of kernels_density.hip: the junction list's first capacity per group
WRAPPER_JXN_CAP = 1 << 16         # capi.region_densities: the junction arrays of its first call
WORDS_PER_RECORD = 4              # kWordsPerRecord: a chunk of C records holds max(4 C, longest CIGAR) words


def header(refs):
    return "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)


def line(name, flag, rname, pos0, cigar):
    return "%s\t%d\t%s\t%d\t50\t%s\t*\t0\t0\t*\t*" % (name, flag, rname, pos0 + 1, cigar)


def n_ops(cigar):
    return sum(1 for ch in cigar if not ch.isdigit())


# ---- density 1: the junction list overruns its first capacity, and the wrapper's arrays theirs ----
def overrun_case(seed=1):
    """9000 records with a D and an N gap each, all inside region 0; 64 regions that each hold all of them.  Region k is
    region 0 widened by k bases on both sides: its junctions are region 0's, its depth and wiggle region 0's behind k
    zeros."""
    rng = random.Random(seed)
    recs = []
    for i in range(9000):
        pos0 = rng.randint(1100, 50000)
        recs.append(line("o%d" % i, 0, "chr1", pos0, "20M3D10M%dN20M" % rng.randint(10, 3000)))
    regions = [("chr1", 1000 - k, 60000 + k) for k in range(64)]
    return header([("chr1", 3000000)]) + "\n".join(recs) + "\n", regions


def group_bytes(regions, n_classes):
    """The accumulator bytes miso_region_densities counts for a group of regions (include/miso_alnio.h: difference rows
    of L + 1 int32 per qlen class, an int32 depth and a double wiggle per base)."""
    return sum(n_classes * (b - a + 2) * 4 + (b - a + 1) * 12 for _, a, b in regions)


# ---- density 2: chunks that end on the CIGAR-word bound ----
WORDY = ["5S10M1D10M1I10M2D10M5S",          # 9 ops
         "5S10M1D10M1I10M2D10M",            # 8
         "10M1I10M1D10M1I10M",              # 7
         "5S20M%dN20M1D5M5S",               # 7, one N
         "10M2D10M%dN10M1I10M",             # 7, one N
         "3H5S15M1D15M1I15M",               # 7
         "20=5X1D10M1I10M5S",               # 7
         "5S15M1I15M2D15M"]                 # 6
WORDS_REGION = ("chr1", 5000, 25000)


def words_case(seed=2):
    """~3000 records of 6 to 9 ops over one 20 kb region and its two edges, one plain 50M in 150."""
    rng = random.Random(seed)
    recs = []
    for i in range(3000):
        cigar = rng.choice(WORDY)
        if "%d" in cigar:
            cigar = cigar % rng.randint(10, 1500)
        if i % 150 == 75:
            cigar = "50M"
        recs.append(line("w%d" % i, 0, "chr1", rng.randint(4900, 25050), cigar))
    return header([("chr1", 3000000)]) + "\n".join(recs) + "\n", [WORDS_REGION]


def cigars_of(sam):
    return [f.split("\t")[5] for f in sam.splitlines() if f and not f.startswith("@")]


# ---- density 3: the CIGAR shapes the rules mention in passing ----
SHAPES = ["0M50M", "50M0M", "5H45M", "10M5P40M", "10M0N40M", "5D50M", "5N50M", "50M5D", "3I", "10S", "20M5D0M5D30M",
          "1M1D1M1D1M1D1M", "25M2I23M"]
SHAPES_AT = 2100                  # shape k at pos0 = SHAPES_AT + 100 k


def shapes_case():
    """One record per shape, 100 bases apart, and one flagged unmapped with a position and 50M.  Three regions: one
    around all of them, one that begins inside the first D gap of 20M5D0M5D30M, one whose tx_end is the rightss of the
    second gap of 1M1D1M1D1M1D1M (rule 5 is strict: that junction does not count)."""
    recs = [line("s%d" % k, 0, "chr1", SHAPES_AT + 100 * k, cg) for k, cg in enumerate(SHAPES)]
    recs.append(line("unmapped", 4, "chr1", SHAPES_AT + 100 * len(SHAPES), "50M"))
    gap = SHAPES_AT + 100 * SHAPES.index("20M5D0M5D30M") + 20          # pos0 of the first deleted base
    steps = SHAPES_AT + 100 * SHAPES.index("1M1D1M1D1M1D1M")
    regions = [("chr1", 2000, 4000), ("chr1", gap + 2, 4000), ("chr1", 2000, steps + 5)]
    return header([("chr1", 3000000)]) + "\n".join(recs) + "\n", regions


# ---- density 4: the top of the qlen bitmap and the refusal beyond it ----
QLEN_REGION = ("chr1", 1000, 70999)


def qlen_case(extra=None):
    """65535M (word 2047, bit 31 of the bitmap) beside two 50M, in a region of 70 000 bases.  extra = "inside": a 65536M
    record the region fetches; "outside": the same record where no region fetches it."""
    recs = [line("short1", 0, "chr1", 1500, "50M"), line("top", 0, "chr1", 2000, "65535M"),
            line("short2", 0, "chr1", 60000, "50M")]
    if extra == "inside":
        recs.insert(2, line("over", 0, "chr1", 3000, "65536M"))
    elif extra == "outside":
        recs.insert(2, line("over", 0, "chr1", 500000, "65536M"))
    return header([("chr1", 3000000)]) + "\n".join(recs) + "\n", [QLEN_REGION]


# ---- density 5: records at the int32 end, regions beyond it ----
def coords_case():
    recs = [line("zero", 0, "chrBig", 0, "50M"),
            line("zero_jx", 0, "chrBig", 10, "20M10N20M"),
            line("jx", 0, "chrBig", BIG - 55, "20M10N20M"),      # rightss = BIG - 24, its last base BIG - 6 (0-based)
            line("last", 0, "chrBig", BIG - 50, "50M")]          # bam_endpos = BIG: ends on the last base
    regions = [("chrBig", BIG - 100, BIG + 50),
               ("chrBig", BIG - 100, 2 ** 31 + 1000),
               ("chrBig", COORD_LIMIT, COORD_LIMIT),
               ("chrBig", -COORD_LIMIT, -COORD_LIMIT),
               ("chrBig", -50, 200)]
    return header([("chrBig", BIG)]) + "\n".join(recs) + "\n", regions


# ---- insert 6: the record search against brute force ----
TAG_FLAGS = [99, 147, 0, 4 | 99, 0x200 | 99, 0x8 | 99]
REF_LEN = 100000


def tagging_case(seed=6):
    """~250 intervals on three references and ~8000 records, 60 % within +-60 of an interval edge.
    chrA: one interval over the whole reference (the search starts at the first interval) and scattered, nested ones;
    chrB: short disjoint intervals only (the search starts next to the record);
    chrC: nests with exact duplicates, groups of 3 to 5 with one start and different ends, the longest never listed
    first, an interval with start > end and two with start == end.  chrD has records and no interval, chrQ an interval
    and no records.  Intervals are listed out of coordinate order."""
    rng = random.Random(seed)
    blocks = [[("chrA", 1, REF_LEN)]]
    for _ in range(45):                                          # chrA: scattered, a third nested in the one before
        if len(blocks) > 1 and rng.random() < 0.33:
            _, s, e = blocks[-1][0]
            a = rng.randint(s, e)
            blocks.append([("chrA", a, rng.randint(a, e))])
        else:
            a = rng.randint(100, REF_LEN - 4000)
            blocks.append([("chrA", a, a + rng.randint(50, 3000))])
    for k in range(90):                                          # chrB: disjoint, 30 to 200 bases
        a = 500 + 1000 * k + rng.randint(0, 300)
        blocks.append([("chrB", a, a + rng.randint(30, 200))])
    for k in range(15):                                          # chrC: nests, the inner one sometimes twice
        s = 1000 + 3000 * k
        nest = [("chrC", s, s + 2000), ("chrC", s + 200, s + 1500), ("chrC", s + 400, s + 800)]
        if k % 2:
            nest.append(nest[2])
        if k % 5 == 0:
            nest.append(nest[0])
        rng.shuffle(nest)
        blocks.append(nest)
    for k in range(12):                                          # chrC: one start, 3 to 5 ends
        s = 50000 + 3000 * k
        ends = rng.sample(range(s + 40, s + 900), rng.randint(3, 5))
        if ends[0] == max(ends):
            ends[0], ends[-1] = ends[-1], ends[0]
        blocks.append([("chrC", s, e) for e in ends])
    blocks += [[("chrC", 90500, 90400)], [("chrQ", 1, REF_LEN)], [("chrC", 95000, 95000)], [("chrB", 95000, 95000)]]
    rng.shuffle(blocks)
    ivs = [iv for block in blocks for iv in block]
    live = [iv for iv in ivs if iv[0] != "chrQ"]
    recs = []

    def cigar(span):
        u = rng.random()
        if span >= 3 and u < 0.25:
            a = rng.randint(1, span - 2)
            n = rng.randint(1, span - 1 - a)
            return "%dM%dN%dM" % (a, n, span - a - n)
        if u < 0.32:
            return "5S%dM" % span
        return "%dM" % span
    for i in range(8000):
        span = rng.randint(1, 120)
        if rng.random() < 0.6:
            seqid, a, b = rng.choice(live)
            edge = a - 1 if rng.random() < 0.5 else b
            pos0 = edge + rng.randint(-60, 60) - (span if rng.random() < 0.5 else 0)
        else:
            seqid, pos0 = rng.choice(["chrA", "chrB", "chrC", "chrC", "chrD"]), rng.randint(0, REF_LEN - 200)
        recs.append(line("t%d" % i, rng.choice(TAG_FLAGS), seqid, max(0, pos0), cigar(span)))
    for seqid, a, b in live:                                     # every interval's own span, and one base more
        if a <= b:
            recs.append(line("own%d" % len(recs), 99, seqid, a - 1, "%dM" % (b - a + 1)))
            recs.append(line("own%d" % len(recs), 99, seqid, a - 1, "%dM" % (b - a + 2)))
    refs = [("chrA", REF_LEN), ("chrB", REF_LEN), ("chrC", REF_LEN), ("chrD", REF_LEN)]
    return ivs, header(refs) + "\n".join(recs) + "\n"


# ---- insert 7: the pair pass on wavefronts of 64 different intervals ----
PAIR_INTERVALS, PAIRS_EACH, ONE_INTERVAL_PAIRS, REFUSALS_EACH = 128, 20, 500, 64


def pairs_case(seed=7):
    """128 disjoint intervals, 20 proper pairs each in an order that cycles through the intervals (any 64 consecutive
    pairs lie in 64 different intervals); then 500 pairs in one interval; then 64 pairs each of: mates on one strand, a
    spliced mate, mates in two intervals, insert <= 0 (the right mate first in the file)."""
    rng = random.Random(seed)
    ivs = [("chr1", 1001 + 10000 * k, 4000 + 10000 * k, "+-"[k % 2]) for k in range(PAIR_INTERVALS)]
    out = []

    def pair(name, k, a, b, ca="50M", cb="50M", fa=99, fb=147, kb=None):
        base = 1000 + 10000 * k
        base_b = base if kb is None else 1000 + 10000 * kb
        out.append("%s\t%d\tchr1\t%d\t50\t%s\t=\t1\t0\t*\t*" % (name, fa, base + a + 1, ca))
        out.append("%s\t%d\tchr1\t%d\t50\t%s\t=\t1\t0\t*\t*" % (name, fb, base_b + b + 1, cb))
    for rnd in range(PAIRS_EACH):
        for k in range(PAIR_INTERVALS):
            a = rng.randint(0, 2000)
            pair("c%d_%d" % (rnd, k), k, a, a + rng.randint(1, 900))
    for i in range(ONE_INTERVAL_PAIRS):
        a = rng.randint(0, 2000)
        pair("one%d" % i, 5, a, a + rng.randint(1, 900))
    for i in range(REFUSALS_EACH):
        pair("same%d" % i, i, 100, 400, fa=99, fb=131)
    for i in range(REFUSALS_EACH):
        pair("spl%d" % i, 64 + i, 100, 400, cb="20M100N30M")
    for i in range(REFUSALS_EACH):
        pair("two%d" % i, i, 100, 400, kb=i + 1)
    for i in range(REFUSALS_EACH):
        pair("neg%d" % i, 2 * i, 500, 450 - (i % 3) * 25, fa=147, fb=99)       # inserts 0, -25, -50
    return ivs, header([("chr1", 10000 * PAIR_INTERVALS + 10000)]) + "\n".join(out) + "\n"


def gff_text(ivs):
    return "##gff-version 3\n" + "".join("%s\tt\texon\t%d\t%d\t.\t%s\t.\tID=x%d\n" % (s, a, b, st, k)
                                         for k, (s, a, b, st) in enumerate(ivs))
