"""The annotation and reads of the sam_rpkm tests (CPU and GPU): eight small genes, one for every per-gene rule of
misopy/sam_rpkm.py:109-195, and a few thousand reads over them.  Text only; the tests write the files."""
import random

READ_LEN = 36

# gene id -> (seqid of the GFF, [transcript: [(start, end) of its exons]])
GENES = [
    # two isoforms, a skipped exon: the flanking exons are constitutive, two copies each
    ("se2", "chr1", [[(1000, 1100), (1300, 1350), (1600, 1700)], [(1000, 1100), (1600, 1700)]]),
    # three isoforms on the file's "2"; the middle exon has the same start and another end in the third
    ("alt3", "chr2", [[(5000, 5100), (5300, 5400), (5700, 5800)], [(5000, 5100), (5300, 5400), (5700, 5800)],
                      [(5000, 5100), (5300, 5450), (5700, 5800)]]),
    # no constitutive part
    ("noconst", "chr1", [[(9000, 9100)], [(9200, 9300)]]),
    # constitutive exons of 21 and 31 bases, all shorter than the reads
    ("small", "chr1", [[(12000, 12020), (12100, 12200), (12300, 12330)], [(12000, 12020), (12300, 12330)]]),
    ("onrandom", "chr5_random", [[(100, 400)], [(100, 400), (600, 700)]]),
    # neither "chr9" nor "9" is in the file
    ("absent", "chr9", [[(100, 400), (600, 700)], [(100, 400)]]),
    # one shared exon, a record per transcript: counted twice into the total, one entry in the row
    ("shared", "chr1", [[(20000, 20500)], [(20000, 20500), (20700, 20800)]]),
    # a long and a short constitutive exon: the short one adds to the total only
    ("mixed", "chr1", [[(30000, 30020), (30100, 30300), (30500, 30600)], [(30000, 30020), (30100, 30300)]]),
]
REFS = [("chr1", 100000), ("2", 100000), ("chr5_random", 100000)]


def gff_text():
    lines = ["##gff-version 3"]
    for gid, seqid, transcripts in GENES:
        lo = min(s for t in transcripts for s, _ in t)
        hi = max(e for t in transcripts for _, e in t)
        lines.append("%s\tx\tgene\t%d\t%d\t.\t+\t.\tID=%s" % (seqid, lo, hi, gid))
        for m, exons in enumerate(transcripts):
            tid = "%s.t%d" % (gid, m)
            lines.append("%s\tx\tmRNA\t%d\t%d\t.\t+\t.\tID=%s;Parent=%s" % (seqid, exons[0][0], exons[-1][1], tid, gid))
            lines += ["%s\tx\texon\t%d\t%d\t.\t+\t.\tID=%s.e%d;Parent=%s" % (seqid, s, e, tid, k, tid)
                      for k, (s, e) in enumerate(exons)]
    return "\n".join(lines) + "\n"


def sam_text(n_reads=3000, seed=11):
    rng = random.Random(seed)
    name_in_file = {"chr1": "chr1", "chr2": "2", "chr5_random": "chr5_random"}
    near = [(name_in_file[seqid], s, e) for _, seqid, ts in GENES if seqid in name_in_file for t in ts for s, e in t]
    recs = []
    for i in range(n_reads):
        u = rng.random()
        if u < 0.85:
            name, s, e = near[rng.randrange(len(near))]
            pos0 = max(0, rng.randint(s - 60, e + 20) - 1)
        else:
            name, pos0 = rng.choice(REFS)[0], rng.randint(0, 40000)
        v = rng.random()
        cigar = "36M" if v < 0.7 else "16M%dN20M" % rng.randint(50, 400) if v < 0.9 else "6S30M" if v < 0.95 else "*"
        flag = rng.choice([0, 0, 0, 16, 256, 1024, 4])
        if flag & 4 and rng.random() < 0.5:
            name, pos0, cigar = "*", -1, "*"
        recs.append((name, pos0, "q%d\t%d\t%s\t%d\t50\t%s\t*\t0\t0\t*\t*" % (i, flag, name, pos0 + 1, cigar)))
    order = {n: k for k, (n, _) in enumerate(REFS)}
    recs.sort(key=lambda r: (order.get(r[0], len(order)), r[1]))
    head = "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)
    return head + "\n".join(r[2] for r in recs) + "\n"
