"""Test checker: a literal, slow restatement of `sam_rpkm --compute-rpkm` (misopy/sam_rpkm.py:23-212 with
Gene.get_const_parts, Gene.py:155-181) over SAM text and GFF text (gene -> mRNA -> exon by ID / Parent), sharing no
code with the package.  A fetch is the brute-force count of the records of the named reference with
pos < end and bam_endpos > start.  With the three deviations DESIGN.md section 21 states: rows and the too-small list in
GFF order; a chromosome maps to the file's reference the way every tool here maps it (itself, else without its first
"chr"), messages print the annotation's spelling; a gene on a chromosome the file lacks prints the fetch error for its
first part and is listed as too small with total 0.
"""
import math
import re


class Rec(object):
    __slots__ = ("flag", "rname", "pos", "end")

    def __init__(self, flag, rname, pos, cigar):
        self.flag, self.rname, self.pos = flag, rname, pos
        reflen = sum(n for op, n in cigar if op in "MDN=X")
        # htslib bam_endpos: the spliced span; pos + 1 without a reference-consuming operation or when unmapped
        self.end = pos + 1 if (flag & 4) or reflen == 0 else pos + reflen


def parse_sam(text):
    """(reference names of the header in order, records)."""
    refs, recs = [], []
    for line in text.splitlines():
        if not line:
            continue
        if line.startswith("@"):
            if line.startswith("@SQ"):
                refs.append(dict(x.split(":", 1) for x in line.split("\t")[1:])["SN"])
            continue
        f = line.split("\t")
        cigar = [] if f[5] == "*" else [(op, int(n)) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", f[5])]
        recs.append(Rec(int(f[1]), f[2], int(f[3]) - 1, cigar))
    return refs, recs


def fetch_count(recs, name, start, end):
    """len(bamfile.fetch(name, start, end)): no flag matters, a record without a reference ("*") is on none."""
    n = 0
    for r in recs:
        if r.rname == name and r.rname != "*" and r.pos < end and r.end > start:
            n += 1
    return n


def fetch_counts(sam_text, intervals):
    """The count of every (name, start, end); start > end counts 0 (pysam raises there; the device call answers 0)."""
    _, recs = parse_sam(sam_text)
    by_name = {}
    for r in recs:
        by_name.setdefault(r.rname, []).append(r)
    return [fetch_count(by_name.get(name, []), name, start, end) if start <= end else 0
            for name, start, end in intervals]


def resolve(refs, seqid):
    """The file's name for a seqid: itself, else without its first "chr"; None if the file has neither."""
    if seqid in refs:
        return seqid
    pieces = seqid.split("chr")
    name = pieces[1] if len(pieces) > 1 else pieces[0]
    return name if name in refs else None


def parse_genes(gff_text):
    """[(gene id, chromosome, [transcript: [(start, end) of its exons, by start]])] in file order; a transcript
    without exons is dropped, a gene without transcripts too."""
    genes, mrnas, exons = [], [], []
    for line in gff_text.splitlines():
        if line.startswith("#"):
            continue
        f = line.split("\t")
        if len(f) < 9:
            continue
        attrs = dict(p.split("=", 1) for p in f[8].split(";") if "=" in p)
        if f[2] == "gene":
            genes.append((attrs["ID"], f[0]))
        elif f[2] == "mRNA":
            mrnas.append((attrs["ID"], attrs["Parent"]))
        elif f[2] == "exon":
            exons.append((attrs["Parent"], int(f[3]), int(f[4])))
    out = []
    for gene_id, chrom in genes:
        transcripts = []
        for mrna_id, parent in mrnas:
            if parent != gene_id:
                continue
            mine = sorted([(s, e) for p, s, e in exons if p == mrna_id], key=lambda x: x[0])
            if mine:
                transcripts.append(mine)
        if transcripts:
            out.append((gene_id, chrom, transcripts))
    return out


def const_parts(transcripts):
    """Gene.get_const_parts: every part (one per exon record, transcript after transcript) that every isoform holds,
    by start and end."""
    parts = [p for t in transcripts for p in t]
    out = []
    for part in parts:
        add = True
        for iso in transcripts:
            has = False
            for q in iso:
                if q[0] == part[0] and q[1] == part[1]:
                    has = True
            if not has:
                add = False
        if add:
            out.append(part)
    return out


def ieee_div(a, b):
    if b != 0:
        return a / b
    if a == 0 or a != a:
        return float("nan")
    return math.copysign(float("inf"), a) * math.copysign(1.0, b)


def rpkm_per_region(region_lens, region_counts, read_len, num_total_reads):
    num_reads = float(sum(region_counts))
    num_positions_in_kb = sum(l - read_len + 1 for l in region_lens) / 1e3
    num_reads_in_millions = num_total_reads / 1e6
    return ieee_div(ieee_div(num_reads, num_positions_in_kb), num_reads_in_millions)


def compute(sam_text, gff_text, read_len):
    """(row dicts, the .rpkm file's text, the lines printed by the gene loop and the closing summary)."""
    refs, recs = parse_sam(sam_text)
    num_total_reads = len(recs)
    rows, lines, too_small = [], [], []
    num_genes = num_no_const = 0
    for gene_id, chrom, transcripts in parse_genes(gff_text):
        const = const_parts(transcripts)
        if "random" in chrom:
            lines.append("Skipping random chromosome gene: %s, %s" % (gene_id, chrom))
            continue
        if len(const) == 0:
            lines.append("Gene %s has no constitutive regions!" % gene_id)
            num_no_const += 1
            continue
        name = resolve(refs, chrom)
        num_reads, exon_lens, counted = [], [], {}
        total = 0
        for start, end in const:
            exon_len = end - start + 1
            if name is None:
                lines.append("Error fetching region: %s:%d-%d" % (chrom, start, end))
                break
            counts = fetch_count(recs, name, start, end)
            total += counts
            if (start, end) in counted or exon_len < read_len:
                continue
            exon_lens.append(exon_len)
            num_reads.append(counts)
            counted[(start, end)] = True
        if len(counted) == 0:
            too_small.append((gene_id, total))
            continue
        rpkm = rpkm_per_region(exon_lens, num_reads, read_len, num_total_reads)
        rows.append({"gene_id": gene_id, "rpkm": "%.2f" % rpkm,
                     "const_exon_lens": ",".join(str(e) for e in exon_lens),
                     "num_reads": ",".join(str(n) for n in num_reads)})
        num_genes += 1
    lines.append("Computed RPKMs for %d genes." % num_genes)
    lines.append("  - Total of %d genes cannot be used because they lack const. regions." % num_no_const)
    lines.append("  - Total of %d genes cannot be used since their exons are too small." % len(too_small))
    for gene_id, total in too_small:
        lines.append("      gene_id\ttotal_counts")
        lines.append("    * %s\t%d" % (gene_id, total))
    text = "gene_id\trpkm\tconst_exon_lens\tnum_reads\n" + "".join(
        "%s\t%s\t%s\t%s\n" % (r["gene_id"], r["rpkm"], r["const_exon_lens"], r["num_reads"]) for r in rows)
    return rows, text, lines
