"""Test checker: a literal, slow restatement of the coverage table of `miso --run --prefilter` (misopy/exon_utils.py:198-250:
`bedtools intersect -abam BAM -b genes.gff -f 1 -ubam | bedtools coverage -abam - -b genes.gff -counts`) and of its
filter (run_events_analysis.py:28-68), over SAM text and GFF text, sharing no code with the package.  With the two
deviations DESIGN.md section 10 states: seqids map to the file's references the way the run maps them (a "chr" prefix
the file lacks is dropped), and the table comes in GFF order.
"""
import re
from urllib.parse import unquote


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


def gff_lines(text):
    """The fields of every interval line: not a comment, at least 9 tab-separated fields."""
    out = []
    for line in text.splitlines():
        if line.startswith("#"):
            continue
        fields = line.split("\t")
        if len(fields) >= 9:
            out.append(fields)
    return out


def resolve(refs, seqid):
    """The file's name for a seqid: itself, else without its first "chr"; None if the file has neither."""
    if seqid in refs:
        return seqid
    pieces = seqid.split("chr")
    name = pieces[1] if len(pieces) > 1 else pieces[0]
    return name if name in refs else None


def counts(sam_text, gff_text):
    refs, recs = parse_sam(sam_text)
    ivs = []
    for f in gff_lines(gff_text):
        ivs.append((resolve(refs, f[0]), int(f[3]), int(f[4])))
    # intersect -f 1: mapped records whose whole span some interval on their reference holds
    kept = []
    for r in recs:
        if r.flag & 4 or r.rname == "*":
            continue
        for name, start, end in ivs:
            if name == r.rname and start - 1 <= r.pos and r.end <= end:
                kept.append(r)
                break
    # coverage -counts: kept records overlapping [start - 1, end)
    out = []
    for name, start, end in ivs:
        n = 0
        if name is not None and start <= end:
            for r in kept:
                if r.rname == name and r.pos < end and r.end > start - 1:
                    n += 1
        out.append(n)
    return out


def table(sam_text, gff_text):
    """The coverage table's text: each interval line's fields, a tab and its count, in GFF order."""
    return "".join("%s\t%d\n" % ("\t".join(f), n) for f, n in zip(gff_lines(gff_text), counts(sam_text, gff_text)))


def passing_ids(table_text, min_event_reads):
    """(IDs of the lines with count >= min_event_reads, lines with such a count but no ID)."""
    ids, no_id = [], []
    for line in table_text.splitlines():
        if line.startswith("#"):
            continue
        fields = line.split("\t")
        if int(fields[-1]) < min_event_reads:
            continue
        found = None
        for pair in fields[8].split(";"):
            tag, sep, value = pair.partition("=")
            if sep and "=" not in value and unquote(tag) == "ID":
                found = unquote(value.split(",")[0]).rstrip()
        if found is None:
            no_id.append(line)
        else:
            ids.append(found)
    return ids, no_id
