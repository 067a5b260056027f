"""Test checker: a literal, slow restatement of `pe_utils --compute-insert-len` (misopy/pe_utils.py:148-302, 422-494;
exon_utils.py:110-196; sam_utils.py:194-290) and of `exon_utils --get-const-exons` (exon_utils.py:42-83, 253-318), over
SAM text and GFF text, sharing no code with the package.  With the two deviations DESIGN.md section 9 states: the sd
filter removes by value, and regions come in GFF order, inserts inside a region in file order of the left mate.
"""
import math
import re
from urllib.parse import unquote

TAG_NONE, TAG_MULTI = 0x1FFFFFFF, 0x1FFFFFFE
ONE_M, FILTER_OK = 1 << 29, 1 << 30


class Rec(object):
    __slots__ = ("name", "flag", "rname", "pos", "cigar", "end")

    def __init__(self, name, flag, rname, pos, cigar):
        self.name, self.flag, self.rname, self.pos, self.cigar = name, flag, rname, pos, cigar
        reflen = sum(n for op, n in cigar if op in "MDN=X")
        # htslib bam_endpos
        self.end = pos + 1 if (flag & 4) or reflen == 0 else pos + reflen


def parse_sam(text):
    recs = []
    for line in text.splitlines():
        if not line or line.startswith("@"):
            continue
        f = line.split("\t")
        cigar = [] if f[5] == "*" else [(op, int(n)) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", f[5])]
        recs.append(Rec(f[0], int(f[1]), f[2], int(f[3]) - 1, cigar))
    return recs


class Interval(object):
    __slots__ = ("seqid", "start", "end", "strand")

    def __init__(self, seqid, start, end, strand):
        self.seqid, self.start, self.end, self.strand = seqid, start, end, strand

    def name(self):
        return "%s:%d-%d:%s" % (self.seqid, self.start, self.end, self.strand)


def parse_gff(text):
    """Every record line as a dict: seqid, type, start, end, strand, attrs (tag -> [values])."""
    out = []
    for line in text.splitlines():
        if not line.strip() or line.startswith("#"):
            continue
        if line.startswith(">"):
            break
        c = line.rstrip("\n").split("\t")
        start, end = int(c[3]), int(c[4])
        if start > end:
            start, end = end, start
        attrs = {}
        for pair in filter(None, c[8].split(";")):
            tag, _, value = pair.partition("=")
            attrs[unquote(tag)] = [unquote(v) for v in value.split(",")]
        out.append({"seqid": unquote(c[0]), "type": c[2], "start": start, "end": end,
                    "strand": c[6] if c[6] != "." else None, "attrs": attrs})
    return out


def gff_intervals(text):
    return [Interval(r["seqid"], r["start"], r["end"], r["strand"] or ".") for r in parse_gff(text)]


# ---- step 1: tagBam -f 1, strand ignored ----
def tags(rec, intervals):
    if rec.flag & 4 or rec.rname == "*":
        return []
    return [k for k, iv in enumerate(intervals)
            if iv.seqid == rec.rname and iv.start - 1 <= rec.pos and rec.end <= iv.end]


def passes_filter(rec, filter_reads):
    if not filter_reads:
        return True
    return not (rec.flag & 0x200) and not (rec.flag & 0x4) and not (rec.flag & 0x8) and bool(rec.flag & 0x1)


def one_m(rec):
    return len(rec.cigar) == 1 and rec.cigar[0][0] == "M"


def record_codes(recs, intervals, filter_reads=True):
    """The MISO_INSERT_* code of every record (include/miso_alnio.h)."""
    out = []
    for r in recs:
        t = tags(r, intervals)
        code = TAG_NONE if not t else (t[0] if len(t) == 1 else TAG_MULTI)
        out.append(code | (ONE_M if one_m(r) else 0) | (FILTER_OK if passes_filter(r, filter_reads) else 0))
    return out


def strip_mate_id(name):
    if name.endswith("/1") or name.endswith("/2") or name.endswith("#1") or name.endswith("#2"):
        name = name[0:-3]
    return name


def insert_len(recs, intervals, filter_reads=True):
    """Steps 1-3: ({interval index: [inserts]} in GFF order, counts)."""
    tagged = [(r, tags(r, intervals)) for r in recs]
    tagged = [(r, t) for r, t in tagged if t]
    groups = {}                                   # insertion order = first appearance
    for r, t in tagged:
        if not passes_filter(r, filter_reads):
            continue
        groups.setdefault(strip_mate_id(r.name), []).append((r, t))
    counts = {"kept": 0, "skipped": 0, "unpaired": 0, "same_strand": 0, "nonpositive": 0,
              "tagged": sum(len(g) for g in groups.values())}
    by_interval = {}
    for members in groups.values():
        if len(members) != 2:
            counts["unpaired"] += 1
            continue
        (left, lt), (right, rt) = members
        if bool(left.flag & 0x10) == bool(right.flag & 0x10):
            counts["same_strand"] += 1
            continue
        if (len(lt) != 1 or len(rt) != 1 or intervals[lt[0]].name() != intervals[rt[0]].name()
                or not one_m(left) or not one_m(right)):
            counts["skipped"] += 1
            continue
        insert = right.pos + right.cigar[0][1] - left.pos
        if insert <= 0:
            counts["nonpositive"] += 1
            continue
        by_interval.setdefault(lt[0], []).append(insert)
        counts["kept"] += 1
    return {k: by_interval[k] for k in sorted(by_interval)}, counts


# ---- step 4 ----
def _stats(values):
    n = len(values)
    mu = math.fsum(values) / n
    sd = math.sqrt(math.fsum((v - mu) ** 2 for v in values) / n)
    return mu, sd, sd / math.sqrt(mu), n


def summarize(by_interval, intervals, sd_max=2):
    """(the file's text, (mu, sd, dispersion, n)); None when nothing is left."""
    every = [v for vs in by_interval.values() for v in vs]
    if not every:
        return None
    mu, sd, _, _ = _stats(every)
    lo, hi = mu - sd_max * sd, mu + sd_max * sd
    kept = [(k, [v for v in vs if lo <= v <= hi]) for k, vs in by_interval.items()]
    kept = [(k, vs) for k, vs in kept if vs]
    if not kept:
        return None
    stats = _stats([v for _, vs in kept for v in vs])
    text = "#mean=%.1f,sdev=%.1f,dispersion=%.1f,num_pairs=%d\n#region\tinsert_len\n" % stats
    text += "".join("%s\t%s\n" % (intervals[k].name(), ",".join(map(str, vs))) for k, vs in kept)
    return text, stats


# ---- exon_utils --get-const-exons ----
def const_exons(gff_text, min_size=20):
    """[(seqid, start, end, strand, gene id)] in GFF order."""
    recs = parse_gff(gff_text)
    ident = lambda r: r["attrs"].get("ID", [""])[0].rstrip()
    parent = lambda r: r["attrs"].get("Parent", [""])[0].rstrip()
    transcripts, exons = {}, {}
    for r in recs:
        if r["type"] in ("mRNA", "transcript"):
            transcripts.setdefault(parent(r), []).append(r)
        elif r["type"] == "exon":
            exons.setdefault(parent(r), []).append(r)
    chosen = []
    for gene, ts in transcripts.items():
        for ex in exons.get(ident(ts[0]), []):
            if ex["end"] - ex["start"] + 1 < min_size:
                continue
            if all(any((o["start"], o["end"], o["strand"]) == (ex["start"], ex["end"], ex["strand"])
                       for o in exons.get(ident(t), [])) for t in ts[1:]):
                chosen.append((id(ex), gene))
    place = {id(r): k for k, r in enumerate(recs)}
    chosen.sort(key=lambda c: place[c[0]])
    by_id = {id(r): r for r in recs}
    return [(by_id[i]["seqid"], by_id[i]["start"], by_id[i]["end"], by_id[i]["strand"], g) for i, g in chosen]
