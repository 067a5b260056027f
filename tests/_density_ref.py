"""Test checker: a literal, slow restatement of sashimi_plot's read density and junction counts
(misopy/sashimi_plot/plot_utils/plot_gene.py:48-57, 398-444: bamfile.fetch + readsToWiggle_pysam) over SAM text, record by
record and base by base, sharing no code with the package.  Coordinates as the reference mixes them: `pos` 0-based,
tx_start / tx_end the GFF numbers unchanged.

Per region it gives the integer depth, the reference's own value (1. / qlen added into a float32 array in file order), the
exact value as fractions.Fraction (Region.exact), the junction dict, and what the bounds of the tests need: per base the
number of distinct qlen (Region.classes) and the number of records (the depth).
"""
import re
from fractions import Fraction

import numpy as np


class Rec(object):
    __slots__ = ("rname", "pos", "cigar", "end")

    def __init__(self, flag, rname, pos, cigar):
        self.rname, self.pos, self.cigar = rname, pos, cigar
        reflen = sum(n for op, n in cigar if op in "MDN=X") if cigar else 0
        # htslib bam_endpos: the spliced span; pos + 1 without a reference-consuming operation or when flagged unmapped
        self.end = pos + 1 if (flag & 4) or reflen == 0 else pos + reflen

    def positions(self):
        """pysam read.positions: the reference positions of the M, = and X bases."""
        out, x = [], self.pos
        for op, n in self.cigar:
            if op in "M=X":
                out.extend(range(x, x + n))
                x += n
            elif op in "DN":
                x += n
        return out

    def qlen(self):
        """pysam read.qlen: the query without its soft clips."""
        return sum(n for op, n in self.cigar if op in "MI=X")


def parse_sam(text):
    """(reference names of the header in order, records in file order)."""
    refs, recs = [], []
    for line in text.splitlines():
        if not line:
            continue
        if line.startswith("@"):
            if line.startswith("@SQ"):
                refs.append(dict(x.split(":", 1) for x in line.split("\t")[1:])["SN"])
            continue
        f = line.split("\t")
        cigar = None if f[5] == "*" else [(op, int(n)) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", f[5])]
        recs.append(Rec(int(f[1]), f[2], int(f[3]) - 1, cigar))
    return refs, recs


class Region(object):
    """What one region gets."""

    def __init__(self, length):
        self.depth = np.zeros(length, dtype=np.int64)
        self.float32 = np.zeros(length, dtype="f")     # the reference's array
        self.by_qlen = {}                              # base -> {qlen: records}, the bases with a record only
        self.jxns = {}                                 # (leftss, rightss) -> count
        self.fetched = self.multi_n = self.no_cigar = self.indel = 0
        self.d_junctions = 0                           # junctions counted from a D gap
        self.qlen_seen = set()

    def exact(self, w):
        """The density at base w as a rational number: the sum of 1 / qlen over its records."""
        return sum((Fraction(n, q) for q, n in self.by_qlen.get(w, {}).items()), Fraction(0))

    def classes(self, w):
        """Distinct qlen among the records at base w."""
        return len(self.by_qlen.get(w, ()))


def region(refs, recs, seqid, tx_start, tx_end):
    """Rules 1 - 7 for one region, alone; recs in file order (records of other references may be left out)."""
    out = Region(max(0, tx_end - tx_start + 1))
    if seqid not in refs or tx_start > tx_end:
        return out
    for r in recs:
        if r.rname != seqid or not (r.pos < tx_end and r.end > tx_start):
            continue
        out.fetched += 1
        if r.cigar is None:
            out.no_cigar += 1
            continue
        if sum(1 for op, _ in r.cigar if op == "N") > 1:
            out.multi_n += 1
            continue
        if any(op in "ID" for op, _ in r.cigar):
            out.indel += 1
        aligned = r.positions()
        if not aligned:
            continue
        qlen = r.qlen()
        out.qlen_seen.add(qlen)
        # which gaps a D made: the reference position right after each D
        after_d, x = set(), r.pos
        for op, n in r.cigar:
            if op in "M=X":
                x += n
            elif op in "DN":
                x += n
                if op == "D":
                    after_d.add(x)
        for i, pos in enumerate(aligned):
            if pos < tx_start or pos > tx_end:
                continue
            w = pos - tx_start
            out.depth[w] += 1
            out.float32[w] += 1. / qlen
            counts = out.by_qlen.setdefault(w, {})
            counts[qlen] = counts.get(qlen, 0) + 1
            if i + 1 < len(aligned) and aligned[i + 1] > pos + 1:
                leftss, rightss = pos + 1, aligned[i + 1] + 1
                if tx_start < leftss < tx_end and tx_start < rightss < tx_end:
                    out.jxns[(leftss, rightss)] = out.jxns.get((leftss, rightss), 0) + 1
                    if aligned[i + 1] in after_d:
                        out.d_junctions += 1
    return out


def regions(sam_text, triples):
    """[Region] for (seqid, tx_start, tx_end) triples, and the stats over all of them: records fetched by at least one
    region, of those skipped for more than one N / for no CIGAR, of the rest those with I or D, distinct qlen."""
    refs, recs = parse_sam(sam_text)
    by_name = {}
    for r in recs:
        by_name.setdefault(r.rname, []).append(r)
    out = [region(refs, by_name.get(s, []), s, a, b) for s, a, b in triples]
    fetched = multi_n = no_cigar = indel = 0
    qlens = set()
    live = [(s, a, b) for s, a, b in triples if s in refs and a <= b]
    by_ref = {}
    for s, a, b in live:
        by_ref.setdefault(s, []).append((a, b))
    for r in recs:
        if not any(r.pos < b and r.end > a for a, b in by_ref.get(r.rname, ())):
            continue
        fetched += 1
        if r.cigar is None:
            no_cigar += 1
        elif sum(1 for op, _ in r.cigar if op == "N") > 1:
            multi_n += 1
        else:
            if any(op in "ID" for op, _ in r.cigar):
                indel += 1
            if r.positions():
                qlens.add(r.qlen())
    stats = {"fetched": fetched, "skipped_multi_n": multi_n, "skipped_no_cigar": no_cigar, "with_indel": indel,
             "qlen_classes": len(qlens)}
    return out, stats


def bam_to_sam(path):
    """SAM text (@SQ lines and the eleven mandatory fields; SEQ and QUAL as `*`) of a BAM file, read with the standard
    library alone: BGZF is a series of gzip members (SAM spec v1 section 4.1), the records section 4.2."""
    import gzip
    import struct
    with gzip.open(path, "rb") as handle:
        data = handle.read()
    assert data[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<i", data, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, at)
    at += 4
    names, lines = [], []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, at)
        name = data[at + 4:at + 4 + l_name - 1].decode()
        l_ref, = struct.unpack_from("<i", data, at + 4 + l_name)
        at += 8 + l_name
        names.append(name)
        lines.append("@SQ\tSN:%s\tLN:%d" % (name, l_ref))
    while at < len(data):
        size, ref_id, pos, l_read_name, mapq, _bin, n_cigar, flag, l_seq, next_ref, next_pos, tlen = \
            struct.unpack_from("<iiiBBHHHiiii", data, at)
        body = at + 36
        qname = data[body:body + l_read_name - 1].decode()
        words = struct.unpack_from("<%dI" % n_cigar, data, body + l_read_name)
        cigar = "".join("%d%s" % (w >> 4, "MIDNSHP=X"[w & 15]) for w in words) or "*"
        rnext = "*" if next_ref < 0 else "=" if next_ref == ref_id else names[next_ref]
        lines.append("\t".join([qname, str(flag), names[ref_id] if ref_id >= 0 else "*", str(pos + 1), str(mapq), cigar,
                                rnext, str(next_pos + 1), str(tlen), "*", "*"]))
        at += 4 + size
    return "\n".join(lines) + "\n"
