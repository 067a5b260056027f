"""exon_utils --get-const-exons: the constitutive exons of a GFF3 annotation (misopy/exon_utils.py:42-83, 253-318,
331-369), the first step of the fragment-length recipe (`pe_utils --compute-insert-len` takes the file it writes).

Per gene: the exons of its first transcript whose length (end - start + 1) is at least --min-exon-size and which every
other transcript of the gene has too (same start, end and strand).  Each is written with the attribute
`GeneParent=<gene id>` added, to `<output dir>/<GFF basename without .gff/.gff3>.min_<N>.const_exons.gff`, in the order
the records have in the input (the reference's order comes from a dict).

Also the read coverage of `miso --run --prefilter` (exon_utils.py:198-250): `get_bam_gff_coverage` writes
`<output dir>/<BAM basename without .bam>.bed`, every interval line of the GFF followed by a tab and the number of
records that lie whole inside some interval and overlap this one -- what `bedtools intersect -f 1 -ubam | bedtools
coverage -counts` writes, counted on the GPU (csrc/kernels_coverage.hip, include/miso_alnio.h miso_region_counts), in
GFF order.  `get_ids_passing_filter` reads the IDs of the lines with at least min_event_reads.
"""
import argparse
import os
import re
import sys
import time

from miso_amd import gff_utils

# GFF3 column 9: these characters are escaped inside tags and values; columns 1-8 escape tab, newline and '%'
_ATTR_ESCAPE = re.compile(r"[\t\n\r\f\v;=%&,]")
_COLUMN_ESCAPE = re.compile(r"[\t\n\r%]")


def _escape(pattern, text):
    return pattern.sub(lambda m: "%%%02X" % ord(m.group(0)), text)


def is_exon_in_mRNA(gff_db, exon, mRNA):
    """Does the transcript have an exon with the same start, end and strand?"""
    return any(e.start == exon.start and e.end == exon.end and e.strand == exon.strand
               for e in gff_db.exons_by_mRNA.get(mRNA.get_id(), []))


def get_const_exons_from_mRNA(gff_db, mRNAs, min_size=0):
    """The constitutive exons of one gene (its transcripts `mRNAs`, file order), GeneParent set."""
    first = mRNAs[0]
    gene_id = first.get_parent()
    const = []
    for exon in gff_db.exons_by_mRNA.get(first.get_id(), []):
        if exon.end - exon.start + 1 < min_size:
            continue
        if all(is_exon_in_mRNA(gff_db, exon, m) for m in mRNAs[1:]):
            exon.attributes["GeneParent"] = [gene_id]
            const.append(exon)
    return const


def get_const_exons(gff_filename, min_size=0):
    """Every gene's constitutive exons, in the order of the input file."""
    gff_db = gff_utils.GFFDatabase(from_filename=gff_filename)
    place = {id(rec): k for k, rec in enumerate(gff_db.exons)}
    const = []
    for mRNAs in gff_db.mRNAs_by_gene.values():
        const.extend(get_const_exons_from_mRNA(gff_db, mRNAs, min_size=min_size))
    return sorted(const, key=lambda rec: place[id(rec)])


def const_exons_filename(gff_filename, output_dir, min_size):
    basename = re.sub("[.]gff3?", "", os.path.basename(gff_filename))
    return os.path.join(output_dir, "%s.min_%d.const_exons.gff" % (basename, min_size))


def _field(value):
    return "." if value is None or value == "" else str(value)


def format_record(rec):
    """One GFF3 line (no newline)."""
    attrs = ";".join("%s=%s" % (_escape(_ATTR_ESCAPE, tag), ",".join(_escape(_ATTR_ESCAPE, v) for v in values))
                     for tag, values in rec.attributes.items())
    return "\t".join([_escape(_COLUMN_ESCAPE, rec.seqid), _escape(_COLUMN_ESCAPE, rec.source),
                      _escape(_COLUMN_ESCAPE, rec.type), str(rec.start), str(rec.end), _field(rec.score),
                      _field(rec.strand), _field(rec.phase), _field(attrs)])


def write_gff(records, output_filename):
    with open(output_filename, "w") as out:
        out.write("##gff-version 3\n")
        for rec in records:
            out.write(format_record(rec) + "\n")


def get_const_exons_by_gene(gff_filename, output_dir, min_size=0):
    """Write the constitutive exons of `gff_filename` into output_dir; returns (records, output filename)."""
    os.makedirs(output_dir, exist_ok=True)
    t0 = time.time()
    const = get_const_exons(gff_filename, min_size=min_size)
    output_filename = const_exons_filename(gff_filename, output_dir, min_size)
    write_gff(const, output_filename)
    print("Constitutive exons: %d (at least %d bp) in %.2f s -> %s"
          % (len(const), min_size, time.time() - t0, output_filename))
    return const, output_filename


# ---- read coverage per interval: `miso --run --prefilter` ----
def coverage_filename(bam_filename, output_dir):
    """<output_dir>/<BAM basename with ".bam" removed, case-insensitive>.bed (exon_utils.py:232-234)."""
    output_basename = re.sub(r"\.bam", "", os.path.basename(bam_filename), flags=re.IGNORECASE)
    return "%s.bed" % os.path.join(output_dir, output_basename)


def read_coverage_intervals(gff_filename):
    """The fields of every line that is an interval: not a comment, at least 9 tab-separated fields."""
    out = []
    with open(gff_filename) as stream:
        for line in stream:
            if line.startswith("#"):
                continue
            fields = line.rstrip("\r\n").split("\t")
            if len(fields) >= 9:
                out.append(fields)
    return out


def coverage_counts(bamfile, intervals, device=0, chunk_records=0):
    """(counts per interval, stats of the device pass) of an open alignment file (sam_utils.Samfile); a seqid maps to
    the file's reference the way the run maps it (sam_utils.resolve_chrom)."""
    from miso_amd import capi, sam_utils
    return capi.region_counts(bamfile, [sam_utils.resolve_chrom(bamfile, f[0]) for f in intervals],
                              [int(f[3]) for f in intervals], [int(f[4]) for f in intervals], device=device,
                              chunk_records=chunk_records)


def format_coverage(intervals, counts):
    return "".join("%s\t%d\n" % ("\t".join(f), c) for f, c in zip(intervals, counts))


def compute_bam_gff_coverage(bam_filename, gff_filename, output_filename, bamfile=None, device=0, chunk_records=0):
    """Count on the device and write the table (under a temporary name first: a partly written table is never taken
    for a finished one).  bamfile: the file already open, else it is opened here.  Returns the pass's stats."""
    from miso_amd import sam_utils
    t0 = time.time()
    own = bamfile is None
    if own:
        bamfile = sam_utils.Samfile(bam_filename)
    t_decode = time.time() - t0
    intervals = read_coverage_intervals(gff_filename)
    counts, st = coverage_counts(bamfile, intervals, device=device, chunk_records=chunk_records)
    n_records = len(bamfile)
    if own:
        bamfile.close()
    tmp = "%s.tmp%d" % (output_filename, os.getpid())
    with open(tmp, "w") as out:
        out.write(format_coverage(intervals, counts))
    os.replace(tmp, output_filename)
    print("Coverage of %d intervals from %d records (%d kept): decode %.3f s, device pass %.3f s (tables %.3f s, "
          "record pass %.3f s in %d chunks, rank step %.3f s)"
          % (len(intervals), n_records, st["kept"], t_decode, st["total_ms"] / 1e3, st["sort_ms"] / 1e3,
             st["records_ms"] / 1e3, st["chunks"], st["rank_ms"] / 1e3))
    sys.stdout.flush()
    return st


def get_bam_gff_coverage(bam_filename, gff_filename, output_dir, compute=None):
    """Write (or reuse) the coverage table of bam_filename over the intervals of gff_filename; returns its path.
    compute(bam_filename, gff_filename, output_filename) writes the table (default: compute_bam_gff_coverage in this
    process)."""
    if not os.path.isfile(bam_filename):
        raise IOError("BAM file %s does not exist." % bam_filename)
    if not os.path.isfile(gff_filename):
        raise IOError("GFF file %s does not exist." % gff_filename)
    os.makedirs(output_dir, exist_ok=True)
    output_filename = coverage_filename(bam_filename, output_dir)
    print("Generating coverage file...")
    print("  - BAM file: %s" % bam_filename)
    print("  - GFF file: %s" % gff_filename)
    print("  - Output file: %s" % output_filename)
    if os.path.isfile(output_filename):
        print("  - File exists. Skipping...")
        return output_filename
    (compute or compute_bam_gff_coverage)(bam_filename, gff_filename, output_filename)
    return output_filename


def get_ids_passing_filter(coverage_filename, min_event_reads):
    """IDs of the table's lines whose count (the last field) is at least min_event_reads, in table order
    (run_events_analysis.py:49-68); a passing line without an ID is reported and skipped."""
    ids = []
    with open(coverage_filename) as coverage_in:
        for line in coverage_in:
            if line.startswith("#"):
                continue
            fields = line.rstrip("\r\n").split("\t")
            if int(fields[-1]) < min_event_reads:
                continue
            values = gff_utils.parse_gff_attribs(fields[8]).get("ID")
            if not values:
                print("WARNING: No ID= found for line:\n%s\nSkipping..." % line)
                continue
            ids.append(values[0].rstrip())
    return ids


def main(argv=None):
    parser = argparse.ArgumentParser(prog="exon_utils", description="Constitutive exons of a GFF3 annotation.")
    parser.add_argument("--get-const-exons", dest="get_const_exons", metavar="GFF", default=None,
                        help="Get constitutive exons from an input GFF file.")
    parser.add_argument("--min-exon-size", dest="min_exon_size", type=int, default=20,
                        help="Minimum size of a constitutive exon (in nucleotides). Default is 20 bp.")
    parser.add_argument("--output-dir", dest="output_dir", default=None, help="Output directory.")
    options = parser.parse_args(argv)
    if options.get_const_exons is None or options.output_dir is None:
        parser.print_help(sys.stderr)
        return 1
    get_const_exons_by_gene(os.path.abspath(os.path.expanduser(options.get_const_exons)),
                            os.path.abspath(os.path.expanduser(options.output_dir)),
                            min_size=options.min_exon_size)
    return 0


if __name__ == "__main__":
    sys.exit(main())
