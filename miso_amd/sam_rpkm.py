"""sam_rpkm --compute-rpkm: the RPKM of every gene of a GFF3 annotation from the reads on its constitutive exons
(misopy/sam_rpkm.py; names kept).

    python -m miso_amd.sam_rpkm --compute-rpkm GENES.gff READS.bam OUT_DIR --read-len L [--device D]

writes OUT_DIR/<basename of READS.bam>.rpkm: a header `gene_id rpkm const_exon_lens num_reads` and one tab-separated
row per gene, rpkm as %.2f, the two list columns comma-joined integers.

Per gene (sam_rpkm.py:109-195), odd parts included:
  * a gene whose chromosome name contains "random" is skipped with a message;
  * a gene without constitutive parts (gene_utils.Gene.get_const_parts) is counted and reported, no row;
  * every constitutive part is counted with bamfile.fetch(chrom, part.start, part.end) -- the GFF's 1-based inclusive
    numbers in pysam's 0-based half-open slot, as the reference has it -- and added to the gene's total; an exon all T
    transcripts share is T parts and adds its count T times;
  * a part joins const_exon_lens / num_reads only when its (start, end) is new in this gene and
    end - start + 1 >= read_len;
  * a gene with nothing joined goes to the "exons are too small" list with its total, no row;
  * rpkm = (sum of counts / (sum of (len - read_len + 1) / 1e3)) / (records in the file / 1e6), in doubles.

The reference fetches once per constitutive exon, 10^5 - 10^6 index look-ups for a genome annotation.  Here all
constitutive parts of all genes go to the device in ONE capi.fetch_counts call per file (csrc/kernels_rpkm.hip: one
thread per record, two integer rank histograms, a difference of prefix sums per interval).  There is
no per-exon fetch on the host and no CPU path.

Deliberate deviations from the reference:
  1. Row order.  Rows and the too-small list come in GFF order (the reference iterates a Python 2 dict).
  2. Chromosome names.  A gene's chromosome is spelled as the file spells it (sam_utils.resolve_chrom: unchanged when
     the file has it, else without its first "chr"), as every other tool here does; the reference forces a "chr"
     prefix.  Messages print the annotation's own spelling.
  3. Absent chromosome.  A gene whose chromosome the file lacks even then prints `Error fetching region: ...` for its
     first part and lands in the too-small list with total 0 -- what the reference's `break` out of the part loop
     amounts to.
"""
import argparse
import csv
import os
import sys
import time

import numpy as np

from miso_amd import capi, sam_utils
from miso_amd.gene_utils import load_genes_from_gff

RPKM_FIELDNAMES = ["gene_id", "rpkm", "const_exon_lens", "num_reads"]


def rpkm_per_region(region_lens, region_counts, read_len, num_total_reads):
    """RPKM of a set of regions (their lengths) and the counts in them, for the given read length.  Doubles, in the
    reference's order of operations; a zero total divides as IEEE does (nan or inf), never an exception."""
    lens = np.array(region_lens, dtype=np.int64)
    num_reads = np.float64(np.sum(np.array(region_counts, dtype=np.int64)))
    with np.errstate(divide="ignore", invalid="ignore"):
        num_positions_in_kb = np.float64(np.sum(lens - read_len + 1)) / 1e3    # mappable positions, in KB
        num_reads_in_millions = np.float64(num_total_reads) / 1e6
        return float((num_reads / num_positions_in_kb) / num_reads_in_millions)


def count_total_reads(bam_filename, bamfile=None):
    """Every record of the file (the reference iterates it and counts).  bamfile: the file already open."""
    if bamfile is None:
        bamfile = sam_utils.load_bam_reads(bam_filename)
    return len(bamfile)


def _gene_chrom(bamfile, gene):
    """The file's name of the gene's chromosome; None when the file does not have it."""
    name = sam_utils.resolve_chrom(bamfile, gene.chrom)
    return name if name in bamfile.references else None


def _fetched_genes(gff_genes, bamfile):
    """(gene id, gene, chromosome as the file names it, constitutive parts) of the genes whose parts are fetched, in
    GFF order: not on a "random" chromosome, with constitutive parts, on a chromosome the file has."""
    for gene_id, gene_info in gff_genes.items():
        gene = gene_info["gene_object"]
        if "random" in gene.chrom:
            continue
        const_exons = gene.get_const_parts()
        chrom = _gene_chrom(bamfile, gene)
        if const_exons and chrom is not None:
            yield gene_id, gene, chrom, const_exons


def const_part_intervals(gff_genes, bamfile):
    """(seqids, starts, ends) of every constitutive part, copies included, of every fetched gene: the one interval list
    of the file's device pass, in the order gene_rpkms reads the counts back."""
    seqids, starts, ends = [], [], []
    for _, _, chrom, const_exons in _fetched_genes(gff_genes, bamfile):
        for exon in const_exons:
            seqids.append(chrom)
            starts.append(exon.start)
            ends.append(exon.end)
    return seqids, starts, ends


def gene_rpkms(gff_genes, bamfile, counts, read_len, num_total_reads):
    """The per-gene rules over counts, one per interval of const_part_intervals(gff_genes, bamfile).  Prints the
    reference's per-gene messages and closing summary; returns (row dicts, genes without constitutive parts,
    [(gene id, total) of the genes whose exons are too small])."""
    fetched = {gene_id: chrom for gene_id, _, chrom, _ in _fetched_genes(gff_genes, bamfile)}
    rpkms_dictlist, exons_too_small = [], []
    num_genes = num_no_const = at = 0
    for gene_id, gene_info in gff_genes.items():
        gene = gene_info["gene_object"]
        const_exons = gene.get_const_parts()
        if "random" in gene.chrom:
            print("Skipping random chromosome gene: %s, %s" % (gene_id, gene.chrom))
            continue
        if len(const_exons) == 0:
            print("Gene %s has no constitutive regions!" % gene_id)
            num_no_const += 1
            continue
        if gene_id not in fetched:
            print("Error fetching region: %s:%d-%d" % (gene.chrom, const_exons[0].start, const_exons[0].end))
            exons_too_small.append((gene_id, 0))
            continue
        num_reads, exon_lens, regions_counted = [], [], set()
        total_num_reads = 0
        for exon in const_exons:
            exon_len = exon.end - exon.start + 1
            n = int(counts[at])
            at += 1
            total_num_reads += n
            # exons seen already in this gene, and exons shorter than the read length, only add to the total
            if (exon.start, exon.end) in regions_counted or exon_len < read_len:
                continue
            exon_lens.append(exon_len)
            num_reads.append(n)
            regions_counted.add((exon.start, exon.end))
        if not regions_counted:
            exons_too_small.append((gene_id, total_num_reads))
            continue
        rpkm = rpkm_per_region(exon_lens, num_reads, read_len, num_total_reads)
        rpkms_dictlist.append({"gene_id": gene_id,
                               "rpkm": "%.2f" % rpkm,
                               "const_exon_lens": ",".join(str(e) for e in exon_lens),
                               "num_reads": ",".join(str(n) for n in num_reads)})
        num_genes += 1
    if at != len(counts):
        raise ValueError("%d counts for %d constitutive parts" % (len(counts), at))
    print("Computed RPKMs for %d genes." % num_genes)
    print("  - Total of %d genes cannot be used because they lack const. regions." % num_no_const)
    print("  - Total of %d genes cannot be used since their exons are too small." % len(exons_too_small))
    for gene_id, total_counts in exons_too_small:
        print("      gene_id\ttotal_counts")
        print("    * %s\t%d" % (gene_id, total_counts))
    return rpkms_dictlist, num_no_const, exons_too_small


def write_rpkms(rpkms_dictlist, output_filename):
    """parse_csv.dictlist2file: the header, then one tab-separated row per gene, "\\n" line ends."""
    with open(output_filename, "w", newline="") as out:
        out.write("\t".join(RPKM_FIELDNAMES) + "\n")
        rows = csv.DictWriter(out, RPKM_FIELDNAMES, delimiter="\t", lineterminator="\n", extrasaction="ignore")
        for row in rpkms_dictlist:
            rows.writerow(row)


def compute_rpkm(gff_filename, bam_filename, read_len, output_dir, device=0):
    """RPKMs of the genes of gff_filename from the reads of bam_filename; writes <output_dir>/<bam basename>.rpkm and
    returns the row dicts."""
    print("Computing RPKMs...")
    print("  - GFF filename: %s" % gff_filename)
    print("  - BAM filename: %s" % bam_filename)
    print("  - Output dir: %s" % output_dir)
    os.makedirs(output_dir, exist_ok=True)
    output_filename = os.path.join(output_dir, "%s.rpkm" % os.path.basename(bam_filename))
    print("Outputting RPKMs to: %s" % output_filename)

    print("Parsing GFF into genes...")
    t1 = time.time()
    gff_genes = load_genes_from_gff(gff_filename)
    print("Parsing took %.2f seconds" % (time.time() - t1))

    bamfile = sam_utils.load_bam_reads(bam_filename)
    print("Counting all reads...")
    t1 = time.time()
    num_total_reads = count_total_reads(bam_filename, bamfile=bamfile)
    print("Took: %.2f seconds" % (time.time() - t1))
    print("Number of total reads in BAM file: %d" % num_total_reads)

    # every constitutive part of every gene: one pass over the records on the device
    seqids, starts, ends = const_part_intervals(gff_genes, bamfile)
    counts, st = capi.fetch_counts(bamfile, seqids, starts, ends, device=device)
    print("Counted %d constitutive parts over %d records: device pass %.3f s (tables %.3f s, record pass %.3f s in %d "
          "chunks, rank step %.3f s)" % (len(seqids), num_total_reads, st["total_ms"] / 1e3, st["sort_ms"] / 1e3,
                                         st["records_ms"] / 1e3, st["chunks"], st["rank_ms"] / 1e3))
    rpkms_dictlist, _, _ = gene_rpkms(gff_genes, bamfile, counts, read_len, num_total_reads)
    write_rpkms(rpkms_dictlist, output_filename)
    sys.stdout.flush()
    return rpkms_dictlist


def main(argv=None):
    parser = argparse.ArgumentParser(prog="sam_rpkm", description="RPKM of genes from the reads on their constitutive "
                                                                  "exons.")
    parser.add_argument("--compute-rpkm", dest="compute_rpkm", nargs=3, metavar=("GFF", "BAM", "OUT_DIR"), default=None,
                        help="Compute RPKMs.  Takes a GFF file with genes, a BAM/SAM file and an output directory.")
    parser.add_argument("--read-len", dest="read_len", type=int, default=0,
                        help="Read length to use for RPKM computation.")
    parser.add_argument("--device", dest="device", type=int, default=0, help="HIP device. Default 0.")
    options = parser.parse_args(argv)
    if options.compute_rpkm is not None:
        if options.read_len == 0:
            print("Error: Must give --read-len to compute RPKMs.")
            return 1
        gff_filename, bam_filename, output_dir = (os.path.abspath(os.path.expanduser(p))
                                                  for p in options.compute_rpkm)
        compute_rpkm(gff_filename, bam_filename, options.read_len, output_dir, device=options.device)
    return 0


if __name__ == "__main__":
    sys.exit(main())
