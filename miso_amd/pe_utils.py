"""pe_utils --compute-insert-len: the fragment (insert) length distribution of paired-end alignments, from the read
pairs that fall inside one interval of a GFF -- usually the constitutive exons `exon_utils --get-const-exons` writes
(misopy/pe_utils.py:148-302, 422-494).  Its mean and sd are what `miso --run ... --paired-end MEAN SD` takes.

Tagging every record with the intervals that contain it, pairing by name and measuring the pairs run natively, the
per-record and per-pair work on the GPU (csrc/kernels_insert.hip, include/miso_alnio.h miso_insert_len); no
intermediate BAM, no bedtools or samtools.  Here: the statistics (numpy) and the `<bam>.insert_len` file:

    #mean=...,sdev=...,dispersion=...,num_pairs=...
    #region\tinsert_len
    chrom:start-end:strand\t<inserts, comma-separated>      (one line per interval with any, in GFF order)

Two deliberate differences from the reference: outliers beyond sd_max deviations are removed
by value (the reference deletes by indices computed on another array, so its result depends on dict order), and the
order of regions and of the inserts inside a line is defined (GFF order; file order of the left mate).
"""
import argparse
import os
import sys
import time
from collections import OrderedDict

import numpy as np

from miso_amd import capi, gff_utils, sam_utils


class InsertLenError(Exception):
    """No pair is left to compute the distribution from."""


def interval_name(rec):
    """chrom:start-end:strand, the region key of the output (pe_utils.py:131-142)."""
    return "%s:%d-%d:%s" % (rec.seqid, rec.start, rec.end, rec.strand or ".")


def read_intervals(gff_filename):
    """Every record line of the GFF is an interval (tagBam -files GFF)."""
    with open(gff_filename) as stream:
        return list(gff_utils.Reader(stream))


def compute_insert_len_stats(insert_dist):
    """(mean, sd (ddof 0), sd / sqrt(mean), count) of an array of insert lengths (pe_utils.py:448-471)."""
    insert_dist = np.asarray(insert_dist, dtype=np.float64)
    mu = np.mean(insert_dist)
    sdev = np.std(insert_dist)
    return mu, sdev, sdev / np.sqrt(float(mu)), len(insert_dist)


def filter_insert_len(region_to_dists, sd_max):
    """Drop the inserts outside [mu - sd_max sd, mu + sd_max sd] of all regions together, by value."""
    values = [np.asarray(d) for d in region_to_dists.values()]
    mu, sdev, _, _ = compute_insert_len_stats(np.concatenate(values) if values else np.zeros(0))
    lo, hi = mu - sd_max * sdev, mu + sd_max * sdev
    return OrderedDict((region, d[(d >= lo) & (d <= hi)]) for region, d in zip(region_to_dists, values))


def format_header(mu, sdev, dispersion, num_pairs):
    return "#mean=%.1f,sdev=%.1f,dispersion=%.1f,num_pairs=%d\n" % (mu, sdev, dispersion, num_pairs)


def summarize_insert_len_dist(region_to_dists, output_filename, sd_max=2):
    """Filter, summarise and write `output_filename`; returns (mean, sdev, dispersion, num_pairs)."""
    filtered = filter_insert_len(region_to_dists, sd_max) if any(len(d) for d in region_to_dists.values()) else {}
    values = [d for d in filtered.values() if len(d)]
    if not values:
        raise InsertLenError("could not find any properly mated pairs to compute the insert length with: are the "
                             "BAM reads properly paired, and do they name the chromosomes of the GFF?")
    stats = compute_insert_len_stats(np.concatenate(values))
    lines = [format_header(*stats), "#region\tinsert_len\n"]
    lines += ["%s\t%s\n" % (region, ",".join(str(int(v)) for v in d)) for region, d in filtered.items() if len(d)]
    with open(output_filename, "w") as out:
        out.write("".join(lines))
    return stats


def parse_insert_len_params(insert_len_header):
    """'#mean=..,sdev=..,...' -> {name: text}."""
    header = insert_len_header.strip()
    if header.startswith("#"):
        header = header[1:]
    params = {}
    for param in header.split(","):
        name, value = param.split("=")
        params[name] = value
    return params


def load_insert_len(insert_dist_filename, delim="\t"):
    """(every insert length of the file as one array, the header's parameters)."""
    inserts = []
    with open(insert_dist_filename) as stream:
        params = parse_insert_len_params(stream.readline())
        for line in stream:
            if line.startswith("#"):
                continue
            fields = line.strip().split(delim)
            if len(fields) != 2:
                continue
            inserts.extend(int(v) for v in fields[1].split(","))
    return np.array(inserts, dtype=np.int64), params


def insert_lengths(bamfile, intervals, filter_reads=True, device=0, chunk_records=0):
    """The kept pairs of an open alignment file (sam_utils.Samfile) by region: (OrderedDict region -> inserts in file
    order of the left mate, regions in GFF order; the native pass's counts and stage times)."""
    iv, ins, stats = capi.insert_len(bamfile, [r.seqid for r in intervals], [r.start for r in intervals],
                                     [r.end for r in intervals], device=device, filter_reads=filter_reads,
                                     chunk_records=chunk_records)
    region_to_dists = OrderedDict()
    if len(iv):
        cut = np.flatnonzero(np.diff(iv)) + 1
        for first, part in zip(np.concatenate(([0], cut)), np.split(ins, cut)):
            region_to_dists.setdefault(interval_name(intervals[iv[first]]), []).append(part)
        region_to_dists = OrderedDict((k, np.concatenate(v)) for k, v in region_to_dists.items())
    return region_to_dists, stats


def compute_insert_len(bams_to_process, gff_filename, output_dir, min_exon_size=None, no_bam_filter=False,
                       sd_max=2, device=0, chunk_records=0):
    """One `<bam>.insert_len` per alignment file; returns {bam: output filename} of the files written.
    min_exon_size has no effect (the reference passes it to a computation whose result it never uses)."""
    os.makedirs(output_dir, exist_ok=True)
    intervals = read_intervals(gff_filename)
    filter_reads = not no_bam_filter
    written = OrderedDict()
    for bam_filename in bams_to_process:
        if not os.path.isfile(bam_filename):
            raise IOError("cannot find BAM file %s" % bam_filename)
        output_filename = os.path.join(output_dir, "%s.insert_len" % os.path.basename(bam_filename))
        t0 = time.time()
        bamfile = sam_utils.Samfile(bam_filename)
        t_decode = time.time() - t0
        region_to_dists, st = insert_lengths(bamfile, intervals, filter_reads=filter_reads, device=device,
                                             chunk_records=chunk_records)
        n_records = len(bamfile)
        bamfile.close()
        pairs = st["kept"] + st["skipped"] + st["nonpositive"]   # the reference's paired mates (same strand dropped)
        print("%s: %d records, %d tagged; %d read pairs, %d unpaired names, %d pairs on the same strand"
              % (bam_filename, n_records, st["tagged"], pairs, st["unpaired"], st["same_strand"]))
        if pairs == 0:
            sys.stderr.write("WARNING: no paired mates in %s. Skipping... Are you sure the read IDs match? If your BAM "
                             "paired flags are unset, try using --no-bam-filter.\n" % bam_filename)
            continue
        if st["nonpositive"]:
            sys.stderr.write("WARNING: %d pairs with an insert length <= 0 dropped (left mate later in the file, "
                             "e.g. a name-sorted BAM)\n" % st["nonpositive"])
        print("Used %d paired mates, threw out %d" % (st["kept"], st["skipped"]))
        t1 = time.time()
        mu, sdev, dispersion, num_pairs = summarize_insert_len_dist(region_to_dists, output_filename, sd_max=sd_max)
        t_write = time.time() - t1
        print("mean\tsdev\tdispersion\n%.1f\t%.1f\t%.1f\nnum_pairs %d -> %s"
              % (mu, sdev, dispersion, num_pairs, output_filename))
        sys.stderr.write("insert_len %s: decode %.3f s, record pass %.3f s (%d chunks, %.3g records/s), grouping "
                         "%.3f s, pair pass %.3f s, write %.3f s\n"
                         % (os.path.basename(bam_filename), t_decode, st["records_ms"] / 1e3, st["chunks"],
                            n_records / max(st["records_ms"] / 1e3, 1e-9), st["grouping_ms"] / 1e3,
                            st["pairs_ms"] / 1e3, t_write))
        written[bam_filename] = output_filename
    return written


def main(argv=None):
    parser = argparse.ArgumentParser(prog="pe_utils", description="Insert length distribution of paired-end reads.")
    parser.add_argument("--compute-insert-len", dest="compute_insert_len", nargs=2, metavar=("BAMS", "GFF"),
                        default=None,
                        help="Compute the insert length of the comma-separated BAM/SAM files BAMS from the read pairs "
                             "inside one interval of GFF (usually constitutive exons: exon_utils --get-const-exons).")
    parser.add_argument("--output-dir", dest="output_dir", default=None, help="Output directory.")
    parser.add_argument("--sd-max", dest="sd_max", type=float, default=2,
                        help="Drop insert lengths more than this many standard deviations from the mean. Default 2.")
    parser.add_argument("--no-bam-filter", dest="no_bam_filter", action="store_true", default=False,
                        help="Do not drop reads that failed QC, are unmapped, have an unmapped mate or are not "
                             "flagged paired before pairing.")
    parser.add_argument("--min-exon-size", dest="min_exon_size", type=int, default=500,
                        help="Accepted for compatibility and has NO effect: every record of the GFF is used as an "
                             "interval, whatever its size (filter the exons with exon_utils --min-exon-size).")
    parser.add_argument("--device", dest="device", type=int, default=0, help="HIP device. Default 0.")
    options = parser.parse_args(argv)
    if options.compute_insert_len is None or options.output_dir is None:
        parser.print_help(sys.stderr)
        return 1
    bams = [os.path.abspath(os.path.expanduser(b)) for b in options.compute_insert_len[0].split(",") if b]
    gff_filename = os.path.abspath(os.path.expanduser(options.compute_insert_len[1]))
    try:
        compute_insert_len(bams, gff_filename, os.path.abspath(os.path.expanduser(options.output_dir)),
                           min_exon_size=options.min_exon_size, no_bam_filter=options.no_bam_filter,
                           sd_max=options.sd_max, device=options.device)
    except (InsertLenError, IOError) as err:
        sys.stderr.write("Error: %s\n" % err)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
