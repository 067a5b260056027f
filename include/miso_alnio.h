/*
 * miso_alnio.h -- C ABI of the alignment reader: the step
 * immediately before the sampler.  Part of libmiso_amd.so.
 *
 * What it replaces in the reference (all through the third-party `pysam` module, which is not
 * under /root/reference and not installed here):
 *   misopy/sam_utils.py:139-150   load_bam_reads            pysam.Samfile(bam, "rb")
 *   misopy/sam_utils.py:153-186   fetch_bam_reads_in_gene   bamfile.fetch(chrom, start, end)
 *   misopy/sam_utils.py:207-300   pair_sam_reads            mate pairing by read name
 *   misopy/sam_utils.py:303-442   sam_parse_reads           strand / read-length filters,
 *                                                           (positions, CIGAR strings) tuples
 * The reference walks a Python object per read; a GPU batch needs the reads of tens of thousands
 * of events, so here the file is decoded ONCE (BGZF blocks inflated in parallel, or SAM text
 * parsed) into columns, indexed by (reference, position), and an event's reads come out of
 * miso_aln_parse_reads as flat arrays that go straight into miso_batch_add_event.
 *
 * Formats: BAM (BGZF, SAM spec v1 section 4) and SAM text; no .bai needed (the index is built in
 * memory while loading).  Coordinates follow pysam: `pos` 0-based, fetch regions 0-based
 * half-open, a record overlaps a region when pos < end && end_pos > start, end_pos = pos +
 * (reference bases consumed by M/D/N/=/X) or pos + 1 for unmapped / CIGAR-less records (htslib
 * bam_endpos).
 *
 * Errors: functions return 0 on success or a MISO_* code of miso_amd.h (MISO_EINVAL for bad
 * arguments / malformed files, MISO_ENOMEM, MISO_FAILURE for I/O); miso_aln_last_error() has the
 * text.  Not thread-safe per handle for open/close; fetch/parse are read-only and re-entrant.
 */
#ifndef MISO_ALNIO_H
#define MISO_ALNIO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct miso_alnfile miso_alnfile_t;

/* strand_rule values (misopy/sam_utils.py:320-360; settings key `strand`) */
#define MISO_STRAND_UNSTRANDED  0   /* "fr-unstranded" or no rule: nothing is discarded          */
#define MISO_STRAND_FIRSTSTRAND 1   /* "fr-firststrand"                                            */
/* "fr-secondstrand" is an exception in the reference (sam_utils.py:331): callers raise, no code */

/* Columns of the decoded file, one entry per record in file order (borrowed pointers, valid until
 * miso_aln_close).  cigar[cigar_off[i] .. cigar_off[i+1]) are BAM-encoded ops: len << 4 | op with
 * op indexing "MIDNSHP=X".  names[name_off[i] .. name_off[i+1]) is the read name (no NUL). */
typedef struct {
  int64_t n;
  const int32_t *ref_id;     /* -1 = no reference ("*")                                         */
  const int32_t *pos;        /* 0-based leftmost coordinate (pysam read.pos)                      */
  const int32_t *end;        /* htslib bam_endpos                                                 */
  const int32_t *flag;       /* SAM FLAG                                                          */
  const int32_t *l_seq;      /* query length (pysam read.rlen)                                    */
  const uint64_t *cigar_off; /* n + 1                                                             */
  const uint32_t *cigar;
  const uint64_t *name_off;  /* n + 1                                                             */
  const char *names;
} miso_aln_columns_t;

/* Open and decode a BAM or SAM file (detected by content).  n_threads <= 0: all usable cores. */
int miso_aln_open(const char *path, int n_threads, miso_alnfile_t **out);
void miso_aln_close(miso_alnfile_t *f);

int miso_aln_columns(const miso_alnfile_t *f, miso_aln_columns_t *cols);
int miso_aln_n_refs(const miso_alnfile_t *f);
const char *miso_aln_ref_name(const miso_alnfile_t *f, int ref);     /* NULL if out of range    */
int64_t miso_aln_ref_length(const miso_alnfile_t *f, int ref);
int miso_aln_ref_id(const miso_alnfile_t *f, const char *name);      /* -1 if absent            */
int miso_aln_is_bam(const miso_alnfile_t *f);

/* bamfile.fetch(chrom, start, end): indices (into the columns) of the records overlapping
 * [start, end) on reference `ref`, ordered by (pos, file order).  Two-call pattern: *n receives
 * the number of hits; at most `cap` indices are written to idx (idx may be NULL when cap == 0). */
int miso_aln_fetch(const miso_alnfile_t *f, int ref, int64_t start, int64_t end,
                   int64_t *idx, int64_t cap, int64_t *n);

/* fetch + sam_parse_reads in one call: the (positions, CIGAR strings) of one event.
 *   paired        0: single-end (sam_utils.py:417-436); 1: mates paired by name
 *                 (pair_sam_reads, sam_utils.py:207-300), two consecutive entries per pair
 *   strand_rule   MISO_STRAND_*; target_strand '+', '-', 0 = no target strand: no strand check
 *                 (sam_utils.py:385-390; the fr-firststrand mate swap of pair_sam_reads still
 *                 applies), any other character: single-end compares it with the read's strand,
 *                 paired fr-firststrand matches nothing, as the reference's function falls
 *                 through to None (sam_utils.py:337-346)
 *   given_read_len  > 0: drop reads (pairs) whose query length differs (sam_utils.py:399-404,
 *                 423-426); <= 0: no filter
 * Outputs (two-call pattern like miso_aln_fetch): *n_reads = number of reads (pairs) kept --
 * the reference's num_raw_reads; positions (0-based, 1 or 2 per read); the CIGAR strings
 * concatenated, NUL-terminated each, into cigar_buf (needed size in *cigar_bytes).
 * *n_strand_discarded (may be NULL) counts reads dropped by the strand rule. */
int miso_aln_parse_reads(const miso_alnfile_t *f, int ref, int64_t start, int64_t end, int paired,
                         int strand_rule, int target_strand, int given_read_len,
                         int32_t *positions, int64_t pos_cap, char *cigar_buf, int64_t cigar_cap,
                         int64_t *n_reads, int64_t *cigar_bytes, int64_t *n_strand_discarded);

/* One event straight from the file into a sampler batch (miso_amd.h): miso_aln_parse_reads with the
 * batch's single-end / paired-end mode, positions made 1-based (misopy/miso_sampler.py:284), then
 * miso_batch_add_event -- no per-read work in the host language.  *n_reads = reads (pairs) found;
 * the event is added only when 0 < *n_reads and *n_reads >= min_reads (run_miso.py:139-147), else
 * *event_index = -1 and the call still succeeds.  Errors as miso_batch_add_event (bad CIGAR, ...). */
struct miso_batch;
struct miso_gene;
int miso_batch_add_event_aln(struct miso_batch *batch, const struct miso_gene *gene,
                             const miso_alnfile_t *f, int ref, int64_t start, int64_t end,
                             int strand_rule, int target_strand, int given_read_len, int64_t min_reads,
                             const double *hyperp, int n_hyperp, int64_t *n_reads, int *event_index);

/* The same for n events at once, reads collected and CIGARs parsed on n_threads host threads (<= 0:
 * all usable cores), events appended in the order given; default hyperparameters.  n_reads[i] and
 * event_index[i] as above.  On an error (bad CIGAR, ...) nothing is added and the first failing event's
 * error is reported. */
int miso_batch_add_events_aln(struct miso_batch *batch, int n, const struct miso_gene *const *genes,
                              const miso_alnfile_t *f, const int *ref, const int64_t *start,
                              const int64_t *end, int strand_rule, const int *target_strand,
                              int given_read_len, int64_t min_reads, int n_threads, int64_t *n_reads,
                              int *event_index);

/* ---- the fragment length distribution of a paired-end file (misopy/pe_utils.py:148-302) ----
 * Intervals: n_intervals records of a GFF, GFF coordinates (1-based, inclusive): seqid[i], start[i], end[i].  A record
 * is tagged by interval i when it is mapped (not 0x4, ref_id >= 0), its reference is named seqid[i] and its whole span
 * lies inside: start[i] - 1 <= pos && end <= end[i] (pos 0-based, end = bam_endpos, spliced span included).  Strand
 * is not considered.  filter_reads != 0: records with 0x200, 0x4 or 0x8, or without 0x1, do not pair
 * (sam_utils.py:225-230).  chunk_records: records per device chunk (<= 0: the default, 4 M); device memory is bounded by
 * it, whatever the file's size.  Both calls fail with MISO_ENODEVICE without a GPU: there is no CPU path. */

/* One code per record (miso_insert_tag_records): bits 0-28 the tag, bit 29 the CIGAR is exactly one M op, bit 30 the
 * record passes the read filter (always set when filter_reads == 0). */
#define MISO_INSERT_TAG_MASK   0x1FFFFFFF
#define MISO_INSERT_TAG_NONE   0x1FFFFFFF  /* no interval contains the record                      */
#define MISO_INSERT_TAG_MULTI  0x1FFFFFFE  /* two or more do; any other tag value: the interval's index */
#define MISO_INSERT_ONE_M      (1 << 29)
#define MISO_INSERT_FILTER_OK  (1 << 30)

typedef struct {
  int64_t kept;          /* pairs with an insert length > 0                                         */
  int64_t skipped;       /* pairs failing pe_utils.py:170-189 (one tag each, the same one, one M op) */
  int64_t unpaired;      /* names whose tagged, filtered records are not exactly two                 */
  int64_t same_strand;   /* pairs whose mates have equal 0x10                                        */
  int64_t nonpositive;   /* pairs with an insert length <= 0 (dropped with a warning by the reference) */
  int64_t tagged;        /* records that join the pairing (tagged and past the filter)              */
  int64_t chunks;        /* device chunks of the record pass                                         */
  double records_ms, grouping_ms, pairs_ms;   /* wall time of the three stages                     */
} miso_insert_stats_t;

/* The record pass alone: codes[n] (n = the file's record count) as above. */
int miso_insert_tag_records(const miso_alnfile_t *f, int device, int filter_reads, int n_intervals,
                            const char *const *seqid, const int64_t *start, const int64_t *end,
                            int64_t chunk_records, int32_t *codes);

/* The whole computation up to the insert lengths: tag, pair by name (strip_mate_id; groups of exactly two, the left
 * mate the one first in the file, mates on opposite strands), then insert = right.pos + len(right's M) - left.pos for
 * the pairs whose mates carry exactly one tag each, the same one, and a CIGAR of exactly one M op.  Out: the kept pairs
 * as (interval index, insert) ordered by interval index, then by the left mate's position in the file.  Two-call
 * pattern: *n_kept = number of kept pairs, at most `cap` written (arrays may be NULL when cap == 0); a caller that
 * wants one pass gives cap = records / 2, which no file can exceed.  stats may be NULL. */
int miso_insert_len(const miso_alnfile_t *f, int device, int filter_reads, int n_intervals,
                    const char *const *seqid, const int64_t *start, const int64_t *end, int64_t chunk_records,
                    int32_t *interval_out, int32_t *insert_out, int64_t cap, int64_t *n_kept,
                    miso_insert_stats_t *stats);

/* ---- per-interval read coverage (`miso --run --prefilter`, misopy/exon_utils.py:198-250) ----
 * Intervals as for miso_insert_len (GFF coordinates, seqid[i] named exactly as the file names it; a seqid the file
 * does not name, or start[i] > end[i], counts 0).  A record is kept when it is mapped (not 0x4, ref_id >= 0) and some
 * interval on its reference holds its whole span (start - 1 <= pos && bam_endpos <= end; bedtools intersect -f 1); no
 * other flag matters.  counts[i] = the kept records on interval i's reference with pos < end[i] and
 * bam_endpos > start[i] - 1 (bedtools coverage -counts).  chunk_records: records per device chunk (<= 0: the default,
 * 4 M); device memory is bounded by it and by n_intervals.  The counts do not depend on it or on the record order.
 * Fails with MISO_ENODEVICE without a GPU: there is no CPU path.  stats may be NULL. */
typedef struct {
  int64_t kept;          /* records held whole by some interval                                             */
  int64_t chunks;        /* device chunks of the record pass                                                */
  double records_ms;     /* record pass: copies of the columns to the device and the kernel (device time)   */
  double sort_ms;        /* the host tables: intervals sorted per reference, the sorted rank keys           */
  double rank_ms;        /* rank step: prefix sums of the rank histograms and the per-interval differences  */
  double total_ms;       /* wall time of the whole call                                                     */
} miso_region_stats_t;

int miso_region_counts(const miso_alnfile_t *f, int device, int n_intervals, const char *const *seqid,
                       const int64_t *start, const int64_t *end, int64_t chunk_records, int64_t *counts,
                       miso_region_stats_t *stats);

/* ---- fetch counts of many intervals (`sam_rpkm --compute-rpkm`, misopy/sam_rpkm.py:138-154) ----
 * counts[i] = the number miso_aln_fetch(f, miso_aln_ref_id(f, seqid[i]), start[i], end[i], NULL, 0, &n) puts in n: the
 * records whose reference is named exactly seqid[i] with pos < end[i] && bam_endpos > start[i] (pos 0-based, bam_endpos
 * as above).  No flag matters; a record without a reference counts nowhere.  The numbers are used as given, as
 * bamfile.fetch(chrom, exon.start, exon.end) uses them in the reference: a caller that hands over GFF numbers (1-based,
 * inclusive) puts them in pysam's 0-based half-open slot, the mix miso_region_densities documents below.  A seqid the
 * file does not name, or start[i] > end[i], counts 0; intervals may nest, overlap and repeat.  One pass over the record
 * columns on the device, whatever n_intervals is.  chunk_records: records per device chunk (<= 0: the default, 4 M);
 * device memory is bounded by it and by n_intervals.  The counts do not depend on it or on the record order.  Fails
 * with MISO_ENODEVICE without a GPU: there is no CPU path.  stats may be NULL; its fields as for miso_region_counts,
 * `kept` = the records of the file (nothing is filtered). */
int miso_fetch_counts(const miso_alnfile_t *f, int device, int n_intervals, const char *const *seqid,
                      const int64_t *start, const int64_t *end, int64_t chunk_records, int64_t *counts,
                      miso_region_stats_t *stats);

/* ---- per-base read density and junction counts of many regions (sashimi_plot, misopy/sashimi_plot/plot_utils/
 * plot_gene.py:48-57, 398-444 readsToWiggle_pysam) ----
 * Regions: n_regions triples (seqid[i], tx_start[i], tx_end[i]) in the numbers a GFF gives (1-based, inclusive); seqid[i]
 * is matched exactly against the file's reference names.  Record coordinates: pos 0-based, bam_endpos as above.  The
 * reference mixes the two systems and so does this call:
 *   1. a record is fetched for a region when it is on its reference and pos < tx_end && bam_endpos > tx_start; no flag
 *      matters;
 *   2. a fetched record without a CIGAR, or with more than one N op, adds nothing; I and D do not disqualify;
 *   3. its aligned positions are the reference positions of its M, =, X ops (D and N advance the reference; I, S, H, P do
 *      not); qlen = the sum of its M, I, =, X lengths; a record without aligned positions adds nothing;
 *   4. depth[x - tx_start] counts the records with an aligned position x, tx_start <= x <= tx_end; every such position
 *      weighs 1 / qlen in wiggle;
 *   5. two consecutive aligned positions x, y of one record with y > x + 1 (an N or a D between them) and
 *      tx_start <= x <= tx_end give leftss = x + 1, rightss = y + 1; when tx_start < leftss < tx_end and
 *      tx_start < rightss < tx_end the junction (leftss, rightss) of that region counts one more;
 *   6. a region whose seqid the file does not name, or with tx_start > tx_end: all zero, no junction, no error;
 *   7. regions may overlap, nest and repeat: each is computed as if alone.
 * Out: region i owns L_i = max(0, tx_end[i] - tx_start[i] + 1) consecutive entries of depth and wiggle, the regions one
 * after the other in the order given (out_cap = entries the two arrays hold, at least the sum of the L_i).
 * wiggle[b] = the sum over the distinct qlen values q, ascending, of depth_q[b] / q in double, depth_q the depth from
 * records of that qlen: exact integer counts first, so the value does not depend on the record order, the chunk size or
 * the grouping (the reference adds 1. / qlen into a float32 array in file order).  Junctions: (region, leftss, rightss,
 * count) sorted by region, leftss, rightss; two-call pattern: *n_jxn = their number, at most jxn_cap written (arrays may
 * be NULL when jxn_cap == 0).
 * chunk_records: records per device chunk (<= 0: 4 M).  accum_bytes: device bytes for the accumulators of one group of
 * regions (<= 0: 1 GiB); the regions are processed in groups that fit (a region larger than the budget is a group of its
 * own), one pass over the records per group.  qlen up to 65535; a fetched record beyond fails with MISO_EINVAL and names
 * it.  Fails with MISO_ENODEVICE without a GPU: there is no CPU path.  stats may be NULL. */
typedef struct {
  int64_t fetched;           /* records fetched by at least one region                                            */
  int64_t skipped_multi_n;   /* of those: more than one N op                                                     */
  int64_t skipped_no_cigar;  /* of those: no CIGAR                                                               */
  int64_t with_indel;        /* of those, not skipped: an I or a D op                                            */
  int64_t qlen_classes;      /* distinct qlen among the fetched, not skipped records with an aligned position     */
  int64_t chunks;            /* device chunks of one pass over the records                                       */
  int64_t groups;            /* region groups = passes over the records after the mark pass                      */
  int64_t junction_retries;  /* group passes repeated because the junction list had to grow                      */
  double tables_ms;          /* host tables: all regions, then each group's                                      */
  double mark_ms;            /* mark pass: copies of the columns and the kernel (device time)                    */
  double records_ms;         /* group passes: copies of the columns and the kernel (device time)                 */
  double scan_ms;            /* scan and finish kernels (device time)                                            */
  double junction_ms;        /* junction keys back, sorted and counted on the host                               */
  double copy_ms;            /* depth and wiggle back and into the caller's arrays                               */
  double total_ms;           /* wall time of the whole call                                                      */
} miso_density_stats_t;

int miso_region_densities(const miso_alnfile_t *f, int device, int n_regions, const char *const *seqid,
                          const int64_t *tx_start, const int64_t *tx_end, int64_t chunk_records, int64_t accum_bytes,
                          int32_t *depth, double *wiggle, int64_t out_cap, int32_t *jxn_region, int64_t *jxn_left,
                          int64_t *jxn_right, int64_t *jxn_count, int64_t jxn_cap, int64_t *n_jxn,
                          miso_density_stats_t *stats);

/* host threads the library uses by default: affinity mask capped by the cgroup CPU quota, <= 64 */
int miso_usable_threads(void);

const char *miso_aln_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
