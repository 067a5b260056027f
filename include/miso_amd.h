/*
 * miso_amd.h -- C ABI of libmiso_amd.so: the MI355X-native MISO posterior sampler.
 *
 * This is the drop-in boundary for the one hot path of yarden/MISO: what the reference's
 * CPython glue (pysplicing/src/pysplicing.c) binds in the C core for `createGene`, `MISO` and
 * `MISOPaired`.  Plain pointers and sizes only; no Python, no torch, no HIP types.
 *
 *   reference symbol (file:line under /root/reference/pysplicing)   replaced by
 *   ------------------------------------------------------------   ------------------------
 *   splicing_create_gene        src/simulator.c:9                   miso_create_gene
 *   splicing_gff_destroy2       src/gff.c:80                        miso_gene_destroy
 *   splicing_gff_noiso_one      src/gff.c:684                       miso_gene_noiso
 *   splicing_gff_isolength_one  src/gff.c:689                       miso_gene_isolength
 *   splicing_miso               src/miso.c:638   (include/splicing.h:203)  miso_run
 *   splicing_miso_paired        src/miso_paired.c:241 (splicing.h:216)     miso_run_paired
 *   splicing_matchIso           src/solve.c:8                       miso_match_iso
 *   splicing_matchIso_paired    src/solve.c:141                     miso_match_iso_paired
 *   splicing_strerror           src/error.c:71                      miso_strerror
 *   splicing_error handler hook src/pyerror.c:27-44                 miso_last_error
 *
 * The reference runs ONE event per call on one CPU core.  A GPU needs thousands of events in
 * flight, so besides the per-event calls (a batch of one) the library exports a batch object:
 * add events, upload once, launch, read results per event.  Events are independent
 * (SURVEY.md section 8e): sharding a run over GPUs is a static split of the event list, each
 * shard a batch on its own device; results do not depend on the split because every random
 * draw is addressed by (seed, global event id, chain, iteration) -- include/miso_philox.h.
 *
 * Matrices are column-major as in the reference (include/splicing_matrix.h:67):
 * samples[K x S] stores sample s at samples[s*K .. s*K+K-1]; class_templates[K x ncls] likewise.
 * Error codes are the reference's (include/splicing_error.h:314-351).
 *
 * There is NO CPU fallback: every sampler entry point fails with MISO_ENODEVICE when no HIP
 * device is usable.
 */
#ifndef MISO_AMD_H
#define MISO_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes (splicing_error.h:314-351) ---- */
#define MISO_SUCCESS 0
#define MISO_FAILURE 1
#define MISO_ENOMEM 2
#define MISO_EINVAL 4
#define MISO_UNIMPLEMENTED 12
#define MISO_EINTERNAL 38
#define MISO_ENODEVICE 60 /* new: no usable HIP device / HIP runtime error */

/* ---- enums (splicing.h:59-62, 148-158; pysplicing/__init__.py:2-13) ---- */
#define MISO_ALGO_REASSIGN 0
#define MISO_ALGO_MARGINAL 1
#define MISO_ALGO_CLASSES 2
#define MISO_START_AUTO 0
#define MISO_START_UNIFORM 1
#define MISO_START_RANDOM 2
#define MISO_START_GIVEN 3
#define MISO_START_LINEAR 4
#define MISO_STOP_FIXEDNO 0
#define MISO_STOP_CONVERGENT_MEAN 1

/* Most isoforms of one gene.  The reference has no limit (miso.c:696, gff.c:684); here an isoform is a bit of a read's
   compatibility mask ((K + 31) / 32 words per read) and an entry of the chain's vectors; from 65 isoforms on the chain's
   vectors live in LDS (sampler_big) and a read's pick is returned as one byte: 256.  A gene with more is reported
   MISO_UNIMPLEMENTED by the one-event calls and skipped with a message by the batch callers. */
#define MISO_MAX_ISOFORMS 256

/* splicing_miso_rundata_t (splicing.h:143-146), same field order */
typedef struct miso_rundata {
  int noIso, noIters, maxIters, noBurnIn, noLag, noAccepted, noRejected, noChains, noSamples;
} miso_rundata_t;

typedef struct miso_gene miso_gene_t;   /* one gene = the reference's splicing_gff_t handle */
typedef struct miso_batch miso_batch_t;

/* ---- errors ---- */
const char *miso_strerror(int code);
/* "Error at <file>:<line>: <reason>, <strerror>" of the calling thread's last failure
   (the text pyerror.c:27-44 turns into the Python exception). */
const char *miso_last_error(void);

/* ---- device ---- */
int miso_device_count(int *count);
int miso_set_device(int device);

/* ---- gene model ---- */
/* exons: 2*n_exons ints (start,end; 1-based inclusive). isoforms: exon indices, each isoform
   terminated by -1 (the flattening pyconvert.c:55-87 produces). strand: 0 +, 1 -, 2 unknown. */
int miso_create_gene(const int *exons, int n_exons, const int *isoforms, int n_isoforms_flat,
                     const char *id, const char *seqid, const char *source, int strand,
                     miso_gene_t **gene);
void miso_gene_destroy(miso_gene_t *gene);
int miso_gene_noiso(const miso_gene_t *gene, int *noiso);
int miso_gene_isolength(const miso_gene_t *gene, int *isolength /* noiso */);

/* The gene's possible read classes (splicing_assignment_matrix, assignment.c:90-276; the module's assignmentMatrix,
   pysplicing.c:324-349): one column per distinct set of isoforms that share an alignment of a readLength-base read at some
   start position, its entries that number of positions for the set's isoforms and 0 for the others; columns ordered as the
   reference orders them.  matrix: noiso x max_cols doubles, column-major; *n_cols = columns (MISO_EINVAL if more than
   max_cols).  overHang > 1: MISO_UNIMPLEMENTED, as in the reference.  What algorithm = MISO_ALGO_CLASSES sums over. */
int miso_gene_assignment_matrix(const miso_gene_t *gene, int readLength, int overHang, double *matrix, int max_cols,
                                int *n_cols);

/* ---- problem construction on the host (input builder of the path) ---- */
/* match: noiso x n_reads, 1.0 / 0.0 */
int miso_match_iso(const miso_gene_t *gene, const int *position, const char *const *cigarstr,
                   int n_reads, int overHang, int readLength, double *match);
/* position/cigarstr hold 2*n_pairs mates (consecutive). match: noiso x n_pairs fragment
   probabilities (0 = incompatible); fragmentLength: noiso x n_pairs (-1 = none), may be NULL */
int miso_match_iso_paired(const miso_gene_t *gene, const int *position,
                          const char *const *cigarstr, int n_positions, int readLength,
                          int overHang, double normalMean, double normalVar, double numDevs,
                          double *match, int *fragmentLength);

/* ---- one event per call: splicing_miso / splicing_miso_paired ---- */
/* Output sizes: samples noiso*S, logLik S with S = noChains*(noIterations-noBurnIn)/noLag;
   class_templates noiso*n_reads (worst case), class_counts n_reads, assignment n_reads.
   Any output pointer may be NULL.  seed: the one addition to the reference signature. */
int miso_run(const miso_gene_t *gene, const int *position, const char *const *cigarstr,
             int n_reads, int readLength, int overHang, int noChains, int noIterations,
             int maxIterations, int noBurnIn, int noLag, const double *hyperp, int n_hyperp,
             int algorithm, int start, int stop, uint64_t seed, double *samples, double *logLik,
             double *class_templates, double *class_counts, int *n_classes, int *assignment,
             miso_rundata_t *rundata);

int miso_run_paired(const miso_gene_t *gene, const int *position, const char *const *cigarstr,
                    int n_positions, int readLength, int overHang, int noChains,
                    int noIterations, int maxIterations, int noBurnIn, int noLag,
                    const double *hyperp, int n_hyperp, int start, int stop, double normalMean,
                    double normalVar, double numDevs, uint64_t seed, double *samples,
                    double *logLik, double *bin_class_templates, double *bin_class_counts,
                    int *n_classes, int *assignment, miso_rundata_t *rundata);

/* ---- many events per launch ---- */
typedef struct miso_params {
  int paired;                /* 0 single-end (splicing_miso), 1 paired-end (splicing_miso_paired) */
  int readLength, overHang;
  int noChains, noIterations, maxIterations, noBurnIn, noLag;
  int algorithm, start, stop;
  double normalMean, normalVar, numDevs; /* paired only */
  int want_counts_trace;     /* tests: keep the per-iteration assignment counts of every chain */
  int device_match;          /* 1: miso_batch_add_event only parses the CIGAR strings; the
                                compatibility of every read with every isoform (solve.c:8-108,
                                141-218) is computed by one GPU kernel for the whole batch at
                                miso_batch_upload.  Read classes (miso_batch_event_info's
                                n_classes, class templates) are then available after the upload.
                                0: on the host, at miso_batch_add_event */
} miso_params_t;

/* Paired-end: the fragment-length distribution (the lengths max(readLength, normalMean - numDevs * sd) ..
   normalMean + numDevs * sd, sd = sqrt(normalVar), both truncated to integers) may hold at most 65535 lengths: a
   pair's fragment length is kept as a 16-bit index into it and 0xFFFF stands for "none".  A wider one is
   MISO_UNIMPLEMENTED. */
int miso_batch_create(const miso_params_t *params, miso_batch_t **batch);
void miso_batch_destroy(miso_batch_t *batch);

/* Adds one event built from alignments; hyperp NULL = all ones. *event_index = position in
   the batch (also its offset from first_event_id in the RNG address). */
int miso_batch_add_event(miso_batch_t *batch, const miso_gene_t *gene, const int *position,
                         const char *const *cigarstr, int n_positions, const double *hyperp,
                         int n_hyperp, int *event_index);

/* Adds one event from an already built problem: match noiso x n_reads as miso_match_iso[_paired]
   returns it (+ fragmentLength for paired), isoform lengths and exon counts (gff.c:583-657). */
int miso_batch_add_problem(miso_batch_t *batch, int noiso, int n_reads, const double *match,
                           const int *fragmentLength, const int *isolength, const int *noexons,
                           const double *hyperp, int *event_index);

/* Synthetic reads for one gene (the module's simulateReads / simulatePairedReads,
   pysplicing.c:280-330 -> simulator.c:68, 221): n_reads single-end reads, or n_reads PAIRS when
   normalVar > 0.  position: n (2n paired) ints; cigar: n (2n) slots of cigar_stride bytes;
   isoform (may be NULL): true isoform of every read.  Deterministic in sim_seed. */
int miso_simulate_reads(const miso_gene_t *gene, const double *expression, int n_reads,
                        int readLength, double normalMean, double normalVar, double numDevs,
                        uint64_t sim_seed, int *isoform, int *position, char *cigar,
                        int cigar_stride);

/* miso_simulate_reads + miso_batch_add_event in one call (the batch's readLength / paired /
   fragment parameters apply): bulk synthetic workloads without string traffic over the ABI. */
int miso_batch_add_simulated(miso_batch_t *batch, const miso_gene_t *gene,
                             const double *expression, int n_reads, uint64_t sim_seed,
                             const double *hyperp, int n_hyperp, int *event_index);

int miso_batch_size(const miso_batch_t *batch, int *n_events);

/* pack + copy to HBM (idempotent) */
/* The random stream of an event is addressed by (seed, event id): by default first_event_id (a launch
 * argument) + the event's index in the batch.  A caller that drops events between numbering and
 * batching (skip rules) pins the id here instead, so results do not depend on batch composition,
 * chunk size or the number of GPUs.  Before miso_batch_upload. */
int miso_batch_set_event_id(miso_batch_t *batch, int event_index, uint32_t event_id);
/* Single-end batches: on != 0 selects the COLLAPSED Gibbs step for the two-isoform events (csrc/kernels_lane.hip).
   The reference reassigns every read by itself (miso.c:30-91 inside miso.c:493-552) and then uses the per-isoform
   counts only (miso.c:243-307); reads compatible with the same isoforms are exchangeable, so their counts are drawn
   directly -- Binomial(n, psi_0 / (psi_0 + psi_1)) from the counter RNG, include/miso_binomial.h -- which is the same
   Markov chain on (psi, counts) at O(1) instead of O(reads) per iteration.  The run's last reassignment is made per
   read, so the returned assignment is a per-read draw.  Different draws than the default mode (same distribution):
   checked bit for bit against the checker's collapsed mode and statistically against the reference.  Events with
   more than two isoforms of such a batch run as always -- unless on == 2: then they draw, per compatibility class, a
   chain of binomials (sampler_lane_k; same contract, same checker).  That pays from ~10^4 reads per event only: with
   ~1000 reads spread over the classes of a five- or ten-isoform event it is slower than the per-read sweep
   (profiles/r03_collapsed.txt).  Before miso_batch_launch; MISO_EINVAL for paired-end. */
int miso_batch_set_collapsed(miso_batch_t *batch, int on);
/* Single-end batches, algorithm = MISO_ALGO_REASSIGN: on != 0 selects the EXACT-POSTERIOR mode for the eligible
   two-isoform events (csrc/kernels_exact.hip).  With x = psi_0 the reference's joint score summed
   over the reads' assignments is a density of one variable,
       log p(x) = (n10 + h0 - 1) log x + (n01 + h1 - 1) log(1 - x) - n log(x e0 + (1 - x) e1) + const
   (n10 / n01 reads compatible with isoform 0 / 1 only, n all reads with a compatible isoform, e the effective lengths,
   h the Dirichlet hyperparameters).  An eligible event -- two isoforms, both hyperparameters in [1, 2^20], both effective
   lengths in [2^-40, 2^40] and within a factor 2^20 of each other (the fence of DESIGN.md section 15: inside it the scheme
   keeps its stated accuracy at any counts; an infinity or a NaN is outside; miso_exact_eligible) -- runs no chain: the
   density is tabulated once on a grid in logit space
   and the event's noSamples rows are INDEPENDENT draws from it, row s by inverting the CDF at the uniform of
   (seed, event id, sample s, MISO_SITE_EXACT).  What such an event returns: samples as ever (row order = sample
   index); logLik[s] = the MARGINAL score log p at the sample with the Dirichlet normaliser, not a joint score with an
   assignment; assignment = one per-read reassignment from the last sample's psi, drawn as algorithm = MARGINAL draws
   its one (Gibbs words of chain 0, MISO_ITER_INIT); rundata accepted = noSamples, rejected = 0; under stop =
   CONVERGENT_MEAN it is done after the first round.  Every other event of the batch runs through the sampler kernels,
   bit-identical to the same event in a batch without the mode.  May be combined with miso_batch_set_collapsed: exact
   takes the eligible events, collapsed the rest it would have taken.  Before miso_batch_launch; MISO_EINVAL for
   paired-end batches and for algorithm != MISO_ALGO_REASSIGN. */
int miso_batch_set_exact(miso_batch_t *batch, int on);
/* the eligibility rule on its own (host arithmetic, no device): eff_len / hyper: noiso doubles each.  Every entry point that
   takes raw statistics (the miso_selftest_exact* calls, the exact comparisons) answers an element outside it with
   MISO_EINVAL; a batch in the mode leaves such an event to the sampler; the replicate-group calls report was_exact = 0. */
int miso_exact_eligible(int paired, int noiso, const double *eff_len, const double *hyper, int *eligible);
/* After miso_batch_sync: posterior mean and the quantiles (1 - confidence_level) / 2 and 1 - (1 - confidence_level) / 2
   of an event the exact mode took, from the grid itself: no Monte-Carlo error.  mean / ci_low / ci_high: two doubles
   each (isoform 0, isoform 1; isoform 1's from 1 - x computed on its own, so a value near 0 keeps its relative
   precision).  *was_exact = 0 and the outputs untouched for an event that ran the sampler. */
int miso_batch_get_exact_summary(miso_batch_t *batch, int event_index, double *mean, double *ci_low, double *ci_high,
                                 double confidence_level, int *was_exact);
/* Paired-end batches, algorithm = MISO_ALGO_REASSIGN: on != 0 selects the exact-posterior mode of the eligible
   PAIRED-END two-isoform events (csrc/kernels_exact_paired.hip); a switch of its own, apart from
   miso_batch_set_exact.  Summed over the pairs' assignments the law of x = psi_0 under the reference's paired chain
   (miso_paired.c:24-174) is
       log p(x) = (n10 + h0 - 1) log x + (n01 + h1 - 1) log(1 - x) + sum_i log(x m0_i + (1 - x) m1_i)
                  - n log(x A0 + (1 - x) A1) + const
   (n10 / n01 pairs compatible with isoform 0 / 1 only; the sum over the pairs compatible with both, m their
   fragment-length probabilities under the two isoforms; n all pairs with a compatible isoform; A_k = exp(assscores_k),
   miso_paired.c:403-419).  An eligible event -- two isoforms, both hyperparameters in [1, 2^20], A0 and A1 in
   [2^-40, 2^40] and within a factor 2^20 of each other (the single-end mode's fence), no pair on a non-finite score
   entry (miso_exact_paired_eligible) -- runs no chain: one wavefront tabulates the density (which may
   have SEVERAL modes) and row s of the samples inverts the CDF at the uniform of (seed, event id, sample s,
   MISO_SITE_EXACT).  logLik[s] = log p at the sample with the Dirichlet normaliser and without psi-free constants: the
   MARGINAL log density, not the reference's joint score -- the additive terms of quirk C5 are absent by construction;
   assignment = one reassignment of the pairs from the last row's psi by the paired pick rule
   U (psi0 m0 + psi1 m1) < psi0 m0, on the words of the paired sampler's initial reassignment of chain 0 (MISO_SITE_GIBBS,
   MISO_ITER_INIT); accepted = noSamples, rejected = 0; done after round one under stop = CONVERGENT_MEAN;
   miso_batch_get_exact_summary serves these events too.  Every other event runs through the sampler kernels,
   bit-identical to the same event in a batch without the mode.  Before miso_batch_launch; MISO_EINVAL for single-end
   batches and for algorithm != MISO_ALGO_REASSIGN. */
int miso_batch_set_exact_paired(miso_batch_t *batch, int on);
/* the eligibility rule on its own (host arithmetic): A = exp(assscores), hyper: noiso doubles each; any_bad != 0: a pair
   of the event touches a non-finite score entry */
int miso_exact_paired_eligible(int noiso, const double *A, const double *hyper, int any_bad, int *eligible);
int miso_batch_upload(miso_batch_t *batch, int device);
/* enqueue the sampler kernels for every event on the batch's stream; returns immediately */
int miso_batch_launch(miso_batch_t *batch, uint64_t seed, uint32_t first_event_id);
/* wait for the stream; *kernel_ms (may be NULL) = HIP-event time of the launches */
int miso_batch_sync(miso_batch_t *batch, float *kernel_ms);
/* copy results back to the host (after sync) */
int miso_batch_download(miso_batch_t *batch);
/* upload + launch + sync + download */
int miso_batch_run(miso_batch_t *batch, int device, uint64_t seed, uint32_t first_event_id);

int miso_batch_event_info(const miso_batch_t *batch, int event_index, int *noiso, int *n_reads,
                          int *n_samples, int *n_classes);
int miso_batch_get_result(const miso_batch_t *batch, int event_index, double *samples,
                          double *logLik, double *class_templates, double *class_counts,
                          int *assignment, miso_rundata_t *rundata);

/* The `.miso` files of many events at once (misopy/miso_sampler.py:444-464, output_miso_results):
 * for each j < n, paths[j] receives headers[j] (the caller's "#isoforms=...\n" line), the column
 * line "sampled_psi\tlog_score\n" and one row per kept sample, "%.4f,%.4f,...\t%.2f\n", with the
 * digits Python's % operator prints (nan for NaN).  The rows are formatted and written by n_threads
 * host threads (<= 0: all cores): at 5000 rows per event the reference's Python loop is the slowest
 * step of a whole-genome run once sampling takes milliseconds.  Needs downloaded results. */
int miso_batch_write_miso_files(const miso_batch_t *batch, int n, const int *event_index,
                                const char *const *paths, const char *const *headers, int n_threads);
/* tests: the writer's number formatter on its own ("%.2f" / "%.4f"), NUL-terminated strings `stride`
 * bytes apart */
int miso_selftest_format(const double *x, int n, int decimals, char *out, int stride);
/* tests: the stopping rule of stop = MISO_STOP_CONVERGENT_MEAN on its own (splicing_i_check_convergent_mean,
 * miso.c:556-636): samples = noSamples columns of noiso values, column i from chain i % noChains; *stop = 1 converged.
 * Host arithmetic, no device needed. */
int miso_selftest_convergent_mean(const double *samples, int noiso, int noChains, int noSamples, int *stop);
/* tests: the planner's MISO_* tuning knobs as the next upload or launch would read them now (csrc/knobs.hpp Knobs::from_env):
 * one "NAME=value" line per knob that is set -- a switch as 1, a number as parsed and clamped, a list with commas --
 * NUL-terminated, cut at `cap` bytes.  Returns the bytes the whole text needs (buf may be NULL), -1 out of memory.
 * No device needed. */
int miso_selftest_knobs(char *buf, int cap);
/* parity instrumentation: FNV-1a over every chain's per-iteration assignment counts
   (counts_hash: noChains words) and, if want_counts_trace, the counts themselves
   ((noIterations+1) x noChains x noiso int32, row m = counts the MH step of iteration m saw,
   last row = final state). */
int miso_batch_get_trace(const miso_batch_t *batch, int event_index, uint64_t *counts_hash,
                         int32_t *counts_trace);

/* Posterior summaries on the device, from the samples of the last launch (after miso_batch_sync;
   no miso_batch_download needed): what summarize_miso computes per event
   (misopy/credible_intervals.py:4-72): per isoform the mean of psi and the Chen-Shao credible
   interval = order statistics int(round(alpha/2 n)) - 1 and int(round((1-alpha/2) n)) - 1 of the
   sorted samples, alpha = 1 - confidence_level.  mean / ci_low / ci_high: noiso doubles each. */
int miso_batch_summarize(miso_batch_t *batch, double confidence_level);
/* The same summaries of the samples AS THE `.miso` FILE HANDS THEM ON: summarize_miso never sees the sampler's
   doubles, it parses the file's "%.4f" text (misopy/samples_utils.py:130-262).  Every sample is first rounded to
   four decimals exactly as a correctly rounded "%.4f" prints it and read back as the nearest double; the credible
   interval bounds are order statistics of those values, the mean their exact sum / n: what the reference computes
   from the file this run writes, bit for bit for the bounds, to the last bit or two of a float sum for the mean. */
int miso_batch_summarize_as_text(miso_batch_t *batch, double confidence_level);
int miso_batch_get_summary(const miso_batch_t *batch, int event_index, double *mean, double *ci_low,
                           double *ci_high);

/* Chain diagnostics on the device, from the samples of the last launch (same preconditions as miso_batch_summarize;
   DESIGN.md 14): per (event, isoform) column the split R-hat of its chains, the effective sample size and Monte-Carlo
   standard error of the psi mean, and the lag at which Geyer's initial monotone sequence was cut.  Sample column s
   belongs to chain s % noChains; each chain's n = S div noChains draws are split into their first and last h = n div 2.
   noChains = 0: the batch's own chains -- MISO_EINVAL for a batch of adopted samples (miso_batch_from_samples,
   miso_batch_from_miso_text), which has none; any other value is used as given (1 .. 2048).  h < 4: MISO_EINVAL
   "Too few samples per chain for diagnostics", before any launch.  A column that is constant or holds a NaN or an
   infinity gets rhat = ess = mcse = NaN and lag = 0.  rhat / ess / mcse / lag: noiso doubles each. */
int miso_batch_diagnose(miso_batch_t *batch, int noChains);
int miso_batch_get_diagnostics(const miso_batch_t *batch, int event_index, double *rhat, double *ess, double *mcse,
                               double *lag);
/* Kernel time (HIP events) of the last miso_batch_summarize[_as_text] and miso_batch_diagnose of this batch, ms; 0 before. */
int miso_batch_pass_ms(const miso_batch_t *batch, float *summarize_ms, float *diagnose_ms);

/* Rank-normalised chain diagnostics on the device (Vehtari, Gelman, Simpson, Carpenter & Buerkner 2021),
   same preconditions and the same split sequences as miso_batch_diagnose.  The N = 2 noChains (S div noChains div 2) used
   draws of a column are replaced by the normal scores of their average ranks (bulk), by the normal scores of the ranks
   of their distance from the median (folded), and by the indicators of lying at or below / at or above the bounds of
   the `confidence_level` interval -- the order statistics of miso_batch_summarize, taken over the N used draws -- and
   each goes through miso_batch_diagnose's computation:  rhat_bulk, rhat_fold, ess_bulk, ess_ci_low, ess_ci_high;
   distinct: the number of distinct values among the used draws.  noiso doubles each.  A column that holds a NaN or an
   infinity gets five NaN and distinct = 0, a constant one five NaN and distinct = 1; a column whose folded values are
   all equal (a two-valued column) gets rhat_fold = NaN.  MISO_EINVAL before any launch, for the whole batch:  "Too few
   samples per chain for diagnostics" as miso_batch_diagnose;  "Too few samples for a credible interval" as
   miso_batch_summarize, with N for the sample count;  "Too many samples for rank diagnostics": N > 8192;  "Too many chains
   for rank diagnostics": noChains > 512 (the column is sorted in the workgroup's local memory). */
int miso_batch_diagnose_rank(miso_batch_t *batch, int noChains, double confidence_level);
int miso_batch_get_rank_diagnostics(const miso_batch_t *batch, int event_index, double *rhat_bulk, double *rhat_fold,
                                    double *ess_bulk, double *ess_ci_low, double *ess_ci_high, double *distinct);
/* Kernel time (HIP events) of the last miso_batch_diagnose_rank of this batch, ms; 0 before. */
int miso_batch_rank_pass_ms(const miso_batch_t *batch, float *ms);

/* Posterior predictive model check of single-end events (csrc/kernels_model_check.hip; the arithmetic
   contract is include/miso_model_check.h).  The model draws a read uniformly from the start positions of its isoform, so a
   read falls into class c of the gene's assignment matrix (pattern_c = its set of isoforms, m_c > 0 its start positions,
   columns in miso_gene_assignment_matrix's order) with probability p_c = w_c / T_0, w_c = m_c sum_{k in pattern_c} psi_k.
   For every posterior row s the kernel draws a replicate n_rep ~ Multinomial(N, p(psi_s)) and compares the Freeman-Tukey
   discrepancy D(n, p) = sum_c (sqrt n_c - sqrt(N p_c))^2 of the replicate with the observed counts'.  A row whose T_0 is
   zero, negative or not finite is a bad row: counted, skipped.
     status      MISO_FIT_OK; MISO_FIT_NO_GENE (added without a gene structure); MISO_FIT_NO_READS (N = 0);
                 MISO_FIT_TOO_MANY_CLASSES (more than 64 classes or isoforms); MISO_FIT_NO_ROWS (every row bad).
                 Every other result of an event whose status is not MISO_FIT_OK is 0.
     rows, bad_rows, exceed = #{s : D(n_rep_s, p_s) >= D(n, p_s)}: the posterior predictive p-value is exceed / rows
     sum_obs, sum_rep = the sums of the two discrepancies over the rows
     per class: expected = N (sum_s p_c) / rows;  ge = #{n_rep_c >= n_c},  le = #{n_rep_c <= n_c}
   The integers are exact; the double sums are made in one fixed order (every thread its own rows ascending, then the 256
   partial sums folded in halves): two runs give the same bits.
   miso_model_check, the raw call: n_events events; event i has noiso[i] isoforms, n_classes[i] classes at
   class_off[i] .. class_off[i + 1] of pattern / m / n (class_off: n_events + 1 entries from 0), n_samples[i] rows of
   noiso[i] doubles at samples + sample_off[i] (row s = psi of draw s; n_sample_doubles = the extent of `samples`), and
   the Philox event id event_id[i]: the replicate of row s draws from the word stream (seed, event_id, chain 0, iteration
   s, site 6).  Results per event, and per class in class_off's layout.  MISO_EINVAL for tables that do not fit together
   (offsets, a pattern naming an isoform >= noiso or none, m < 1, n < 0, N > 2^24, rows outside `samples`);
   MISO_ENODEVICE without a GPU: there is no CPU path.  A failed call leaves the result arrays as they were. */
#define MISO_FIT_OK 0
#define MISO_FIT_NO_GENE 1
#define MISO_FIT_NO_READS 2
#define MISO_FIT_TOO_MANY_CLASSES 3
#define MISO_FIT_NO_ROWS 4
int miso_model_check(int device, int n_events, const int32_t *noiso, const int32_t *n_classes, const int64_t *class_off,
                     const uint64_t *pattern, const int64_t *m, const int32_t *n, const uint64_t *sample_off,
                     const int32_t *n_samples, const uint32_t *event_id, const double *samples, uint64_t n_sample_doubles,
                     uint64_t seed, int32_t *status, int32_t *rows, int32_t *bad_rows, int32_t *exceed, double *sum_obs,
                     double *sum_rep, double *expected, int32_t *ge, int32_t *le, float *kernel_ms);
/* The same for a batch.  miso_batch_set_model_check, before any event is added: MISO_EINVAL for a paired-end batch (its
   classes are compatibility x fragment length), MISO_UNIMPLEMENTED with overHang > 1 (the assignment matrix's own
   limit).  With the switch on, miso_batch_add_event and miso_batch_add_simulated keep the gene's class table; an event
   added any other way has status MISO_FIT_NO_GENE.  With it off nothing is computed and nothing changes.
   miso_batch_model_check_table (host only, no device): the event's table -- status (MISO_FIT_OK, _NO_GENE or
   _TOO_MANY_CLASSES), n_classes, and up to max_classes entries of pattern / m / n; n_reads = N = sum n; n_off = the
   reads with a non-empty compatibility pattern that is no column (clipped reads, indels, a template the positions cannot
   produce); reads compatible with no isoform are in neither.  Any output may be NULL.
   miso_batch_model_check, after the batch was launched (stop = CONVERGENT_MEAN: its further rounds are finished first):
   the raw call's kernel over the resident samples, event ids as the launch's; it only reads.  Results are stored in the
   batch; a refused or failed call leaves the earlier ones in place.  miso_batch_get_model_check: one event's results,
   the per-class ones up to max_classes entries.  miso_batch_model_check_ms: kernel time (HIP events) of the last pass. */
int miso_batch_set_model_check(miso_batch_t *batch, int on);
int miso_batch_model_check_table(const miso_batch_t *batch, int event_index, int max_classes, int *status, int *n_classes,
                                 uint64_t *pattern, int64_t *m, int32_t *n, int64_t *n_reads, int64_t *n_off);
int miso_batch_model_check(miso_batch_t *batch, uint64_t seed);
int miso_batch_get_model_check(const miso_batch_t *batch, int event_index, int max_classes, int *status, int32_t *rows,
                               int32_t *bad_rows, int32_t *exceed, double *sum_obs, double *sum_rep, double *expected,
                               int32_t *ge, int32_t *le);
int miso_batch_model_check_ms(const miso_batch_t *batch, float *ms);

/* Samples that were produced elsewhere -- parsed `.miso` files: summarize_miso and compare_miso work on directories of
   them (misopy/samples_utils.py:263-329, hypothesis_test.py:186-345).  Event i has noiso[i] isoforms and n_samples
   samples in the file's layout (samples[i]: n_samples rows of noiso[i] values).  The batch lives on `device` and
   supports miso_batch_summarize[_as_text], miso_batch_compare and their getters only. */
int miso_batch_from_samples(int n_events, const int *noiso, int n_samples, const double *const *samples, int device,
                            miso_batch_t **batch);

/* The same batch straight from the files' TEXT, decoded on the device (a `.miso` file after its two header lines, or
   the psi_vals_and_scores column of a `.miso_db` row; miso_amd/miso_db.py).  Event i's body is
   text[offsets[i] .. offsets[i + 1]); a row is "f_1,...,f_K<TAB>g<LF>", empty lines are ignored, the last LF may be
   missing.

   miso_text_shape (host only, no device needed): per event the isoform count (commas before the first TAB of the first
   non-empty line, plus one; 0 for a body without one) and the number of non-empty lines.  The caller groups events by
   the latter: a batch has one n_samples.

   miso_batch_from_miso_text: the sample pool is written by the decode kernel only.  status[i] == 0: event i's pool
   region holds its n_samples x noiso[i] values, each the correctly rounded double of its decimal text (what strtod
   gives).  status[i] != 0, a sum of the MISO_TEXT_* bits below: the event is not in the fast grammar, its pool region is
   unspecified and its summaries must not be read; every other event is unaffected.  The fast grammar: a psi field is
   -?digits[.digits] with at most 15 significant digits and at most 22 digits after the point (value = digits as an
   integer / 10^decimals, one IEEE division of two exact doubles); the log-score field g is not stored but must be
   -?digits[.digits], nan, inf or -inf; no CR, no exponent, K fields in every row, n_samples rows.
   The text streams through the device in chunks of whole events of about chunk_bytes (<= 0: the default, 64 MiB; an
   event larger than that is a chunk of its own), so device memory is bounded by the chunk size plus the pool.
   MISO_ENODEVICE without a GPU: there is no CPU path.  stats may be NULL. */
#define MISO_TEXT_EPSI 1    /* a psi field outside the fast grammar (exponent, nan, inf, > 15 digits, > 22 decimals)  */
#define MISO_TEXT_EROW 2    /* a row with another number of fields than noiso[i], or without TAB                      */
#define MISO_TEXT_ESCORE 4  /* a log-score field that is no plain decimal, nan, inf or -inf (a CR at the line's end)  */
#define MISO_TEXT_ECOUNT 8  /* another number of non-empty lines than n_samples                                       */
typedef struct {
  int64_t chunks;        /* device chunks                                                                  */
  int64_t decoded;       /* events with status 0                                                           */
  int64_t not_decoded;   /* events with another status                                                     */
  int64_t text_bytes;    /* bytes of text sent to the device                                               */
  int64_t sample_bytes;  /* bytes of samples the pool holds (8 per psi field)                              */
  double kernel_ms;      /* the decode kernels alone (device time, summed over the chunks)                 */
  double decode_ms;      /* copies to the device and kernels (device time, summed over the chunks)         */
  double total_ms;       /* wall time of the whole call                                                    */
} miso_text_stats_t;
int miso_text_shape(int n_events, const unsigned char *text, const int64_t *offsets, int32_t *noiso, int32_t *n_rows);
int miso_batch_from_miso_text(int n_events, const unsigned char *text, const int64_t *offsets, const int *noiso,
                              int n_samples, int device, int64_t chunk_bytes, miso_batch_t **batch, int32_t *status,
                              miso_text_stats_t *stats);

/* Two-sample comparison on the device (compare_miso, misopy/hypothesis_test.py:89-179, 348-380):
   `sample1` and `sample2` hold the SAME events in the same order (one batch per RNA-seq sample),
   both launched on the same device.  Per event and isoform: index-paired delta = psi1 - psi2;
   mean|delta| <= 0.009 or constant delta -> Bayes factor 0 (posterior peaked on the null);
   otherwise Gaussian KDE of delta with covariance factor `smoothing` (reference: 0.3) evaluated at
   0, BF = 1 / density, 1e12 if the density is 0, capped at 1e12.  Results are stored in sample1. */
int miso_batch_compare(miso_batch_t *sample1, miso_batch_t *sample2, double smoothing);
int miso_batch_get_comparison(const miso_batch_t *sample1, int event_index, double *mean1, double *mean2,
                              double *bayes_factor, double *density_at_0);   /* noiso doubles each */

/* The comparison of two batches that both ran with the exact-posterior mode (miso_batch_set_exact), without a draw
   (csrc/kernels_exact_compare.hip).  Preconditions and errors as miso_batch_compare: both synced,
   same device, the same events in the same order.  An event pair is EXACT-COMPARABLE when the exact mode took the event
   in both batches and its two effective lengths are bit-equal in both; every other pair gets was_exact = 0 and nothing
   else.  For a comparable pair the product of the two posteriors is a posterior of the same family (pooled counts,
   hyperparameters h1 + h2 - 1), so the posterior density of delta = psi_1 - psi_2 at 0 is a ratio of three normalisers of
   the mode's own tables: log_density_at_0 = log Z12 - log Z1 - log Z2.  The Savage-Dickey Bayes factor is the prior
   density of delta at 0 (from the hyperparameters, std::lgamma on the host; 1 at h = (1, 1)) over it:
   log10_bayes_factor is uncapped, bayes_factor = min(exp(log BF), 1e12); no "peaked on the null" rule applies.
   z: n_z points in (-1, 1), 0 <= n_z <= 8: cdf[j] = P(psi_1 - psi_2 <= z[j]), the trapezoid sum over the narrower
   posterior's 2049 grid points of its density times the other posterior's tabulated CDF at the shifted argument.
   mean1 / mean2: the grid means of psi_0.  No Monte-Carlo error, no dependence on the seed.  MISO_EINVAL when either
   batch lacks the exact mode, n_z is outside [0, 8] or a z outside (-1, 1); MISO_ENODEVICE without a GPU.  Results are
   stored in sample1; the launch appears in miso_batch_last_kernels as exact_compare. */
int miso_batch_compare_exact(miso_batch_t *sample1, miso_batch_t *sample2, const double *z, int n_z);
int miso_batch_get_exact_comparison(const miso_batch_t *sample1, int event_index, double *mean1, double *mean2,
                                    double *log_density_at_0, double *bayes_factor, double *log10_bayes_factor,
                                    double *cdf /* n_z */, int *was_exact);
/* The same comparison for two PAIRED-END batches that both ran with miso_batch_set_exact_paired
   (csrc/kernels_exact_paired_compare.hip).  Preconditions and errors as miso_batch_compare_exact; an
   event is comparable when the paired exact mode took it in both batches (nothing has to be equal between the samples:
   each has its own A = exp(assscores), its own pairs).  The product of the two posteriors is tabulated as a density of
   its own over both samples' resident pair records -- pooled exponents, hyperparameters h1 + h2 - 1, both pair sums, both
   denominators --, and log_density_at_0, the Bayes factor and cdf follow as above.  MISO_EINVAL when either batch is
   single-end or lacks the paired exact mode.  Results are stored in sample1 in the place of miso_batch_compare_exact's and
   read through miso_batch_get_exact_comparison; the launch appears in miso_batch_last_kernels as exact_paired_compare. */
int miso_batch_compare_exact_paired(miso_batch_t *sample1, miso_batch_t *sample2, const double *z, int n_z);
/* Kernel time (HIP events) of the last miso_batch_compare and of the last miso_batch_compare_exact or
   miso_batch_compare_exact_paired stored in this batch, ms; 0 before. */
int miso_batch_compare_ms(const miso_batch_t *sample1, float *compare_ms, float *exact_compare_ms);
/* Quantiles of delta = psi_1 - psi_2 from the exact CDF H(z) = P(psi_1 - psi_2 <= z), without a draw
   (csrc/kernels_exact_delta.hip, csrc/kernels_exact_paired_delta.hip).  Preconditions and errors as
   miso_batch_compare_exact (single-end batches) or miso_batch_compare_exact_paired (paired-end batches: the batch kind
   chooses); in addition sample1 must hold an exact comparison of either kind -- MISO_EINVAL "has not run" otherwise, as
   miso_batch_get_exact_comparison's --, and exactly the pairs whose was_exact is set there are taken, sample2 being the
   batch that comparison was made with.  H is the comparison's own cdf (the same operations in the same order); the device
   chooses the points itself: per probability five rounds of eight points inside the bracket, which starts as (-1, 1) with
   H = 0 and 1 at its ends, then one linear interpolation inside the last bracket, 2 / 9^5 wide.  p: n_p probabilities,
   1 <= n_p <= 4, each inside (0, 1), MISO_EINVAL otherwise.  No Monte-Carlo error, no dependence on the seed.  Results are
   stored in sample1 beside the comparison's; a later miso_batch_compare_exact or miso_batch_compare_exact_paired on sample1
   discards them.  The launch appears in miso_batch_last_kernels as exact_delta_quantiles or exact_paired_delta_quantiles.
   miso_batch_get_exact_delta_quantiles: quantiles[k] of p[k], cdf_at_0 = H(0.0) = P(delta <= 0); was_exact = 0 and nothing
   else for a pair that is not comparable.  miso_batch_exact_delta_ms: kernel time (HIP events) of the last such launch
   stored in this batch, ms; 0 before. */
int miso_batch_exact_delta_quantiles(miso_batch_t *sample1, miso_batch_t *sample2, const double *p, int n_p);
int miso_batch_get_exact_delta_quantiles(const miso_batch_t *sample1, int event_index, double *quantiles /* n_p */,
                                         double *cdf_at_0, int *was_exact);
int miso_batch_exact_delta_ms(const miso_batch_t *sample1, float *ms);

/* The same quantiles between two GROUPS of replicates, pooled, from the exact posteriors and without a draw
   (csrc/kernels_exact_delta_groups.hip).  Single-end two-isoform events only.  The law of "psi of a
   replicate of group 1 minus psi of a replicate of group 2", equal weights, is the mixture of the n1 * n2 pairwise laws:
   H(z) = (sum_a sum_b H_ab(z)) / (double) (n1 * n2), summed from 0.0 with a outer and b inner, H_ab being
   miso_batch_exact_delta_quantiles' CDF of the pair (a, b) bit for bit; the search is that function's on this H.
   miso_exact_delta_groups works on caller-given statistics: stats7_g holds n_events * n_g rows {n10, n01, n, e0, e1, h0, h1},
   [event][replicate][7], 1 <= n1, n2 <= 8; p: 1 <= n_p <= 4 probabilities inside (0, 1); z: 0 <= n_z <= 8 points inside
   (-1, 1); MISO_EINVAL otherwise, MISO_ENODEVICE without a device, in either case before anything is allocated.  An event is
   comparable when every one of its rows is eligible for the exact mode and all carry bit-equal (e0, e1): it gets
   was_exact[event] = 1 and the row out[event * (2 + n_p + 1 + n_z)] = {m1, m2, q[0 .. n_p), H(0.0), H(z[0 .. n_z))}, m_g the
   mean over the group's replicates of their posterior means of psi.  Any other event gets was_exact = 0 and its row is left
   untouched; that is no error.  A call is split into launches over event ranges so that what it holds on the device stays
   within 256 MiB; max_events_per_launch > 0 lowers the range further, 0 derives it.  kernel_ms (may be NULL): the HIP-event
   time of the launches.
   miso_batch_get_exact_stats: the seven statistics of an event of a launched single-end batch as the functions above take
   them; was_exact = 0 (and the statistics as they are) for an event the exact mode did not take and for every event of a
   paired-end batch.
   miso_batch_exact_delta_groups: the same pass over launched batches, preconditions as miso_batch_compare_pairs_groups (the
   same events in the same order, one device); a paired-end batch or one that did not run with the exact mode is MISO_EINVAL
   naming the group and the index of the batch.  The rows come from miso_batch_get_exact_stats; an event that some batch's
   exact mode did not take is not comparable.  out_len: doubles available in out, n_events * (2 + n_p + 1 + n_z) at least;
   was_exact: n_events ints.  Nothing is stored in any batch. */
int miso_exact_delta_groups(const double *stats7_1, int n1, const double *stats7_2, int n2, int n_events, const double *p, int n_p,
                            const double *z, int n_z, int max_events_per_launch, double *out, int *was_exact, float *kernel_ms);
int miso_batch_get_exact_stats(const miso_batch_t *batch, int event_index, double *stats7, int *was_exact);
int miso_batch_exact_delta_groups(miso_batch_t *const *group1, int n1, miso_batch_t *const *group2, int n2, const double *p, int n_p,
                                  const double *z, int n_z, double *out, int64_t out_len, int *was_exact, float *kernel_ms);

/* The same for PAIRED-END replicates (csrc/kernels_exact_paired_delta_groups.hip): the mixture, the
   search, p, z, the output row, was_exact, the launch ranges and kernel_ms are as above; H_ab is
   miso_batch_exact_delta_quantiles' CDF of two paired-end posteriors bit for bit (A, the replicate with the narrower window in
   psi, contributes its own tabulated density; a tie goes to the group-1 replicate).  No equality of A0, A1 between replicates
   is needed.
   miso_exact_paired_delta_groups works on caller-given elements: stats6, m, offs are arrays of n1 + n2 pointers, group 1's
   replicates first, each replicate's elements in miso_selftest_exact_paired's layout over the same n_events (stats6[r]:
   n_events rows {n10, n01, A0, A1, h0, h1}; offs[r]: n_events + 1 offsets from 0, ascending; m[r]: offs[r][n_events] pairs
   (m0, m1), NULL allowed when there is none).  An event is comparable when every replicate's row passes
   miso_exact_paired_eligible; any other event gets was_exact = 0 and an untouched row.  MISO_EINVAL, before anything is
   allocated: counts outside their ranges, p, z, offsets that do not start at 0 or descend, a negative count or a pair
   probability outside [2^-63, 1] in a comparable event.
   miso_batch_exact_paired_delta_groups: the same pass over launched batches, preconditions as
   miso_batch_compare_pairs_groups; every batch must be paired-end and have run with miso_batch_set_exact_paired, otherwise
   MISO_EINVAL naming the group and the index of the batch.  An event that some batch's mode did not take is not comparable.
   The kernels read the batches' resident pair records, on the first batch's stream after all have been waited for.  Nothing
   is stored in any batch.
   miso_batch_get_exact_paired_element: event_index of a launched batch as the first function takes it: the six statistics,
   n_pairs, and -- m != NULL, m_cap pairs of room, MISO_EINVAL when too few -- the drawing pairs' probabilities (m0, m1) in
   record order, the doubles the kernels multiply.  was_exact = 0, n_pairs = 0 and nothing else for an event the paired exact
   mode did not take and for every event of a single-end batch. */
int miso_exact_paired_delta_groups(const double *const *stats6, const double *const *m, const int64_t *const *offs, int n1, int n2,
                                   int n_events, const double *p, int n_p, const double *z, int n_z, int max_events_per_launch,
                                   double *out, int *was_exact, float *kernel_ms);
int miso_batch_exact_paired_delta_groups(miso_batch_t *const *group1, int n1, miso_batch_t *const *group2, int n2, const double *p,
                                         int n_p, const double *z, int n_z, double *out, int64_t out_len, int *was_exact,
                                         float *kernel_ms);
int miso_batch_get_exact_paired_element(const miso_batch_t *batch, int event_index, double *stats6, double *m, int64_t m_cap,
                                        int64_t *n_pairs, int *was_exact);

/* The posterior of delta = psi_1 - psi_2 over ALL pairs of the two samples' draws (csrc/kernels_compare_pairs.hip, DESIGN.md
   section 19): the samples are independent posteriors, so given the draws the law of delta is the empirical law of the
   M = S1 * S2 differences, not of the index-paired ones.  Preconditions and errors as miso_batch_compare -- both launched
   (a batch not yet synced is waited for), same device, the same events with the same isoform counts in the same order --
   except that the two batches' n_samples may differ.
   Per (event, isoform), with a[0..S1) and b[0..S2) the rows the summaries use and D the multiset of the IEEE doubles a_i - b_j:
   ci_low / ci_high: the order statistics of D at ranks max(0, floor(alpha/2 M + 0.5) - 1) and floor((1 - alpha/2) M + 0.5) - 1,
   alpha = 1 - confidence_level (the summaries' rule over M; the lower rank is clamped where they refuse);  median: the order
   statistic at rank (M - 1) / 2 (the lower median);  a zero is +0.0;  n_gt0 = #{d > 0}, n_lt0 = #{d < 0}, and per threshold
   n_abs_ge = #{d >= tau} + #{d <= -tau}, exact integers, compared as doubles compare (a decimal difference that equals tau may
   be the double below it: 0.3 - 0.1 < 0.2).  A column pair with a NaN or an infinity in either column: three NaN, counts 0,
   finite = 0; likewise every column of an event whose text miso_batch_from_miso_text did not decode (status != 0) in either
   batch; other columns and events are unaffected.  tau: n_tau thresholds, 0 <= n_tau <= 4, each inside (0, 1);
   confidence_level inside (0, 1).  MISO_EINVAL, nothing launched: any of these violated, or more than 8192 samples per event
   in either batch (both sorted columns stay in the workgroup's local memory).  Results are stored in sample1 beside
   miso_batch_compare's (which they leave as they are); the launch appears in miso_batch_last_kernels as compare_pairs.
   miso_batch_get_pair_comparison: noiso values each, n_abs_ge noiso x n_tau (isoform-major), *n_pairs = M; any pointer may be
   NULL. */
int miso_batch_compare_pairs(miso_batch_t *sample1, miso_batch_t *sample2, double confidence_level, const double *tau, int n_tau);
/* The same of the draws as the `.miso` files print them: every draw rounded to "%.4f" and read back first, as
   miso_batch_summarize_as_text does -- what miso_batch_compare_pairs gives for batches made from the files a run writes. */
int miso_batch_compare_pairs_as_text(miso_batch_t *sample1, miso_batch_t *sample2, double confidence_level, const double *tau,
                                     int n_tau);
int miso_batch_get_pair_comparison(const miso_batch_t *sample1, int event_index, double *median, double *ci_low, double *ci_high,
                                   int64_t *n_gt0, int64_t *n_lt0, int64_t *n_abs_ge, int32_t *finite, int64_t *n_pairs);
/* Kernel time (HIP events) of the last miso_batch_compare_pairs stored in this batch, ms; 0 before. */
int miso_batch_compare_pairs_ms(const miso_batch_t *sample1, float *ms);

/* Every pair of two groups of samples (biological replicates) in one device pass.  group1[i], group2[j]: batches that
   hold the SAME events in the same order with the same n_samples, on the same device (what miso_batch_compare requires of
   its two); n1, n2 >= 1.  out: n1 * n2 * tot doubles, tot = sum over events of 4 * noiso; pair (i, j), event e, isoform k
   at ((i * n2 + j) * tot + off[e] + 4 * k), off[e] = 4 * (isoforms of the events before e): mean1, mean2, bayes_factor,
   density_at_0 -- bit for bit what miso_batch_compare(group1[i], group2[j], smoothing) + miso_batch_get_comparison give.
   One launch serves all pairs: a workgroup per (event, isoform) reads the n1 + n2 sample columns once into LDS and takes
   every pair from there.  staging says which columns: MISO_STAGE_AUTO picks by what fits beside the reduction buffers
   (both groups, else the smaller group, else none: the columns then come from global memory, same bits);
   the other values force one (tools/compare_groups_bench.py measures them; one that does not fit is MISO_EINVAL).
   kernel_ms (may be NULL): the kernel's time.  Errors as miso_batch_compare, naming the group and index of the batch
   at fault; MISO_ENODEVICE without a GPU. */
#define MISO_STAGE_AUTO 0
#define MISO_STAGE_BOTH 1
#define MISO_STAGE_SMALLER 2
#define MISO_STAGE_NONE 3
int miso_batch_compare_groups(miso_batch_t *const *group1, int n1, miso_batch_t *const *group2, int n2,
                              double smoothing, int staging, double *out, int64_t out_len, float *kernel_ms);

/* miso_batch_compare_pairs for two groups of replicates, pooled (csrc/kernels_compare_pairs_groups.hip).
   group1, group2: as miso_batch_compare_groups requires them -- the same events in the same order with the same isoform
   counts and the same n_samples = S, one device, launched (a batch not yet synced is waited for); n1, n2 >= 1.
   Per (event, isoform): A = the multiset union of the group-1 batches' columns (N1 = n1 * S draws), B the same of group 2
   (N2 = n2 * S), D the multiset of the IEEE doubles a - b, M = N1 * N2; ranks, order statistics, counts, the +0.0 of a zero,
   not-finite columns and undecoded events (in ANY batch) exactly as miso_batch_compare_pairs defines them over this D.  The
   result does not depend on the order of the batches within a group; n1 = n2 = 1 gives miso_batch_compare_pairs bit for bit.
   as_text != 0: every draw rounded to "%.4f" and read back first, as miso_batch_compare_pairs_as_text.
   out: pairs_words = 6 + n_tau 64-bit words per (event, isoform), event e's isoform k at (isoforms of the events before e + k)
   * pairs_words: the bits of median, ci_low, ci_high; n_gt0; n_lt0; finite; n_abs_ge per threshold.  *n_pairs = M;
   *kernel_ms: the launches' time (a call is split over event ranges so that its device workspace stays within 256 MiB);
   either may be NULL.  Nothing is stored in a batch: earlier results of every batch stay as they were.
   MISO_EINVAL, nothing launched: 0 <= n_tau <= 4, each tau inside (0, 1), confidence_level inside (0, 1) violated; N1 or N2
   above 16384; out too short; a batch at fault (the message names its group and index).  MISO_ENODEVICE without a GPU. */
int miso_batch_compare_pairs_groups(miso_batch_t *const *group1, int n1, miso_batch_t *const *group2, int n2,
                                    double confidence_level, const double *tau, int n_tau, int as_text, uint64_t *out,
                                    int64_t out_len, int64_t *n_pairs, float *kernel_ms);

/* Part-level psi: isoform-group columns (csrc/kernels_groups.hip).  A group is (group_event[g],
   group_mask[g]): an event index of the batch and a set of that event's isoform indices, bit k = isoform k; the mask must be
   non-empty and set no bit at or above the event's isoform count, and the event may have 64 isoforms at most.  The group's
   draw of pool row s is v_s = ((0.0 + psi[s][k1]) + psi[s][k2]) + ... over the mask's k ascending, plain IEEE adds; with
   as_text != 0 every member is first rounded to "%.4f" and read back as miso_batch_compare_pairs_as_text does it.  v_s + 0.0
   is the column's value.  A NaN or an infinity among the v_s makes the group not finite (values of isoforms outside the mask
   are never read).
   miso_batch_summarize_isoform_groups: out[3 g ..] = mean, ci_low, ci_high of group g's column, by miso_batch_summarize's
   rules: the mean as 256 strided partial sums folded in halves, over n_samples; the bounds the order statistics of the
   strict ranks (too few samples: MISO_EINVAL).  Not finite: three NaN.
   miso_batch_compare_pairs_isoform_groups: per group what miso_batch_compare_pairs defines for a column pair, a = the
   group's column of sample1 (S1 draws), b = that of sample2 (S2 draws, S1 != S2 allowed), M = S1 * S2: out[(6 + n_tau) g ..]
   = the bits of median, ci_low, ci_high; n_gt0; n_lt0; finite; n_abs_ge per threshold.  The batches as
   miso_batch_compare_pairs requires them; an event either batch did not decode is not finite.  *n_pairs = M.
   Both: n_samples <= 8192 per batch; n_groups = 0 is valid and launches nothing; a batch not yet synced is waited for;
   *kernel_ms (may be NULL) the launches' time (a call is split over group ranges so that its result buffer stays within
   256 MiB).  Nothing is stored in a batch.  MISO_EINVAL before any launch (the message names the group at fault);
   MISO_ENODEVICE without a GPU.  The launches appear in miso_batch_last_kernels as summarize_groups and
   compare_pairs_groups_iso. */
int miso_batch_summarize_isoform_groups(miso_batch_t *batch, const int32_t *group_event, const uint64_t *group_mask,
                                        int64_t n_groups, double confidence_level, int as_text,
                                        double *out /* 3 per group */, int64_t out_len, float *kernel_ms);
int miso_batch_compare_pairs_isoform_groups(miso_batch_t *sample1, miso_batch_t *sample2, const int32_t *group_event,
                                            const uint64_t *group_mask, int64_t n_groups, double confidence_level,
                                            const double *tau, int n_tau, int as_text,
                                            uint64_t *out /* 6 + n_tau words per group */, int64_t out_len,
                                            int64_t *n_pairs, float *kernel_ms);

/* device_match batches: kernel time of the matching launch done by miso_batch_upload, and (tests:
   want_counts_trace batches only) the kernel's output for event i in the layout of
   miso_match_iso[_paired]: match noiso x n_reads, fragmentLength likewise or NULL. */
int miso_batch_last_match_ms(const miso_batch_t *batch, float *ms);
int miso_batch_get_match(const miso_batch_t *batch, int event_index, double *match, int *fragmentLength);

/* The run-dependent fields of the `.miso` header line (misopy/miso_sampler.py:376-454) of n events in one call.  Writes,
   per event, the line "U<TAB>percent_accept<TAB>counts<TAB>assigned_counts\n" into buf (NUL-terminated): U = 1 when every
   read of the event is unassigned (the caller skips it, miso_sampler.py:352-354); percent_accept as "%.2f"; counts =
   "(1,0):12,(0,1):34" (read class : reads); assigned_counts = "0:5,1:41" (reads_utils.py:37-46).  *needed = bytes the
   text takes incl. the NUL; nothing is written when cap is smaller (call again).  Needs downloaded results. */
int miso_batch_header_fields(const miso_batch_t *batch, int n, const int *event_index, char *buf, int64_t cap,
                             int64_t *needed);

/* names of the kernels the last launch used (for profiles): e.g. "sampler_k2<3, false>" */
int miso_batch_last_kernels(const miso_batch_t *batch, char *buf, int buflen);

/* How many launches of this batch miso_batch_sync() had to repeat because a chain spread over several workgroups
   (the events with 10^4 ... 10^5 reads) did not get all of them resident in time on a busy device.  The repeat runs
   in the same process with one workgroup per chain and returns the same results bit for bit; the batch never fails
   for it -- the reference's workers share nothing either (misopy/miso.py:165-187).  0 on an idle device. */
int miso_batch_coop_retries(const miso_batch_t *batch, int *n);

/* stop = MISO_STOP_CONVERGENT_MEAN (miso.c:903-925, miso_paired.c:501-523): after a launch whose chains have not
   converged for some events -- splicing_i_check_convergent_mean on their kept samples --, miso_batch_sync() runs those
   events again with noIterations' = 3 noIterations - 2 noBurnIn, noBurnIn' = noIterations (while noIterations <
   maxIterations), and the LAST noSamples of that round replace the event's samples (miso.c:976-983): every getter,
   the summaries and the file writer see a batch of noSamples samples per event, as the reference returns them.
   rundata.noAccepted / noRejected count the last round (paired-end: all rounds), as the reference's do.
   *rounds = rounds the slowest event of the last launch took (1: every event converged on its own schedule, and
   always with MISO_STOP_FIXEDNO).
   The rounds have no limit of their own, as in the reference: an event goes on until it converges or its schedule
   reaches maxIterations.  The one limit is the device's 32-bit iteration counter.  The device keeps no chain state
   between launches and runs round r from the chain's first iteration, so the iterations of ALL rounds through the next
   one must stay within INT32_MAX (2^31 - 1); an event that would pass that keeps the samples of its last round, where
   the reference would go on.  The kept window doubles with every round, so this is reached before round 32 whatever
   the schedule; with 5000 / 500 (window 4500) round 18 is the first that does not fit, 2.4 x 10^9 iterations from the
   chain's start. */
int miso_batch_rounds(const miso_batch_t *batch, int *rounds);

/* Measurement: what the last launch put on the device, kernel by kernel (bench.py's VALU roofline
   prices it with the kernels' instruction counts, tools/isa_count.py): wavefronts launched, the sum
   over wavefronts of the read loop's trips per Gibbs step, Gibbs steps run (noIterations + 1),
   chains, and the Philox words (uniforms) the read loops generate per Gibbs step. */
typedef struct {
  char name[64];
  double waves, trips, iterations, chains, words;
} miso_kernel_stat_t;
int miso_batch_launch_stats(const miso_batch_t *batch, miso_kernel_stat_t *stats, int max_kernels,
                            int *n_kernels);
/* The version of the counter-mode contract this library draws by (include/miso_philox.h MISO_CONTRACT_VERSION): seeded
   results are comparable between builds -- and with the CPU checker -- only at equal versions.  No device needed. */
int miso_contract_version(void);

/* Measurement: the shader clock the last launch ran at.  With the probe on, every launch starts ONE extra wavefront on a
   stream of its own that sleeps beside the sampler kernels and reads the shader-cycle counter (s_memtime) and the
   constant reference clock (hipDeviceAttributeWallClockRate) at both ends of the launch; miso_batch_sync() turns the pair
   into cycles per nanosecond.  *shader_ghz = 0 when the probe is off or its window did not cover the launch (its stream
   shared the batch's hardware queue, a profiler serialised the dispatches); *window_ms = what it covered.  The reference
   has no counterpart (a CPU's clock is not part of its results either): bench.py prices its VALU roofline with it. */
int miso_batch_set_clock_probe(miso_batch_t *batch, int on);
int miso_batch_last_clock(const miso_batch_t *batch, double *shader_ghz, double *window_ms);
/* Host arithmetic, no device needed: the lanes-per-chain plan of the two-isoform sampler's one-launch-many-widths
   kernel (sampler_k2_multi) for a list of events ordered by drawing reads, most first -- the answer to "events are
   independent and cost O(reads)" (miso.c:845-900) on a machine whose unit of work is a 64-lane wavefront.
   n_draw[n_events]: reads with two compatible isoforms per event; chains per event; paired: 0 / 1;
   resident_workgroups: what the device holds at once (256 single-end, 512 paired-end on MI355X);
   max_chains_per_wave: LDS limit (64 = none); cost5: {per block, step with 1, 2, 3, >= 4 cooperating lanes} in VALU
   instructions or NULL for the measured defaults; forced_target > 0 fixes the bound on a wavefront's step.
   Out: *n_runs runs (<= 16); run r holds events [run_first_event[r], run_first_event[r + 1]) on workgroups
   [run_first_workgroup[r], run_first_workgroup[r + 1]) with run_lanes[r] lanes per chain (512 = one chain per
   workgroup); both first_* arrays have *n_runs + 1 entries (caller provides 17); estimate3 (may be NULL):
   {sum of wavefront steps, longest wavefront step, 1 = one round of resident workgroups / 2 = several}. */
int miso_plan_lanes(const int *n_draw, int n_events, int chains, int paired, int resident_workgroups,
                    int max_chains_per_wave, const double *cost5, double forced_target, int *n_runs,
                    int *run_first_event, int *run_first_workgroup, int *run_lanes, double *estimate3);

/* placement diagnostics: HW_REG_HW_ID of the wavefront that ran each chain of event i (noChains
   words; 0 for kernels that do not record it).  Needs downloaded results. */
int miso_batch_get_placement(const miso_batch_t *batch, int event_index, uint32_t *hw_id);

/* bytes the kernels of the last launch moved by the reference algorithm's accounting
   (SE (8K+20)N, PE (8K+28)N per chain-iteration + load/store) */
int miso_batch_algorithmic_bytes(const miso_batch_t *batch, double *bytes);

/* device-side self test of the arithmetic contract: evaluates miso_detmath / Philox on the GPU
   for n inputs; out_* are host arrays of n doubles (used by tests/test_gpu_contract.py) */
int miso_selftest_detmath(const double *x, int n, double *out_exp, double *out_log,
                          double *out_sqrt, double *out_qnorm);
int miso_selftest_philox(const uint32_t *ctr_key6, int n, uint32_t *out4);

/* The device functions the sampler kernels are built from, one element per thread over host arrays (test-only surface,
   tests/test_gpu_primitives.py).  Element i runs on thread i of 256-thread workgroups: elements 64 w .. 64 w + 63 share a
   wavefront, which is what the routines that choose a route per wavefront see. */
enum { MISO_SELFTEST_EXP_N = 0,   /* csrc/detmath_n.hpp det_exp_n<width>, width 1, 2, 3 or 5 */
       MISO_SELFTEST_LOG_N,       /* det_log_n<width> */
       MISO_SELFTEST_EXP_T,       /* det_exp_t, det_log_t, det_sqrt_pos: width 1 */
       MISO_SELFTEST_LOG_T,
       MISO_SELFTEST_SQRT_POS };
/* out[i * width + j] = routine(x[(i + j * stride) % n]): the `width` interleaved arguments of one call differ; the
   coefficient tables come from registers, loaded as the kernels load them */
int miso_selftest_detmath_n(int routine, int width, const double *x, int n, int stride, double *out);
/* The exp / log of the two-isoform Metropolis-Hastings step as its kernel calls them (csrc/detmath_n.hpp det_exp_r /
   det_log_r): the wavefront's test, then the routine without special cases or the full one.  out[i] = the value,
   route[i] = the route element i's wavefront took (MISO_SELFTEST_ROUTE_*); force_full != 0: the full routine at every
   call, as MISO_K2_FULL_MATH does in the sampler.  Threads behind the last element carry an argument inside the domain. */
enum { MISO_SELFTEST_EXP_R = 0, MISO_SELFTEST_LOG_R };
enum { MISO_SELFTEST_ROUTE_FAST = 0, MISO_SELFTEST_ROUTE_FULL };
int miso_selftest_detmath_routed(int routine, int force_full, const double *x, int n, double *out, int32_t *route);
/* The draw thresholds: out[i] = #{32-bit words u : the reference's test holds for rnd = fl(fl(u 2^-32) T[i]) against
   c[i]}, 0 .. 2^32 -- `rnd < c` (LT) or `!(rnd > c)` (LE).  Exact for every finite c >= 0, T >= 0. */
enum { MISO_SELFTEST_K2_THRESHOLD = 0,      /* kernels_k2.inl k2_threshold(c, T): route chosen per wavefront */
       MISO_SELFTEST_K2_THRESHOLD_EXACT,    /* k2_threshold_exact */
       MISO_SELFTEST_FLAT_LT,               /* kernels_flat.inl: estimate and choice between flat_threshold and */
       MISO_SELFTEST_FLAT_LE,               /*   flat_threshold_fast as sampler_flat's threshold pass makes them */
       MISO_SELFTEST_FLAT_GENERAL_LT,       /* flat_threshold itself */
       MISO_SELFTEST_FLAT_GENERAL_LE,
       MISO_SELFTEST_FLAT_FAST_LT,          /* flat_threshold_fast itself: the caller keeps to its precondition */
       MISO_SELFTEST_FLAT_FAST_LE,          /*   (T in [1e-280, 1e280], 2 <= c (2^32 / T) <= 2^32 - 3) */
       MISO_SELFTEST_DRAW_LT,               /* kernels_grp.inl draw_threshold<false>, estimate as sampler_grp forms it */
       MISO_SELFTEST_DRAW_LE };             /* draw_threshold<true> */
int miso_selftest_threshold(int routine, const double *c, const double *T, int n, uint64_t *out);
/* kernels_flat.inl count_below: out[i] = D[i] + #{j < 4 : w4[4 i + j] < T[i]} */
int miso_selftest_count_below(const int32_t *D, const uint32_t *w4, const uint32_t *T, int n, int32_t *out);
/* One paired-end read's draw per element (kernels_grp.inl): K = 2 .. 10 isoforms, f[i K + k] the read's index into
   fp_rep[il2] for isoform k (il2 - 2 = incompatible; fp_rep[il2 - 2] must be -0.0), psi[i K + k], rule_le[i]: 1 =
   `!(rnd > c)`, 0 = `rnd < c` then the second isoform; word[i] the uniform.  out[i (K + 1) ...] = { the dense read
   loop's pick (pe_all_tests) or -1 where that loop leaves the read to pe_pick_exact, over[K - 1] (1 where the read
   passed over isoform k), pe_pick_exact's pick }. */
int miso_selftest_pe_pick(int K, const uint8_t *f, const double *psi, const double *fp_rep, int il2,
                          const uint32_t *rule_le, const uint32_t *word, int n, int32_t *out);
/* kernels_k2.inl binomial_coop<G>, G = 1, 2, 4, 8 lanes per chain: `count` draws of Binomial(n, p) from the word streams
   (seed, event_id, chain 0, iteration i, MISO_SITE_COUNTS), i = 0 .. count - 1 */
int miso_selftest_binomial(int G, uint64_t seed, uint32_t event_id, int32_t n, double p, int count, int32_t *out);
/* The law that miso_binomial.h's draws follow, by enumeration of the 32-bit words they are functions of, with the header's own
   miso_binomial_btrs / miso_binomial_inversion compiled for the device (tests/test_gpu_binomial_law.py).  Every stride-th
   first word U from stride / 2 (stride: a power of two): BTRS -- the number of second words V that trial 0 accepts (an
   initial segment, its end by 32 steps of bisection) is added to bin k(U); inversion -- 1 is added to bin x(U).  r = min(p,
   1 - p) and the routine are chosen as miso_binomial chooses them, so the bins are r's.  n: 1 .. 2^24, 0 < p < 1; hist:
   n + 1 entries; info: MISO_SELFTEST_LAW_INFO_N entries; kernel_ms (may be NULL): the kernel's time by HIP events. */
enum { MISO_SELFTEST_LAW_REGIME = 0,        /* MISO_SELFTEST_LAW_INVERSION / _BTRS */
       MISO_SELFTEST_LAW_ENUMERATED,        /* words U enumerated: 2^32 / stride */
       MISO_SELFTEST_LAW_TOTAL,             /* the sum of hist */
       MISO_SELFTEST_LAW_RESTARTS,          /* inversion: words whose search ran past its bound (their x is another word's) */
       MISO_SELFTEST_LAW_OUT_OF_RANGE,      /* BTRS: words whose k is outside 0 .. n (no V accepts) */
       MISO_SELFTEST_LAW_NOT_MONOTONE,      /* enumerated words whose k is below the k of the word before */
       MISO_SELFTEST_LAW_SEGMENT_CHECKED,   /* BTRS: words (one in 2^8) whose accepted V were probed around and away from V* */
       MISO_SELFTEST_LAW_SEGMENT_BAD_NEAR,  /*   probes at V* - 2 .. V* + 3 that contradict "accepted = [0, V*]" */
       MISO_SELFTEST_LAW_SEGMENT_BAD_FAR,   /*   the 16 + 16 probes spread over either side that do */
       MISO_SELFTEST_LAW_INFO_N };
enum { MISO_SELFTEST_LAW_INVERSION = 0, MISO_SELFTEST_LAW_BTRS = 1 };
int miso_selftest_binomial_law(int32_t n, double p, uint32_t stride, uint64_t *hist, uint64_t *info, float *kernel_ms);
/* kernels_exact.hip, the posterior stage alone, one wavefront per element: stats7[7 i ...] = {n10, n01, n, e0, e1, h0, h1}
   (n = all reads with a compatible isoform).  out8[8 i ...] = {mean of x, mean of 1 - x, window low, window high (logit
   space), the normalising sum F[G], the mode (logit space), the grid step, the log density at the mode as tabulated};
   icdf[(i n_prob + j) 2 ...] = {x, 1 - x} at the inverse CDF of prob[j] (0 < prob < 1). */
int miso_selftest_exact(const double *stats7, int n, const double *prob, int n_prob, double *out8, double *icdf);
/* kernels_exact_paired.hip, the posterior stage alone, one wavefront per element: stats6[6 i ...] = {n10, n01, A0, A1, h0, h1};
   the element's drawing pairs are m[2 r], m[2 r + 1] = (m0, m1) for r in [offs[i], offs[i + 1]) (offs: n + 1 ascending
   entries from 0; every m inside [2^-63, 1]: sixteen factors multiply without underflow).  out8[8 i ...] = {mean of x, mean of 1 - x, window
   low, window high (logit space), the normalising sum F[G], gref (the largest log density the last window pass met),
   the grid step, log F[G] + gref}; icdf as miso_selftest_exact. */
int miso_selftest_exact_paired(const double *stats6, const double *m, const int64_t *offs, int n, const double *prob,
                               int n_prob, double *out8, double *icdf);
/* kernels_exact_compare.hip on caller-given statistics, one wavefront per pair: stats7_1 / stats7_2 in miso_selftest_exact's
   layout (sample 1, sample 2).  out[(5 + n_z) i ...] = {mean1, mean2, log_density_at_0, bayes_factor, log10_bayes_factor,
   cdf at z[0 .. n_z)} as miso_batch_get_exact_comparison returns them.  MISO_EINVAL when a pair's e0, e1 differ between
   its samples (bit-wise), when a pair is not eligible for the exact mode, n_z is outside [0, 8] or a z outside (-1, 1). */
int miso_selftest_exact_compare(const double *stats7_1, const double *stats7_2, int n, const double *z, int n_z, double *out);
/* kernels_exact_paired_compare.hip on caller-given elements, one wavefront per pair: stats6_s, m_s, offs_s in
   miso_selftest_exact_paired's layout, sample s = 1, 2 (the two samples' pair lists are independent of each other).
   out[(5 + n_z) i ...] as miso_selftest_exact_compare's.  MISO_EINVAL when an element is not eligible for the paired exact
   mode, a probability lies outside [2^-63, 1], n_z is outside [0, 8] or a z outside (-1, 1). */
int miso_selftest_exact_paired_compare(const double *stats6_1, const double *m_1, const int64_t *offs_1, const double *stats6_2,
                                       const double *m_2, const int64_t *offs_2, int n, const double *z, int n_z, double *out);
/* kernels_exact_delta.hip on caller-given statistics, one wavefront per pair: the pairs, their eligibility and the e0, e1
   error as miso_selftest_exact_compare's.  out[(n_p + 1) i ...] = {quantile of psi_1 - psi_2 at p[0 .. n_p), cdf at 0} as
   miso_batch_get_exact_delta_quantiles returns them.  MISO_EINVAL also when n_p is outside [1, 4] or a p outside (0, 1). */
int miso_selftest_exact_delta_quantiles(const double *stats7_1, const double *stats7_2, int n, const double *p, int n_p, double *out);
/* kernels_exact_paired_delta.hip on caller-given elements, one wavefront per pair: the elements and their errors as
   miso_selftest_exact_paired_compare's, p and out as miso_selftest_exact_delta_quantiles'. */
int miso_selftest_exact_paired_delta_quantiles(const double *stats6_1, const double *m_1, const int64_t *offs_1, const double *stats6_2,
                                               const double *m_2, const int64_t *offs_2, int n, const double *p, int n_p, double *out);
/* csrc/text_digits.hpp text_digits, the rounding of summarize_as_text: out[i] = x[i] x 10^4 rounded to the nearest integer,
   ties to even, on the exact product -- the digits of "%.4f" of x[i], sign included.  Finite |x[i]| < 2^38. */
int miso_selftest_text_digits(const double *x, int n, int64_t *out);
/* csrc/k2_flag.hpp, the trip flag of the single-end two-isoform read loop: element i is one lane, its trips the pairs
   start[i] .. start[i + 1] - 1 (start[0] = 0, n + 1 offsets) of m (a trip's running minimum) and k (its stride position,
   < 2^24), noted in order by k2_flag_note.  k2_flag_read's answer: code[i] = 0 no flagged trip, 1 exactly one, at pos[i],
   2 more than one (or one trip with two bits: see the header). */
int miso_selftest_k2_flag(const uint32_t *m, const uint32_t *k, const int32_t *start, int n, int32_t *code, uint32_t *pos);
/* csrc/k2_count.hpp, the per-word arithmetic of the same loop as the device issues it (the assembly statements): element i
   is one lane, its generator words u[start[i]] .. u[start[i + 1] - 1] (start[0] = 0, n + 1 offsets, an even number of words
   each: two per statement) against the high-half threshold th[i] (0 .. 65536).  masked[i] != 0: the tail's statements, inv =
   per word the halves that are not reads (0xFFFF each); 0: the steady trips' statements, inv must be 0.  acc[i] = the two
   16-bit sums of c = 2 below + on side by side, o[i] = the OR of c (bit 0 of a half: a read on the threshold). */
int miso_selftest_k2_count(const uint32_t *th, const int32_t *start, const uint32_t *u, const uint32_t *inv, const int32_t *masked,
                           int n, uint32_t *acc, uint32_t *o);
/* csrc/kernels_k2.inl k2_finish_lane, what a lane of the same loop does BEHIND it (the settle path, the finishing expression,
   the th = 0xFFFF rule and recount, the t = 2^32 closed form), with a caller-given threshold: element i is a chain on one lane
   with n_draw[i] (0 .. 2^20) drawing reads at iteration iter[i] of (seed, event_id[i], chain[i]); its sum and flag are made by
   k2_count.hpp's plain functions over its generator blocks.  out[i] = the number of its reads whose 32-bit uniform
   (include/miso_philox.h miso_split_word) is below t[i] (0 .. 2^32).  settle_all != 0: every lane rescans, as under
   MISO_K2_SETTLE_ALL. */
int miso_selftest_k2_finish(uint64_t seed, const uint32_t *event_id, const uint32_t *chain, const uint32_t *iter, const int32_t *n_draw,
                            const uint64_t *t, int settle_all, int n, int32_t *out);

#ifdef __cplusplus
}
#endif
#endif /* MISO_AMD_H */
