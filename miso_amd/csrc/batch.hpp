// batch.hpp -- the batch object behind miso_batch_t (definition shared by runtime.hip / launch.hip / capi.hip and the passes
// that are its methods or take batches).  What the batch owns on the device is its pools, tables, streams and the two events
// around its sampler kernels; a pass over the resident samples holds its buffers and events for the call only
// (hip_host.hpp HipCall, column_pass.hpp) and stores its results here when it has succeeded.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "device.hpp"
#include "hip_host.hpp"
#include "host.hpp"
#include "knobs.hpp"
#include "plan.hpp"

namespace miso {
int device_count();
void set_device(int d);
miso_batch *batch_new(const miso_params_t &p);
int choose_lanes_per_chain(long chains, int max_quads, int wave_slots, int max_cpw);
void selftest_detmath(const double *x, int n, double *e, double *l, double *s, double *q);
void selftest_philox(const uint32_t *in6, int n, uint32_t *out4);
// kernels_selftest.hip
void selftest_detmath_n(int fn, int width, const double *x, int n, int stride, double *out);
void selftest_detmath_routed(int fn, int force_full, const double *x, int n, double *out, int32_t *route);
void selftest_threshold(int routine, const double *c, const double *T, int n, uint64_t *out);
void selftest_count_below(const int32_t *D, const uint32_t *w4, const uint32_t *T, int n, int32_t *out);
void selftest_pe_pick(int KK, const uint8_t *f, const double *psi, const double *fp_rep, int il2, const uint32_t *rule_le,
                      const uint32_t *word, int n, int32_t *out);
void selftest_binomial(int G, uint64_t seed, uint32_t event_id, int32_t n, double p, int count, int32_t *out);
void selftest_binomial_law(int32_t n, double p, uint32_t stride, uint64_t *hist, uint64_t *info, float *kernel_ms);
void selftest_text_digits(const double *x, int n, int64_t *out);
void selftest_k2_flag(const uint32_t *m, const uint32_t *k, const int32_t *start, int n, int32_t *code, uint32_t *pos);
void selftest_k2_finish(uint64_t seed, const uint32_t *event_id, const uint32_t *chain, const uint32_t *iter, const int32_t *n_draw,
                        const uint64_t *t, int settle_all, int n, int32_t *out);
void selftest_k2_count(const uint32_t *th, const int32_t *start, const uint32_t *u, const uint32_t *inv, const int32_t *masked, int n,
                       uint32_t *acc, uint32_t *o);
// kernels_exact.hip: the exact-posterior mode's posterior stage on its own (miso_selftest_exact, exact summaries)
void exact_probe_run(const double *stats7, int n, const double *prob, int n_prob, double *out8, double *icdf, hipStream_t st = nullptr);
void exact_check_prob(const double *prob, int n_prob);   // MISO_EINVAL unless every probability lies inside (0, 1)
// kernels_exact_compare.hip: pairs of such posteriors compared (miso_batch_compare_exact, miso_selftest_exact_compare);
// out: 5 + n_z doubles per pair
void exact_compare_run(const double *stats7_1, const double *stats7_2, int n, const double *z, int n_z, double *out,
                       hipStream_t st = nullptr, float *ms = nullptr);
// The fence of both exact-posterior modes (DESIGN.md 15 "The fence"): a hyperparameter counts like reads of its isoform and is
// bounded like few of them; an effective length (paired: A) and the ratio of the two are bounded so that the mode stays within
// +-36.6 in logit space and no term of the log density rounds by more than the counts' own terms do.  Every comparison is
// false for a NaN, and the upper bounds refuse an infinity.
constexpr double EXACT_HYPER_MAX = 1048576.0;                       // 2^20
constexpr double EXACT_LEN_MAX = 1099511627776.0;                   // 2^40
constexpr double EXACT_LEN_MIN = 1.0 / 1099511627776.0;             // 2^-40
constexpr double EXACT_LEN_RATIO_MAX = 1048576.0;                   // 2^20
inline bool exact_fence(const double *len, const double *hyper) {
  for (int k = 0; k < 2; k++)
    if (!(hyper[k] >= 1 && hyper[k] <= EXACT_HYPER_MAX && len[k] >= EXACT_LEN_MIN && len[k] <= EXACT_LEN_MAX)) return false;
  return len[0] <= EXACT_LEN_RATIO_MAX * len[1] && len[1] <= EXACT_LEN_RATIO_MAX * len[0];
}
// the exact-posterior mode takes such an event (include/miso_amd.h miso_exact_eligible)
inline bool exact_eligible(bool paired, int K, const double *eff, const double *hyper) {
  return !paired && K == 2 && exact_fence(eff, hyper);
}
// kernels_exact_paired.hip: the paired-end exact-posterior mode (miso_batch_set_exact_paired).  Its posterior stage on its
// own: ka != null -- the events of ka's list, A2 their A0, A1 on the device (exact summaries); otherwise caller-given
// statistics and pairs (miso_selftest_exact_paired)
void exact_paired_probe_run(const KernelArgs *ka, const double *A2, const double *stats6, const double *m, const int64_t *offs,
                            int n, const double *prob, int n_prob, double *out8, double *icdf, hipStream_t st = nullptr);
const void *exact_paired_sample_fn();   // the kernel exact_paired_sample(KernelArgs, const double *A2, int S)
// sixteen pair factors, each at least the smallest fragment-length probability, must multiply to a normal number
constexpr double EXACT_PAIRED_MIN_PROB = 1.0 / 9223372036854775808.0;   // 2^-63
// the paired mode takes such an event (include/miso_amd.h miso_exact_paired_eligible); A = exp(assscores)
inline bool exact_paired_eligible(int K, const double *A, const double *hyper, bool any_bad) {
  return K == 2 && exact_fence(A, hyper) && !any_bad;
}
// n elements given by a caller: MISO_EINVAL unless every row of stats6 is eligible and -- offs != null: caller-given pairs --
// the offsets start at 0 and ascend and the probabilities m lie in [2^-63, 1]; returns the number of caller-given pairs
int64_t exact_paired_check(const double *stats6, const double *m, const int64_t *offs, int n);
// kernels_exact_paired_compare.hip: pairs of such posteriors compared (miso_batch_compare_exact_paired,
// miso_selftest_exact_paired_compare).  One sample's side of the n pairs, as the host driver takes it: stats6 (host) =
// {n10, n01, A0, A1, h0, h1} per pair, and the drawing pairs EITHER as caller-given probabilities m / offs (host, the
// selftest's layout) OR -- m == null -- as the records of a resident batch (device pointers), pair i being event list[i]
struct ExactPairedCmpInput {
  const double *stats6;
  const double *m; const int64_t *offs;
  const DevEvent *events; const unsigned char *in_pool; const double *frag_prob; int il;
};
// ... and as the kernel takes it (every pointer on the device)
struct ExactPairedCmpSide {
  const double *stats6;
  const double *mm; const int64_t *offs;
  const DevEvent *events; const unsigned char *in_pool; const double *frag_prob; int il;
};
// out: 5 + n_z doubles per pair, as exact_compare_run's
void exact_paired_compare_run(const ExactPairedCmpInput &in1, const ExactPairedCmpInput &in2, const int32_t *list, int n, const double *z,
                              int n_z, double *out, hipStream_t st = nullptr, float *ms = nullptr);
// kernels_exact_delta.hip, kernels_exact_paired_delta.hip: the quantiles of psi_1 - psi_2 of such pairs at the probabilities
// p[0 .. n_p) from the exact CDF (miso_batch_exact_delta_quantiles, miso_selftest_exact_delta_quantiles,
// miso_selftest_exact_paired_delta_quantiles); pairs and errors as the comparisons' drivers'.  out: n_p + 1 doubles per pair,
// the quantiles and then P(psi_1 - psi_2 <= 0)
void exact_delta_run(const double *stats7_1, const double *stats7_2, int n, const double *p, int n_p, double *out,
                     hipStream_t st = nullptr, float *ms = nullptr);
void exact_paired_delta_run(const ExactPairedCmpInput &in1, const ExactPairedCmpInput &in2, const int32_t *list, int n, const double *p,
                            int n_p, double *out, hipStream_t st = nullptr, float *ms = nullptr);
// kernels_exact_delta_groups.hip: the same quantiles between two groups of replicates, from the equal-weight mixture of the
// n1 n2 pairwise CDFs (miso_exact_delta_groups, miso_batch_exact_delta_groups).  Rows [event][replicate][7];
// take (may be null): per event, 0 = not to be compared; out: 2 + n_p + 1 + n_z doubles per event (m1, m2, q, H(0.0), H(z)),
// untouched and was_exact = 0 where the event is not comparable
void exact_delta_groups_run(const double *stats7_1, int n1, const double *stats7_2, int n2, int n_events, const unsigned char *take,
                            const double *p, int n_p, const double *z, int n_z, int max_events_per_launch, double *out,
                            int *was_exact, float *ms, hipStream_t st = nullptr);
void exact_delta_groups(miso_batch *const *g1, int n1, miso_batch *const *g2, int n2, const double *p, int n_p, const double *z, int n_z,
                        double *out, int64_t out_len, int *was_exact, float *kernel_ms);
// kernels_exact_paired_delta_groups.hip: the same for paired-end replicates (miso_exact_paired_delta_groups,
// miso_batch_exact_paired_delta_groups).  stats6, m, offs: n1 + n2 pointers, group 1's first, each replicate's
// elements in miso_selftest_exact_paired's layout over the same n_events; an event is comparable when every replicate's row
// is eligible for the paired exact mode.  out, was_exact: as above
void exact_paired_delta_groups_given(const double *const *stats6, const double *const *m, const int64_t *const *offs, int n1, int n2,
                                     int n_events, const double *p, int n_p, const double *z, int n_z, int max_events_per_launch,
                                     double *out, int *was_exact, float *ms);
void exact_paired_delta_groups(miso_batch *const *g1, int n1, miso_batch *const *g2, int n2, const double *p, int n_p, const double *z,
                               int n_z, double *out, int64_t out_len, int *was_exact, float *kernel_ms);
// kernels_compare_groups.hip
int compare_groups_staging(int n1, int n2, int S, size_t budget);
void compare_groups(miso_batch *const *g1, int n1, miso_batch *const *g2, int n2, double smoothing, int staging, double *out,
                    int64_t out_len, float *kernel_ms);
// kernels_compare_pairs_groups.hip
void compare_pairs_groups(miso_batch *const *g1, int n1, miso_batch *const *g2, int n2, double confidence_level, const double *tau,
                          int n_tau, bool as_text, uint64_t *out, int64_t out_len, int64_t *n_pairs, float *kernel_ms);
// kernels_groups.hip: isoform-group columns (miso_batch_summarize_isoform_groups, miso_batch_compare_pairs_isoform_groups;
// DESIGN.md 23).  Group g is (group_event[g], group_mask[g]); out: 3 doubles, or pairs_words(n_tau) words, per group
void summarize_isoform_groups(miso_batch &b, const int32_t *group_event, const uint64_t *group_mask, int64_t n_groups,
                              double confidence_level, bool as_text, double *out, int64_t out_len, float *kernel_ms);
void compare_pairs_isoform_groups(miso_batch &a, miso_batch &b, const int32_t *group_event, const uint64_t *group_mask,
                                  int64_t n_groups, double confidence_level, const double *tau, int n_tau, bool as_text,
                                  uint64_t *out, int64_t out_len, int64_t *n_pairs, float *kernel_ms);

// A device table and what it was last filled from: its host contents, or the key of the plan it was built for.  reset()
// frees the allocation and forgets both, so that neither outlives it (the next upload may be to another device).
template <class T> struct DevTable {
  T *d = nullptr;
  size_t cap = 0;                // elements allocated
  std::vector<T> host;           // what d holds (put, below)
  long key = -1;                 // the plan it was built for, -1 = none
  DevTable() = default;
  DevTable(const DevTable &) = delete;
  DevTable &operator=(const DevTable &) = delete;
  DevTable(DevTable &&o) noexcept : d(o.d), cap(o.cap), host(std::move(o.host)), key(o.key) { o.d = nullptr; o.cap = 0; o.key = -1; }
  void reset() {
    if (d) (void) hipFree(d);
    d = nullptr; cap = 0; host.clear(); key = -1;
  }
};
// `t` holds `v` from now on, in an allocation of at least `min_n` elements; copied only when it holds something else
template <class T> void put(DevTable<T> &t, const std::vector<T> &v, size_t min_n = 1) {
  const size_t n = std::max(v.size(), min_n);
  if (t.d && n <= t.cap && v.size() == t.host.size() && (v.empty() || std::memcmp(v.data(), t.host.data(), v.size() * sizeof(T)) == 0)) return;
  if (!t.d || n > t.cap) {
    if (t.d) HIP_OK(hipFree(t.d));
    t.d = nullptr; t.cap = 0;
    HIP_OK(hipMalloc(reinterpret_cast<void **>(&t.d), n * sizeof(T)));
    t.cap = n;
  }
  if (!v.empty()) HIP_OK(hipMemcpy(t.d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  t.host = v;
}
inline uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }
template <class K> const void *fn(K *k) { return reinterpret_cast<const void *>(k); }   // a kernel's host stub as hipLaunchKernel takes it
// chains on several workgroups (coop.hpp): which chain every workgroup works on, and the scratch they exchange through
struct CoopTable {
  DevTable<int32_t> tab;         // four words per workgroup
  DevTable<uint32_t> mem;        // COOP_WORDS per chain on more than one workgroup
  int chains = 0;                // chains on more than one workgroup
  void reset() { tab.reset(); mem.reset(); chains = 0; }
};
struct GrpShape { int qs = 0, ts = 0; };   // sampler_grp's slice: class thresholds (single-end), score table (paired-end)
// A sampler kernel's host stub and its name as last_kernels and miso_batch_launch_stats report it (launch.hip: made side by
// side, from the same template arguments)
struct Kernel { const void *fn; std::string name; };
// The kernel a general run is launched as.  The last six are a run's own kernels (launch.hip run_kernel: the one place that
// tells them apart); the first three are what the plan puts a run into instead (plan_runs, group_runs).
enum class RunKernel { LaneK, GrpAll, GrpMulti, GrpWide, GrpWave64, Big, Wave, Grp, Flat };
// ... and a half of the two-isoform list (plan_k2)
enum class K2Kernel { None, Lane, Multi, Mix, Single };
// paired-end size bucket of a general run, in the launch list's order (build_slots: largest first): genes of few pairs in a
// batch of several classes (eight lanes per chain); the class's normal launch; at least 32 lanes per chain (events several
// times the class's mean size); one chain per wavefront (sampler_grp<64, true, KC>); one chain per workgroup (sampler_grp<64,
// true, KC, true>)
enum class Bucket { Small = -1, Normal = 0, Lanes32 = 1, Wavefront = 2, Workgroup = 3 };
}  // namespace miso

// diagnose(): chains at most (three doubles of LDS per split sequence)
constexpr int DIAG_MAX_CHAINS = 2048;
// diagnose_rank(): used draws and chains at most (the column, its sorted copy and the per-sequence scratch stay in LDS:
// (8192 + 8192 + 3 * 1024) * 8 bytes = 152 KB of a workgroup's 160 KiB)
constexpr int RANK_MAX_DRAWS = 8192;
constexpr int RANK_MAX_CHAINS = 512;

struct miso_batch {
  miso_params_t p{};
  miso::Knobs knobs;                     // the MISO_* environment as resolve_pending() / upload() / launch() last found it (knobs.hpp)
  miso::FragmentDist fd;                 // paired only
  std::vector<miso::PackedEvent> events;
  std::vector<int64_t> event_ids;        // per event: explicit Philox event id, -1 = first_event_id + index
  // device
  int device = -1;
  bool uploaded = false, launched = false, downloaded = false;
  bool pool_cleared = false;      // the output pool has been zeroed since the upload
  bool launched_once = false;     // since the upload
  std::vector<int> coop_n;        // per event: workgroups of a workgroup-wide paired-end chain (upload: by its share of the batch's work)
  int coop_wgs_used = 0;          // cooperative workgroups handed out to this batch's wide runs (<= coop_gen_budget)
  int coop_gen_budget = 0;        // ... of the COOP_MAX_WGS a launch may hold in all; the two-isoform plans share the rest (launch())
  bool no_coop = false;           // set by sync() after a chain on several workgroups gave up: every chain on one workgroup from now on
  int coop_retries = 0;           // launches sync() had to repeat that way (miso_batch_coop_retries)
  uint64_t last_seed = 0;         // what the last launch() was called with (sync()'s re-run)
  uint32_t last_first_event_id = 0;
  // stop = CONVERGENT_MEAN (miso.c:903-925): sync() runs the events that have not converged again on the longer
  // schedule (runtime.hip converge_rounds) and puts the tail of their samples where the first round's were
  std::vector<int64_t> iters_counted;   // per event: iterations behind its accept count (empty: noIterations each)
  // a batch that runs a LATER round (made by converge_rounds): that round's own schedule, the reference's noIterations /
  // noBurnIn at that point (p holds the device's: everything from the chain's start), and the iterations at which the
  // rounds after the first open (KernelArgs::round_tab)
  int round_iters = 0, round_burn = 0;
  std::vector<int> round_starts;
  miso::DevTable<miso::GrpSeg> grp_segs;   // sampler_grp_all's segment table (KernelArgs::grp_segs)
  miso::DevTable<int32_t> round_tab;       // ... on the device (KernelArgs::round_tab)
  std::vector<char> went_on;      // per event: it ran a further round in the last launch's converge_rounds
  bool event_went_on(int i) const { return i < static_cast<int>(went_on.size()) && went_on[i] != 0; }
  int rounds = 1;                 // rounds the last launch took (1 = the events' own schedule sufficed)
  int prio_lo = 0, prio_hi = 0;   // the device's stream priority range as this batch uses it (equal: priorities off)
  bool converged_done = false;    // stop = CONVERGENT_MEAN: this launch's further rounds have run (sync() is idempotent; launch() clears it)
  void converge_rounds(float *ms);
  bool coop_enabled() const;      // chains may use several workgroups (coop.hpp): not after a time-out, not with knobs.no_coop
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // the shader clock of a launch (miso_batch_set_clock_probe; launch.hip clock_probe_kernel)
  bool clock_probe = false, probe_armed = false, probe_failed = false;
  hipStream_t probe_stream = nullptr;
  unsigned long long *d_probe = nullptr;   // {t0 real, t0 cycles, t1 real, t1 cycles, gave up, -, -, flag}
  uint32_t probe_gen = 0;                  // the flag's value that ends the current launch's probe
  double wall_khz = 100000.0;              // hipDeviceAttributeWallClockRate
  double last_clock_ghz = 0.0, last_probe_ms = 0.0;   // 0: no probe, or its window did not cover the launch
  void start_clock_probe();
  void read_clock_probe();
  std::vector<hipStream_t> aux_streams;   // kernels 2.. of a mixed batch run beside the first
  std::vector<hipEvent_t> aux_done;
  miso::DevEvent *d_events = nullptr;
  unsigned char *d_in = nullptr, *d_out = nullptr;
  double *d_fp = nullptr;
  int32_t *d_slots = nullptr;     // [k2 events sorted by n_draw desc | all other events]
  std::vector<int32_t> h_slots;   // the same list on the host
  bool k2_general = false;        // paired-end, tables too wide for the two-isoform kernel's LDS: K = 2 events take sampler_grp
  bool use_delta = true;          // paired-end: MODE 2 events first in the list (fixed at upload)
  miso::DevTable<double> logfact; // collapsed: log factorials up to the largest event's drawing reads
  int collapsed_level = 0;        // 1: two-isoform events; 2: also the events with more isoforms (sampler_lane_k)
  bool collapsed = false;         // single-end two-isoform events: the collapsed Gibbs step (kernels_lane.hip); miso_batch_set_collapsed
  // the exact-posterior mode (miso_batch_set_exact; kernels_exact.hip): its events leave the sampler's lists
  bool exact = false;
  bool exact_paired = false;      // ... of paired-end batches (miso_batch_set_exact_paired; kernels_exact_paired.hip): the same lists,
                                  // exact_eff holds A0, A1 (a batch is single-end or paired-end: at most one of the two is set)
  bool exact_any() const { return exact || exact_paired; }
  bool slots_exact = false;       // the mode the launch lists were last built for (build_slots)
  std::vector<char> is_exact;     // per event: the exact kernel takes it
  int n_exact = 0;                // ... their number: the launch lists are [two-isoform | other | exact]
  miso::DevTable<double> exact_eff;   // e0, e1 of every event of the exact list
  std::vector<double> exact_sums; // exact_summaries(): per event of the exact list {mean, ci_low, ci_high} x 2 isoforms
  double exact_sums_level = -1.0; // ... the confidence level they were made for
  bool event_exact(int i) const { return i >= 0 && i < static_cast<int>(is_exact.size()) && is_exact[i] != 0; }
  void build_slots();
  void launch_exact(const miso::KernelArgs &a);
  void exact_summaries(double confidence_level);
  void exact_stats7(int event, double *r) const;   // {n10, n01, n, e0, e1, h0, h1} of an event of the exact list
  // miso_batch_compare_exact (this batch is sample 1): per event 5 + exact_cmp_nz doubles, and whether the pair was comparable
  std::vector<double> h_exact_cmp;
  std::vector<char> exact_cmp_ok;
  int exact_cmp_nz = 0;
  bool exact_compared = false;
  float compare_ms = 0.f, exact_compare_ms = 0.f;   // kernel time of the last compare / compare_exact or compare_exact_paired
  void compare_exact(miso_batch &other, const double *z, int n_z);
  void compare_exact_paired(miso_batch &other, const double *z, int n_z);   // miso_batch_compare_exact_paired: the same stores
  // miso_batch_exact_delta_quantiles, of the pairs the stored exact comparison found comparable: per event exact_delta_np + 1
  // doubles (the quantiles, then the CDF at 0).  The next exact comparison discards them.
  std::vector<double> h_exact_delta;
  int exact_delta_np = 0;
  bool exact_delta_done = false;
  float exact_delta_ms = 0.f;   // kernel time of the last such launch
  void exact_delta_quantiles(miso_batch &other, const double *p, int n_p);
  int n_k2 = 0, n_gen = 0;
  int n_k2w = 0;                  // paired-end: the first n_k2w two-isoform slots take sampler_k2's MODE 2
  // A half of the two-isoform list: k2[0] the paired-end MODE 2 events (no drawing read on a non-finite score), k2[1] the
  // others (MODE 1; single-end: everything, MODE 0).  The slots and the mode are build_slots'; the lane plan, its key and the
  // cooperative table are kept between launches; the rest is what the last launch() decided (plan_sizes, plan_k2).
  struct K2Half {
    int mode = 0;                 // sampler_k2's MODE
    int first = 0, count = 0;     // slots [first, first + count) of d_slots
    miso::K2Kernel kind = miso::K2Kernel::None;
    int G = 0;                    // lanes per chain of the single-width launch (Mix: of its narrow part)
    size_t fp = 0, tab = 0;       // LDS: the fragment-length probabilities, a chain's score table
    miso::LanePlan plan;          // sampler_k2_multi: the runs of equal lanes per chain, valid for plan_key
    long plan_key = -1;
    miso::CoopTable coop;         // the plan's chains on several workgroups (key: the plan's wide run)
  } k2[2];
  bool k2_mode2(const miso::PackedEvent &e) const { return use_delta && e.pe_delta && !e.draw_dense.empty(); }   // k2[0] takes it
  // the other events, grouped by isoform-count class (sampler_grp<G, PE, KC> holds K in (KC_prev, KC])
  struct GenRun {
    int first = 0, count = 0;     // slice of d_slots (after the n_k2 two-isoform events)
    int kc = 4;                   // 4, 8, 12, 16 or 32
    int kmax = 2, kmin = 64, maxq = 1;   // most / fewest isoforms, most draw quads
    double sum_q = 0;             // draw quads of all its events (their mean decides the lanes per chain in a batch of several classes)
    int maxcls = 0;               // most drawing-read classes (single-end)
    bool nocls = false;           // some single-end event has no class table (> MAX_DRAW_CLASSES classes)
    bool dense = true;            // paired-end: every event has dense quad records (pe_dense)
    miso::Bucket bucket = miso::Bucket::Normal;   // paired-end size bucket (runtime.hip build_slots)
    bool small() const { return bucket == miso::Bucket::Small; }
    bool wave64() const { return bucket == miso::Bucket::Wavefront; }
    bool wide() const { return bucket == miso::Bucket::Workgroup; }
    int force_G() const { return bucket == miso::Bucket::Lanes32 ? 32 : (wave64() ? 64 : 0); }   // at least this many lanes per chain
    // wide runs: which chain every workgroup works on, alone or as one of several (coop.hpp; launch.hip wide_setup)
    miso::CoopTable coop;
    int tuned_G = 0;              // lanes per chain picked by the first launch's trial runs
    int tuned_flat = -1;          // sampler_flat (1) or sampler_grp (0) by the first launch's trial runs, -1 = not tried
    // sampler_flat: which chains every wavefront owns (launch.hip flat_waves; two words per wavefront)
    miso::DevTable<int32_t> wave_tab;
    int wave_nc = 0;              // most chains of any wavefront = slices per wavefront in LDS
    int wave_wide = 0;            // chains that own a whole workgroup
    bool wave_packed = false;     // wavefronts packed by work units (events of very different sizes)
  };
  std::vector<GenRun> gen_runs;
  int tuned_k2_G = 0;             // ditto for the two-isoform kernel
  // device_match: events whose compatibility is still to be computed (kernels_match.hip)
  struct Pending {
    int event = 0;               // index into `events` (a placeholder until resolved)
    miso::Gene gene;
    std::vector<int> pos;
    miso::CigarTable ct;
    std::vector<double> hyper;   // empty = all ones
  };
  std::vector<Pending> pending;
  float match_ms = 0.f;          // kernel time of the last resolve
  // tests (want_counts_trace): the kernel's raw outputs, per resolved event
  std::vector<std::vector<uint64_t>> kept_masks;   // single-end: N masks
  std::vector<std::vector<uint16_t>> kept_frags;   // paired-end: N x K fragment indices
  void resolve_pending();        // runs match_kernel for all pending events, packs them
  int lanes_per_chain = 0;        // G of the last sampler_k2 launch (0 = none)
  std::string last_kernels;       // names of the kernels the last launch started, in launch order, comma separated
  // sampler_k2_multi<0, 8>, one round: the launch's wavefronts paired by estimated duration across the runs (runtime.hip)
  miso::DevTable<int32_t> k2_pair_tab;
  int k2_pair_wide_blocks = 0, k2_pair_grid = 0;
  // What launch() decided, kept until the next launch: the launches follow it, launch_stats() reads it (launch.hip)
  struct LaunchPlan {
    bool sampled = false;         // the kernels below ran (not MARGINAL / CLASSES, not adopted samples)
    // this launch's sizes and switches (plan_sizes)
    size_t lds_max = 0;           // a workgroup's LDS budget
    size_t fp_plain = 0;
    bool dense_env = true;
    int il2 = 0;
    long total_chains = 0;
    size_t n_kernels = 0;
    bool tune_runs = false;
    int coop_max = 1;
    // the two-isoform part (plan_k2; the halves' own figures are in k2[])
    bool k2_pair = false;         // single-end sampler_k2<G, 0, 8>
    int k2_mix = 0, k2_mix_blocks = 0;                 // sampler_k2_mix: events of the wide part, its workgroups
    bool k2_narrow = false;       // sampler_k2_multi<0, 4, true>
    bool lane_route = false, lane_ilp = false;         // collapsed: sampler_lane, sampler_lane_ilp or sampler_k2c<lane_G>
    int lane_G = 1;
    // the general runs, one per gen_runs entry (plan_runs, group_runs)
    struct Run {
      miso::RunKernel kind = miso::RunKernel::Grp;     // the kernel it is launched as
      miso::RunKernel layout = miso::RunKernel::Grp;   // ... and, inside a launch of several runs, the run's own kernel: how its wavefronts are cut
      bool lane() const { return kind == miso::RunKernel::LaneK; }
      bool grouped() const { return kind == miso::RunKernel::GrpAll || kind == miso::RunKernel::GrpMulti; }
      int flat_nc = 0, flat_nc_max = 0;   // sampler_flat's chains per wavefront (0: not sampler_flat)
      int flat_ks = 0;            // ... its compile-time isoform count (0: the layout at run time)
      bool flat_uni = false;      // ... every event of the run has flat_ks isoforms
      int G = 64;                 // sampler_grp's lanes per chain
      miso::GrpShape sh;
      bool merge_next = false;    // one launch with the next run
    };
    std::vector<Run> runs;
    bool lane_gen = false;        // some run takes sampler_lane_k
    bool grp_all = false;         // every run in one sampler_grp_all
    std::vector<std::pair<size_t, size_t>> multi;      // runs [r0, r1) of a class in one sampler_grp_multi
  } plan;
  size_t kernel_no = 0;           // kernels of the launch so far (stream_for_next)
  int wave_slots = 2048;          // resident sampler_k2 wavefronts on the device
  std::vector<miso::DevEvent> h_events;
  std::vector<unsigned char> h_out;
  std::vector<double> h_summary;        // per event: K x {mean, ci_low, ci_high}
  std::vector<uint64_t> h_sum_off;      // offsets (in doubles) into h_summary
  bool summarized = false;
  std::vector<double> h_compare;        // per event: K x {mean1, mean2, bayes factor, posterior density at 0}
  std::vector<uint64_t> h_cmp_off;      // offsets (in doubles) into h_compare
  bool compared = false;
  std::vector<double> h_diag;           // per event: K x {rhat, ess, mcse, lag} (kernels_diagnose.hip)
  std::vector<uint64_t> h_diag_off;     // offsets (in doubles) into h_diag
  bool diagnosed = false;
  std::vector<double> h_rank;           // per event: K x {rhat_bulk, rhat_fold, ess_bulk, ess_ci_low, ess_ci_high, distinct}
  std::vector<uint64_t> h_rank_off;     // (kernels_diagnose_rank.hip) and the offsets (in doubles) into it
  bool rank_diagnosed = false;
  float summarize_ms = 0.f, diagnose_ms = 0.f;   // kernel time of the last summarize / diagnose pass
  float rank_ms = 0.f;                  // and of the last diagnose_rank pass (each timed by its own HipCall's events)
  // the posterior predictive model check (miso_batch_set_model_check; kernels_model_check.hip): per event
  // added with a gene its class table (pattern, m); the observed counts are read from the event's own read classes when
  // asked for (fit_counts), so that an event matched on the device has them once it is resolved
  bool model_check_on = false;
  struct FitTable { int status = MISO_FIT_NO_GENE; std::vector<uint64_t> pattern; std::vector<int64_t> m; };
  std::vector<FitTable> fit_tables;     // one per event while the switch is on (an event beyond it: no gene)
  const FitTable &fit_table(int i) const { static const FitTable none; return i < static_cast<int>(fit_tables.size()) ? fit_tables[i] : none; }
  void fit_add(const miso::Gene *g);    // the table of the event added last (null: added without a gene)
  void fit_counts(int i, std::vector<int32_t> &n, int64_t *n_reads, int64_t *n_off) const;
  struct FitResults {                   // per event, per class at class_off[i] + c
    std::vector<int64_t> class_off;
    std::vector<int32_t> status, rows, bad_rows, exceed, ge, le;
    std::vector<double> sum_obs, sum_rep, expected;
  } fit;
  bool model_checked = false;
  float model_check_ms = 0.f;
  void model_check(uint64_t seed);
  bool adopted = false;                 // samples produced elsewhere (adopt_pool): p.noChains says nothing about them
  uint64_t in_bytes = 0, out_bytes = 0;
  float last_ms = 0.f;

  int k2_first_event() const {  // the k2 event with the most drawing reads (list is sorted)
    int best = -1;
    for (size_t i = 0; i < events.size(); i++)
      if (events[i].K == 2 && !k2_general && !event_exact(static_cast<int>(i)) && (best < 0 || events[i].n_draw > events[best].n_draw))
        best = static_cast<int>(i);
    return best;
  }
  int S() const { return p.noChains * (p.noIterations - p.noBurnIn) / p.noLag; }
  ~miso_batch() { release(); }
  void release();
  void upload(int dev);
  void launch(uint64_t seed, uint32_t first_event_id);
  void sync(float *ms);
  void download();
  void summarize(double confidence_level, bool as_text = false);
  void diagnose(int noChains);
  void diagnose_rank(int noChains, double confidence_level);
  void adopt_samples(int n, const int *K, int S, const double *const *samples, int dev);
  void adopt_pool(int n, const int *K, int S, int dev);
  // kernels_text.hip: the pool filled from `.miso` sample text by text_decode_kernel
  void adopt_text(int n, const unsigned char *text, const int64_t *offsets, const int *K, int S, int dev, int64_t chunk_bytes,
                  int32_t *status, miso_text_stats_t *stats);
  void compare(miso_batch &other, double smoothing);
  // miso_batch_compare_pairs (this batch is sample 1; kernels_compare_pairs.hip): per (event, isoform) column
  // pairs_words(pairs_ntau) 64-bit words (compare_pairs.hpp), event i's first column at h_pairs_off[i]
  std::vector<uint64_t> h_pairs, h_pairs_off;
  int pairs_ntau = 0;
  int64_t pairs_M = 0;                  // S1 * S2
  bool pairs_compared = false;
  float pairs_ms = 0.f;                 // kernel time of the last compare_pairs
  std::vector<int32_t> text_status;     // adopt_text: per event, non-zero = its text was not decoded, its pool region holds no samples
  bool event_unread(int i) const { return i < static_cast<int>(text_status.size()) && text_status[i] != 0; }
  void compare_pairs(miso_batch &other, double confidence_level, const double *tau, int n_tau, bool as_text = false);
  std::vector<miso_kernel_stat_t> launch_stats() const;   // miso_batch_launch_stats: one record per two-isoform part and per run

  // the parts of launch(): the plan (runtime.hip), the launches that follow it (launch.hip)
  void plan_sizes();
  void plan_k2(const miso::KernelArgs &a);
  // a part of the two-isoform list as plan_lanes takes it: slots [first, first + count), the lanes per chain a run may have,
  // the wavefronts of a workgroup-wide chain's and of the other workgroups, the workgroups resident at once, the chains per
  // wavefront the LDS allows, the part's share of the cooperative workgroups
  struct K2Part { int first, count; const int *widths; int n_widths; int wide_wpb = 0, wpb = 0, resident = 1, max_cpw = 64, coop_budget = 0; };
  miso::LanePlan k2_lanes(const K2Part &pt, const std::vector<int> &nd, const miso::LaneCost &cost) const;
  bool plan_k2_lanes(const K2Part &pt, bool forced, miso::LaneCost &cost, std::vector<int> &nd, K2Half &h);
  void k2_pair_table(const std::vector<int> &nd, const miso::LaneCost &cost);
  void plan_runs(const miso::KernelArgs &a);
  int flat_wgs(int kc) const;
  void plan_flat(size_t ri);
  void plan_grp(size_t ri, const miso::KernelArgs &a);
  void group_runs();
  void launch_planned(const miso::KernelArgs &a, const miso::KernelArgs &k2a);
  template <class F> int fastest(const miso::KernelArgs &a, const std::vector<int> &cand, F &&trial);
  int slots_for(long chains) const;
  hipStream_t stream_for_next();
  // launch.hip: every sampler launch goes through launch_kernel, which also records the kernel's name -- unless it is a
  // trial launch (fastest)
  bool trial_launch = false;
  void note_kernel(const std::string &name) { last_kernels += (last_kernels.empty() ? "" : ",") + name; }
  // ... a pass over the launch's samples, named once however often it is called (a whole name: compare_pairs is not
  // compare_pairs_groups_iso)
  void note_pass(const std::string &name) {
    if (("," + last_kernels + ",").find("," + name + ",") == std::string::npos) note_kernel(name);
  }
  void launch_kernel(const miso::Kernel &k, unsigned grid, unsigned block, size_t lds, hipStream_t st, void **args);
  void launch_kernel(const miso::Kernel &k, unsigned grid, unsigned block, size_t lds, hipStream_t st, const miso::KernelArgs &ka);
  static miso::RunKernel run_kernel(const GenRun &run, int G, bool flat, bool dense_env, bool paired);
  miso::Kernel k2_kernel_of(const K2Half &h) const;
  miso::Kernel run_kernel_of(miso::RunKernel kind, int kc, const LaunchPlan::Run &r) const;
  void launch_marginal(const miso::KernelArgs &a);
  int fp_rows(const GenRun &run) const;
  size_t fp_bytes_of(const GenRun &run) const;
  miso::GrpShape grp_shape(const GenRun &run) const;
  bool grp_fits(const GenRun &run, const miso::GrpShape &sh, int G) const;
  GenRun joined_run(size_t r0, size_t r1) const;
  void launch_k2(miso::KernelArgs ka, const K2Half &h, int G, hipStream_t st);
  void launch_k2_mix(miso::KernelArgs ka, hipStream_t st);
  void k2_coop(miso::KernelArgs &ka, K2Half &h, hipStream_t st);
  void launch_k2_multi(miso::KernelArgs ka, K2Half &h, hipStream_t st);
  void launch_lane(miso::KernelArgs ka, hipStream_t st);
  unsigned wide_setup(GenRun &run, long chains, hipStream_t st);
  void launch_grp(miso::KernelArgs ka, GenRun &run, const miso::GrpShape &sh, int G, hipStream_t st);
  void flat_waves(GenRun &run, int nc, int nc_max_u, long resident_u, int nc_max_p, long resident_p);
  void launch_flat(miso::KernelArgs ka, size_t ri, hipStream_t st);
  void launch_run(const miso::KernelArgs &a, size_t ri);
  void launch_grp_all(const miso::KernelArgs &a);
  void launch_grp_multi(const miso::KernelArgs &a, size_t r0, size_t r1);
  template <class F> void each_coop_table(F &&f) { for (GenRun &r : gen_runs) f(r.coop); f(k2[0].coop); f(k2[1].coop); }
  template <class F> void each_table(F &&f) {   // every device table above (release())
    f(grp_segs); f(round_tab); f(logfact); f(k2_pair_tab); f(exact_eff);
    for (GenRun &r : gen_runs) f(r.wave_tab);
    each_coop_table(f);
  }
};

// runtime.hip: an event's row {n10, n01, A0, A1, h0, h1} as the paired exact passes take it, and a launched paired-end batch's
// side of such a pass (its resident pair records; stats6: the rows of the pass's events, on the host)
void exact_paired_stats6(const miso_batch &b, int i, double *row);
miso::ExactPairedCmpInput exact_paired_resident(const miso_batch &b, const double *stats6);
