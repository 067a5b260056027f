// kernels_groups.hip -- part-level psi: isoform-group columns of the resident sample pool: kernels and host
// drivers of miso_batch_summarize_isoform_groups and miso_batch_compare_pairs_isoform_groups (include/miso_amd.h).
//
// A group is (event, mask), the mask a set of the event's isoforms; its draw of pool row s is
//   v_s = ((0.0 + psi[s][k1]) + psi[s][k2]) + ...   over the mask's k ascending, plain IEEE adds,
// the inclusion of a part (an exon) that exactly the mask's isoforms contain.  Every other pass reduces one (event, isoform)
// column as it lies in the pool; these form the column first.  No reference counterpart (its users add up posterior means
// and have no interval).
//
// One 256-thread workgroup per group.  The column is derived from the pool rows into dynamic LDS as order_keys (thread t
// rows t, t + 256, ...: a row's members are neighbours in memory), the mean comes from the values as they are derived --
// summarize_kernel's order: 256 strided partial sums folded in halves --, the column is sorted by pairs_sort and the order
// statistics are two LDS reads.  The comparison derives both samples' columns and goes on as compare_pairs_kernel does after
// its two sorts (compare_pairs_device.hpp pairs_statistics): a group of one isoform gives that kernel's bits.
// Dynamic LDS: S * 8 bytes, (S1 + S2) * 8 for the comparison -- 128 KB of a workgroup's 160 KB at the limit of 8192 draws.
// Plain C++, f64 additions, subtractions and comparisons only, no atomics; every barrier in workgroup-uniform control flow.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "batch.hpp"
#include "column_pass.hpp"
#include "compare_pairs.hpp"
#include "compare_pairs_device.hpp"
#include "order_key.hpp"
#include "text_digits.hpp"

namespace miso {

// A group as the kernels get it: the event's index, PAIRS_SKIP_EVENT set when its samples were never decoded; the mask
struct DevGroup {
  uint64_t event;
  uint64_t mask;
};

// The group's column over the S rows at x (K values a row) into keys[0 .. S) as order_keys; `acc` takes this thread's
// values in the order it meets them (rows t, t + 256, ...).  Returns whether this thread met a NaN or an infinity.
// as_text: a member as its `.miso` file prints it and a reader parses it back (text_digits.hpp), as compare_pairs_kernel.
__device__ __forceinline__ int group_column(const double *x, int K, int S, uint64_t mask, int as_text, uint64_t *keys, double &acc) {
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  int bad = 0;
  for (int s = threadIdx.x; s < S; s += 256) {
    const double *row = x + static_cast<size_t>(s) * K;
    double v = 0.0;
    for (uint64_t m = mask; m; m &= m - 1) {
      double c = row[__builtin_ctzll(m)];
      if (as_text && text_rounds(c)) c = static_cast<double>(text_digits(c)) / 10000.0;
      v = v + c;
    }
    v = v + 0.0;
    bad |= !(fabs(v) < inf);
    acc = acc + v;
    keys[s] = order_key(v);
  }
  return bad;
}

// Grid (groups of this launch); out: mean, ci_low, ci_high per group.  The host refuses S outside the strict ranks' range
// and above PAIRS_MAX_DRAWS, checks every mask against its event and sizes the dynamic LDS: S * 8 bytes.
__global__ __launch_bounds__(256) void summarize_groups_kernel(const DevEvent *events, const unsigned char *pool, int S, int rank_lo,
                                                               int rank_hi, int as_text, const DevGroup *groups, int n_groups,
                                                               double *out) {
  extern __shared__ uint64_t groups_lds[];
  __shared__ double part[256];
  const int g = blockIdx.x, t = threadIdx.x;
  if (g >= n_groups) return;
  const DevGroup G = groups[g];
  double *o = out + 3 * static_cast<size_t>(g);
  const bool skip = (G.event & PAIRS_SKIP_EVENT) != 0;   // (the event's samples were never decoded: nothing of it is read)
  double acc = 0.0;
  int bad = 1;
  if (!skip) {
    const DevEvent E = events[G.event];
    bad = group_column(reinterpret_cast<const double *>(pool + E.off_samples), E.K, S, G.mask, as_text, groups_lds, acc);
  }
  part[t] = acc;
  if (__syncthreads_or(bad)) {                          // workgroup-uniform (a skipped event: bad in every thread)
    if (t == 0) {
      const double nan = __longlong_as_double(0x7FF8000000000000ll);
      o[0] = nan; o[1] = nan; o[2] = nan;
    }
    return;
  }
  for (int stride = 128; stride >= 1; stride >>= 1) {
    if (t < stride) part[t] = part[t] + part[t + stride];
    __syncthreads();
  }
  pairs_sort(groups_lds, S);
  if (t == 0) {
    o[0] = part[0] / static_cast<double>(S);
    o[1] = key_value(groups_lds[rank_lo]);
    o[2] = key_value(groups_lds[rank_hi]);
  }
}

// Grid (groups of this launch); out: pairs_words(pa.n_tau) words per group.  The host refuses S1, S2 outside
// [1, PAIRS_MAX_DRAWS] and sizes the dynamic LDS: (S1 + S2) * 8 bytes.
__global__ __launch_bounds__(256) void compare_pairs_groups_iso_kernel(const DevEvent *events1, const unsigned char *pool1, int S1,
                                                                       const DevEvent *events2, const unsigned char *pool2, int S2,
                                                                       PairsArgs pa, int as_text, const DevGroup *groups,
                                                                       int n_groups, uint64_t *out) {
  extern __shared__ uint64_t groups_lds[];
  __shared__ PairsScratch sc;
  const int g = blockIdx.x, t = threadIdx.x;
  if (g >= n_groups) return;
  const DevGroup G = groups[g];
  uint64_t *o = out + static_cast<size_t>(g) * (PAIRS_FIXED_WORDS + pa.n_tau);
  const bool skip = (G.event & PAIRS_SKIP_EVENT) != 0;
  uint64_t *KA = groups_lds, *KB = KA + S1;
  int bad = 1;
  if (!skip) {
    const DevEvent E1 = events1[G.event], E2 = events2[G.event];
    double unused = 0.0;
    bad = group_column(reinterpret_cast<const double *>(pool1 + E1.off_samples), E1.K, S1, G.mask, as_text, KA, unused);
    bad |= group_column(reinterpret_cast<const double *>(pool2 + E2.off_samples), E2.K, S2, G.mask, as_text, KB, unused);
  }
  if (__syncthreads_or(bad)) {                          // workgroup-uniform
    if (t == 0) pairs_not_finite(o, pa.n_tau);
    return;
  }
  pairs_sort(KA, S1);
  pairs_sort(KB, S2);
  double *A = reinterpret_cast<double *>(KA), *B = reinterpret_cast<double *>(KB);
  for (int e = t; e < S1; e += 256) A[e] = key_value(KA[e]);   // (each thread its own words, in place)
  for (int e = t; e < S2; e += 256) B[e] = key_value(KB[e]);
  __syncthreads();
  pairs_statistics(A, S1, B, S2, pa, o, sc);
}

// The result buffer of one launch, bytes at most: a call is split over group ranges, so that what it holds on the device
// does not grow with its groups
constexpr size_t GROUPS_RESULT_BYTES = size_t{256} << 20;

// The groups as the kernels take them, every one checked against its event in `b` (and, `other` given, flagged when either
// batch never decoded the event).  Whatever is refused is refused here, before anything is allocated.
static std::vector<DevGroup> checked_groups(const miso_batch &b, const miso_batch *other, const int32_t *group_event,
                                            const uint64_t *group_mask, int64_t n_groups) {
  if (n_groups < 0) MISO_FAIL(MISO_EINVAL, "Invalid number of isoform groups");
  if (n_groups > 0 && (!group_event || !group_mask)) MISO_FAIL(MISO_EINVAL, "group_event or group_mask is NULL");
  const int64_t n = static_cast<int64_t>(b.events.size());
  std::vector<DevGroup> gs(static_cast<size_t>(n_groups));
  for (int64_t g = 0; g < n_groups; g++) {
    const std::string who = "group " + std::to_string(g) + ": ";
    const int64_t e = group_event[g];
    if (e < 0 || e >= n) MISO_FAIL(MISO_EINVAL, who + "event index " + std::to_string(e) + " outside the batch");
    const int K = b.events[e].K;
    if (K > 64) MISO_FAIL(MISO_EINVAL, who + "event " + std::to_string(e) + " has " + std::to_string(K) + " isoforms, a mask holds 64 at most");
    const uint64_t mask = group_mask[g];
    if (mask == 0) MISO_FAIL(MISO_EINVAL, who + "empty isoform mask");
    if (K < 64 && (mask >> K) != 0) MISO_FAIL(MISO_EINVAL, who + "the mask names an isoform at or above the event's " + std::to_string(K));
    const int i = static_cast<int>(e);
    const bool skip = b.event_unread(i) || (other && other->event_unread(i));
    gs[g] = {static_cast<uint64_t>(e) | (skip ? PAIRS_SKIP_EVENT : 0), mask};
  }
  return gs;
}

static void check_out(const void *out, int64_t out_len, uint64_t need, const char *what) {
  if (out_len < 0 || static_cast<uint64_t>(out_len) < need) MISO_FAIL(MISO_EINVAL, std::string("out is too short for ") + what + " per group");
  if (need && !out) MISO_FAIL(MISO_EINVAL, "out is NULL");
}

// The groups range by range, `w` result values of type T a group: launch(call, d_groups, count, d_res) starts the kernel.
// Returns the launches' time.
template <class T, class Launch>
static float group_ranges(hipStream_t stream, const void *kernel, size_t dyn, const std::vector<DevGroup> &gs, size_t w, T *out,
                          Launch &&launch) {
  const size_t per_range = std::max<size_t>(1, GROUPS_RESULT_BYTES / (w * sizeof(T)));
  const std::vector<uint64_t> no_offsets(1, 0);         // (column_pass's offset table: the groups carry their own places)
  float ms = 0.f;
  for (size_t g0 = 0; g0 < gs.size(); g0 += per_range) {
    const size_t count = std::min(per_range, gs.size() - g0);
    HipCall call(stream);
    const DevGroup *d_groups = call.upload(gs.data() + g0, count * sizeof(DevGroup));
    ms += column_pass(call, kernel, dim3(static_cast<unsigned>(count)), dyn, no_offsets, count * w, out + g0 * w,
                      [&](dim3 grid, const uint64_t *, T *d_res) { launch(call, grid, d_groups, static_cast<int>(count), d_res); });
  }
  return ms;
}

void summarize_isoform_groups(miso_batch &b, const int32_t *group_event, const uint64_t *group_mask, int64_t n_groups,
                              double confidence_level, bool as_text, double *out, int64_t out_len, float *kernel_ms) {
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device: the group summary has no CPU path");
  if (!b.launched) MISO_FAIL(MISO_EINVAL, "batch not launched");
  const int S = b.S();
  const CiRanks r = ci_ranks_strict(S, confidence_level);
  if (S > PAIRS_MAX_DRAWS) MISO_FAIL(MISO_EINVAL, "Too many samples for the isoform-group summary: 8192 per event at most");
  const std::vector<DevGroup> gs = checked_groups(b, nullptr, group_event, group_mask, n_groups);
  check_out(out, out_len, 3 * static_cast<uint64_t>(gs.size()), "3 doubles");
  if (kernel_ms) *kernel_ms = 0.f;
  if (gs.empty()) return;
  finish_rounds(b);
  HIP_OK(hipSetDevice(b.device));
  const int lo = static_cast<int>(r.lo), hi = static_cast<int>(r.hi);
  const size_t dyn = static_cast<size_t>(S) * sizeof(uint64_t);
  const float ms = group_ranges(b.stream, fn(summarize_groups_kernel), dyn, gs, 3, out,
                                [&](HipCall &call, dim3 grid, const DevGroup *d_groups, int count, double *d_res) {
                                  hipLaunchKernelGGL(summarize_groups_kernel, grid, dim3(256), dyn, call.st, b.d_events, b.d_out, S, lo,
                                                     hi, as_text ? 1 : 0, d_groups, count, d_res);
                                });
  b.note_pass("summarize_groups");
  if (kernel_ms) *kernel_ms = ms;
}

void compare_pairs_isoform_groups(miso_batch &a, miso_batch &b, const int32_t *group_event, const uint64_t *group_mask,
                                  int64_t n_groups, double confidence_level, const double *tau, int n_tau, bool as_text,
                                  uint64_t *out, int64_t out_len, int64_t *n_pairs, float *kernel_ms) {
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device: the comparison has no CPU path");
  same_events(a, b, false);
  const int S1 = a.S(), S2 = b.S();
  if (S1 < 1 || S2 < 1) MISO_FAIL(MISO_EINVAL, "Too few samples to compare");
  if (S1 > PAIRS_MAX_DRAWS || S2 > PAIRS_MAX_DRAWS)
    MISO_FAIL(MISO_EINVAL, "Too many samples for the all-pairs comparison: 8192 per event and sample at most");
  const int64_t M = static_cast<int64_t>(S1) * S2;
  const PairsArgs pa = pairs_args(M, confidence_level, tau, n_tau);
  const std::vector<DevGroup> gs = checked_groups(a, &b, group_event, group_mask, n_groups);
  const size_t W = static_cast<size_t>(pairs_words(n_tau));
  check_out(out, out_len, W * gs.size(), "pairs_words(n_tau) words");
  if (n_pairs) *n_pairs = M;
  if (kernel_ms) *kernel_ms = 0.f;
  if (gs.empty()) return;
  finish_rounds(a);
  finish_rounds(b);
  HIP_OK(hipSetDevice(a.device));
  HIP_OK(hipStreamSynchronize(b.stream));
  const size_t dyn = (static_cast<size_t>(S1) + S2) * sizeof(uint64_t);   // both columns: what is live, not the limit
  const float ms = group_ranges(a.stream, fn(compare_pairs_groups_iso_kernel), dyn, gs, W, out,
                                [&](HipCall &call, dim3 grid, const DevGroup *d_groups, int count, uint64_t *d_res) {
                                  hipLaunchKernelGGL(compare_pairs_groups_iso_kernel, grid, dim3(256), dyn, call.st, a.d_events, a.d_out,
                                                     S1, b.d_events, b.d_out, S2, pa, as_text ? 1 : 0, d_groups, count, d_res);
                                });
  a.note_pass("compare_pairs_groups_iso");
  if (kernel_ms) *kernel_ms = ms;
}

}  // namespace miso
