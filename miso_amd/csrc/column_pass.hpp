// column_pass.hpp -- what the reduction passes over the resident sample pool share on the host, one workgroup per (event,
// isoform) column: summarize, diagnose, diagnose_rank, compare, compare_pairs (runtime.hip), compare_groups
// (kernels_compare_groups.hip) and compare_pairs_groups (kernels_compare_pairs_groups.hip).  A driver is its own guards and
// shape arithmetic; the column layout, the guards of a pair of batches, the credible interval's ranks, the pair passes'
// arguments and the launch itself are here, once.  Device memory, the upload and the event pair are a HipCall's (hip_host.hpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "batch.hpp"
#include "compare_pairs.hpp"

namespace miso {

// Where event i's columns start in a pass's results: `w` values per isoform, off[i] counted in values.
struct ColumnLayout {
  std::vector<uint64_t> off;
  uint64_t total = 0;
  int kmax = 1;
};
inline ColumnLayout column_layout(const miso_batch &b, int w) {
  ColumnLayout l;
  l.off.reserve(b.events.size());
  for (const PackedEvent &e : b.events) {
    l.off.push_back(l.total);
    l.total += static_cast<uint64_t>(w) * e.K;
    l.kmax = std::max(l.kmax, e.K);
  }
  return l;
}

// stop = CONVERGENT_MEAN: a launch is only finished once sync() has run its further rounds; without them the pool holds the
// unconverged first round
inline void finish_rounds(miso_batch &b) {
  if (b.p.stop == MISO_STOP_CONVERGENT_MEAN && !b.converged_done) b.sync(nullptr);
}

// The order statistics that bound the `level` credible interval of n draws (credible_intervals.py:31-55:
// int(round(alpha/2 n)) - 1 and int(round((1 - alpha/2) n)) - 1, Python-2 rounding = half away from zero), in double.
// Strict: the reference asserts both indices > 0.  Clamped: into [0, n - 1] and in order, for the all-pairs passes.
struct CiRanks { double lo, hi; };
inline CiRanks ci_ranks(double n, double level) {
  const double alpha = 1 - level;
  return {std::floor((alpha / 2) * n + 0.5) - 1, std::floor((1 - alpha / 2) * n + 0.5) - 1};
}
inline CiRanks ci_ranks_strict(double n, double level) {
  const CiRanks r = ci_ranks(n, level);
  if (!(r.lo > 0 && r.hi > 0 && r.hi < n)) MISO_FAIL(MISO_EINVAL, "Too few samples for a credible interval");
  return r;
}
inline CiRanks ci_ranks_clamped(double n, double level) {
  CiRanks r = ci_ranks(n, level);
  r.lo = std::max(0.0, r.lo);
  r.hi = std::min(n - 1, std::max(r.lo, r.hi));
  return r;
}

// The arguments of an all-pairs pass over M = N1 * N2 differences (M <= 2^28: every product and sum of the ranks is far from
// 2^53), after the guards of the confidence level and the thresholds.
inline PairsArgs pairs_args(int64_t M, double confidence_level, const double *tau, int n_tau) {
  if (!(confidence_level > 0 && confidence_level < 1)) MISO_FAIL(MISO_EINVAL, "Invalid confidence level: it must lie inside (0, 1)");
  if (n_tau < 0 || n_tau > PAIRS_MAX_TAU) MISO_FAIL(MISO_EINVAL, "Invalid number of delta psi thresholds: 0 to 4");
  for (int j = 0; j < n_tau; j++)
    if (!(tau[j] > 0 && tau[j] < 1)) MISO_FAIL(MISO_EINVAL, "Invalid delta psi threshold: it must lie inside (0, 1)");
  const CiRanks r = ci_ranks_clamped(static_cast<double>(M), confidence_level);
  PairsArgs pa{};
  pa.rank[0] = static_cast<uint32_t>((M - 1) / 2);
  pa.rank[1] = static_cast<uint32_t>(r.lo);
  pa.rank[2] = static_cast<uint32_t>(r.hi);
  pa.n_tau = n_tau;
  for (int j = 0; j < n_tau; j++) pa.tau[j] = tau[j];
  return pa;
}

// Batch b holds the events batch a holds: both launched, on one device, as many events, with same_S as many samples per
// event, and event by event as many isoforms.  `who` goes in front of the message (the group drivers name the batch).
inline void same_events(const miso_batch &a, const miso_batch &b, bool same_S, const std::string &who = "") {
  if (!a.launched || !b.launched) MISO_FAIL(MISO_EINVAL, who + "batch not launched");
  if (a.device != b.device) MISO_FAIL(MISO_EINVAL, who + "Batches to compare live on different devices");
  if (a.events.size() != b.events.size() || (same_S && a.S() != b.S()))
    MISO_FAIL(MISO_EINVAL, who + (same_S ? "Batches to compare differ in events or samples per event" : "Batches to compare differ in events"));
  for (size_t i = 0; i < a.events.size(); i++)
    if (a.events[i].K != b.events[i].K) MISO_FAIL(MISO_EINVAL, who + "Events to compare differ in isoforms");
}

// The two groups of a group comparison as one list, group 1 first: every batch there and holding the first one's events.
inline std::vector<miso_batch *> same_events_groups(miso_batch *const *g1, int n1, miso_batch *const *g2, int n2) {
  if (n1 < 1 || n2 < 1) MISO_FAIL(MISO_EINVAL, "Each group needs at least one batch");
  std::vector<miso_batch *> all;
  for (int i = 0; i < n1 + n2; i++) {
    miso_batch *b = i < n1 ? g1[i] : g2[i - n1];
    const std::string who = "group " + std::to_string(i < n1 ? 1 : 2) + " batch " + std::to_string(i < n1 ? i : i - n1) + ": ";
    if (!b) MISO_FAIL(MISO_EINVAL, who + "batch is NULL");
    all.push_back(b);
    same_events(*b, *all[0], true, who);
  }
  return all;
}
// ... and their event tables and sample pools as the group kernels take them: n1 + n2 tables, then n1 + n2 pools
inline std::vector<const void *> group_pointers(const std::vector<miso_batch *> &all) {
  const size_t nb = all.size();
  std::vector<const void *> ptrs(2 * nb);
  for (size_t i = 0; i < nb; i++) { ptrs[i] = all[i]->d_events; ptrs[nb + i] = all[i]->d_out; }
  return ptrs;
}

// The pass itself on the call's stream: `kernel` may use `dyn` bytes of dynamic LDS, the offset table goes up, `launch(grid,
// d_off, d_res)` starts the kernel on `grid` (or, the pooled pass, its kernels on parts of it) between the call's two events,
// the n_out results come back into `out`, the stream is synchronised.  Returns the kernel time.  Whatever fails, the call
// frees what it holds.
template <class T, class Launch>
float column_pass(HipCall &call, const void *kernel, dim3 grid, size_t dyn, const std::vector<uint64_t> &off, size_t n_out, T *out,
                  Launch &&launch) {
  if (dyn > 0) HIP_OK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(dyn)));
  T *d_res = call.alloc<T>(n_out * sizeof(T));
  const uint64_t *d_off = call.upload(off.data(), off.size() * sizeof(uint64_t));
  call.start();
  launch(grid, d_off, d_res);
  HIP_OK(hipGetLastError());
  call.stop();
  HIP_OK(hipMemcpyAsync(out, d_res, n_out * sizeof(T), hipMemcpyDeviceToHost, call.st));
  HIP_OK(hipStreamSynchronize(call.st));
  return call.elapsed_ms();
}

}  // namespace miso
