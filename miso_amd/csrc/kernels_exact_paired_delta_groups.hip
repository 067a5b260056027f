// kernels_exact_paired_delta_groups.hip -- quantiles of delta psi between two GROUPS of paired-end replicates from the exact
// posteriors, without a draw (miso_exact_paired_delta_groups, miso_batch_exact_paired_delta_groups): kernels
// and host driver.
//
// The mixture, the rounds-as-launches shape, the workspace rows and exact_groups_update are kernels_exact_delta_groups.hip's
// (DESIGN.md 20a), and what the two units do alike is in exact_delta_groups.hpp: the exact_groups_sweep template, the argument
// checks, the guards of the batches' route, the driver of the launch ranges and the scatter.  This unit holds
// exact_paired_groups_tables and the two entry points.  H_ab is kernels_exact_paired_delta.hip's, operation for operation: A
// is the replicate with the narrower window in psi (a tie: the group-1 replicate), decided per pair; exact_delta_sweep over
// A's 2049 points with A's own tabulated f as the weight, exact_cdf_at on B's table.
//
// TABLES ONCE.  exact_paired_groups_tables, one wavefront per (event, replicate): the replicate's side of the event loaded
// with exact_paired_element (caller-given probabilities or the resident records of the replicate's batch), exact_paired_window
// and exact_paired_table in ExactPairedLds; F, f (the exact_idx image as it stands), the table's scalars, the window's width
// in psi and the ExactStats go to the replicate's row of the workspace -- EXACT_GROUPS_ROW's layout.  n1 + n2 tabulations an
// event, where n1 n2 pairwise calls make 2 n1 n2.
// THE SIDES.  Up to sixteen replicates, each with its own statistics and pairs or events, pool, fragment-length table: sixteen
// ExactPairedCmpSide travel as ONE kernel argument (896 bytes of the 4 KiB a launch may pass), indexed by the wavefront's
// replicate -- a uniform index into the kernel-argument segment, scalar loads, no scratch; no buffer to upload and one launch
// a range where a launch per replicate would make up to sixteen.
// THE SWEEP.  exact_groups_sweep<true>, the one template of exact_delta_groups.hpp: the weight is read from the f image of A's row
// (rowA[EXACT_PAD + exact_idx(point)]) -- the paired posterior's f needs the pair sum and cannot be made again from scalars.
// The lanes' loads lie 33 doubles apart; a second copy of f laid out [64 j + l] as kernels_exact_paired_delta.hip's row, each
// load one 512-byte line, was built first and read no faster (187.1 against 186.5 ms on DESIGN.md 20b's workload); without
// its 16.9 KB a replicate the call takes 181.8 ms, so there is none.  B's row is copied back into LDS byte for byte, A's
// scalars come from its row.
// No workgroup has more than one wavefront: no barrier in divergent control flow, no cooperative launch, no atomics.  f64, no
// contraction, miso_det_exp / miso_det_log, IEEE division, no inline assembly, plain vector stores.
// tests/_exact_paired_delta_groups_ref.py restates it and the two agree bit for bit
// (tests/test_gpu_exact_paired_delta_groups.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "batch.hpp"
#include "column_pass.hpp"
#include "device.hpp"
#include "miso_amd.h"
#include "miso_detmath.h"

#include "exact_delta.hpp"
#include "exact_delta_groups.hpp"
#include "exact_paired.hpp"
#include "exact_paired_pair.hpp"
#include "hip_host.hpp"

namespace miso {

// the replicates' sides of one call, group 1's first
struct ExactPairedGroupSides { ExactPairedCmpSide s[2 * EXACT_GROUP_MAX]; };

// One workgroup = one wavefront = one (event, replicate) of the launch's ne events, which are the call's events first ..
// first + ne.  ws: nb rows of EXACT_GROUPS_ROW doubles per event of the launch.
__global__ __launch_bounds__(64) void exact_paired_groups_tables(const ExactPairedGroupSides sides, const int32_t *list, int first, int nb,
                                                                 int ne, double *ws) {
  __shared__ ExactPairedLds L;
  const int lane = threadIdx.x;
  if (static_cast<int>(blockIdx.x) >= ne * nb) return;   // (uniform: the whole workgroup)
  const int e = static_cast<int>(blockIdx.x) / nb, r = static_cast<int>(blockIdx.x) % nb;
  ExactStats st; double c8; ExactPairs pr;
  exact_paired_cmp_side(sides.s[r], list, first + e, st, c8, pr);
  const ExactTable W = exact_uni(exact_paired_window(st, c8, pr, L.mbuf, L.red, L.redi, lane));
  const double w = exact_point(st, W.tR).x - exact_point(st, W.tL).x;
  const ExactTable T = exact_paired_table(st, W, pr, L.mbuf, L.F, L.f, L.fext, L.red, lane);
  exact_groups_store_row(ws + static_cast<size_t>(blockIdx.x) * EXACT_GROUPS_ROW, L.F, L.f, T, w, st, lane);
}

// The pass over m comparable events.  in[r]: replicate r's side of them, group 1's first (exact_paired_compare_run's form:
// caller-given m / offs, or a batch's device pointers with event j being list[j]); list may be null when no side is resident.
// rows: 2 + n_p + 1 + n_z doubles per event.  Everything is checked before anything is allocated; the sides go up and
// exact_groups_ranges takes the events through the device.
static void exact_paired_delta_groups_run(const ExactPairedCmpInput *in, int n1, int n2, const int32_t *list, int m, const double *p,
                                          int n_p, const double *z, int n_z, int max_events_per_launch, double *rows, float *ms,
                                          hipStream_t st) {
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device");
  const int nb = n1 + n2;
  int64_t n_pairs[2 * EXACT_GROUP_MAX];
  bool resident = false;
  for (int r = 0; r < nb; r++) {
    n_pairs[r] = exact_paired_check(in[r].stats6, in[r].m, in[r].m ? in[r].offs : nullptr, m);
    resident = resident || !in[r].m;
  }
  if (ms) *ms = 0.f;
  if (m == 0) return;
  HipCall call(st);
  ExactPairedGroupSides sides{};
  for (int r = 0; r < nb; r++) sides.s[r] = exact_paired_cmp_upload(call, in[r], m, n_pairs[r]);
  const int32_t *d_list = resident ? call.upload(list, static_cast<size_t>(m) * sizeof(int32_t)) : nullptr;
  exact_groups_ranges<true>(call, m, n1, n2, p, n_p, z, n_z, max_events_per_launch, [&](int e0, int ne, double *d_ws) {
    hipLaunchKernelGGL(exact_paired_groups_tables, dim3(ne * nb), dim3(64), 0, call.st, sides, d_list, e0, nb, ne, d_ws);
  }, rows);
  if (ms) *ms = call.elapsed_ms();
}

// Caller-given elements.  The comparable events' elements are gathered into the selftest's layout again (statistics, offsets
// from 0, probabilities), replicate by replicate, so that the kernels and exact_paired_check take them as they take a pair's.
void exact_paired_delta_groups_given(const double *const *stats6, const double *const *mm, const int64_t *const *offs, int n1, int n2,
                                     int n_events, const double *p, int n_p, const double *z, int n_z, int max_events_per_launch,
                                     double *out, int *was_exact, float *ms) {
  exact_groups_check(n1, n2, p, n_p, z, n_z);
  if (n_events < 0) MISO_FAIL(MISO_EINVAL, "Negative event count");
  if (max_events_per_launch < 0) MISO_FAIL(MISO_EINVAL, "Negative max_events_per_launch");
  const int nb = n1 + n2;
  for (int r = 0; r < nb && n_events > 0; r++) {
    if (!stats6[r] || !offs[r]) MISO_FAIL(MISO_EINVAL, "A replicate's statistics or offsets are NULL");
    if (offs[r][0] != 0) MISO_FAIL(MISO_EINVAL, "The pair offsets must start at 0");
    for (int i = 0; i < n_events; i++)
      if (offs[r][i + 1] < offs[r][i] || offs[r][i + 1] - offs[r][i] > INT32_MAX) MISO_FAIL(MISO_EINVAL, "The pair offsets must ascend");
    if (offs[r][n_events] > 0 && !mm[r]) MISO_FAIL(MISO_EINVAL, "A replicate has pairs and no probabilities");
  }
  std::vector<int32_t> list;
  for (int i = 0; i < n_events; i++) {
    bool ok = true;
    for (int r = 0; ok && r < nb; r++) {
      const double *q = stats6[r] + 6 * static_cast<size_t>(i);
      ok = exact_paired_eligible(2, q + 2, q + 4, false);
    }
    if (ok) list.push_back(i);
  }
  const int m = static_cast<int>(list.size());
  std::vector<std::vector<double>> cs(nb), cm(nb);
  std::vector<std::vector<int64_t>> co(nb);
  std::vector<ExactPairedCmpInput> in(nb);
  for (int r = 0; r < nb; r++) {
    co[r].push_back(0);
    for (int i : list) {
      const double *q = stats6[r] + 6 * static_cast<size_t>(i);
      cs[r].insert(cs[r].end(), q, q + 6);
      if (offs[r][i + 1] > offs[r][i]) cm[r].insert(cm[r].end(), mm[r] + 2 * offs[r][i], mm[r] + 2 * offs[r][i + 1]);
      co[r].push_back(static_cast<int64_t>(cm[r].size() / 2));
    }
    // (a replicate without a pair still takes the caller-given route: a placeholder stands for the empty list)
    if (cm[r].empty()) cm[r].assign(2, 1.0);
    in[r] = ExactPairedCmpInput{cs[r].data(), cm[r].data(), co[r].data(), nullptr, nullptr, nullptr, 0};
  }
  const size_t ncol = 2 + static_cast<size_t>(n_p) + 1 + static_cast<size_t>(n_z);
  std::vector<double> rows(static_cast<size_t>(m) * ncol);
  exact_paired_delta_groups_run(in.data(), n1, n2, nullptr, m, p, n_p, z, n_z, max_events_per_launch, rows.data(), ms, nullptr);
  exact_groups_scatter(list, rows, ncol, n_events, out, was_exact);
}

// The batches' route: exact_groups_guard's guards for paired-end batches, an event comparable when every batch's mode took it;
// the kernels read the batches' resident pair records, on the first batch's stream after all have been waited for.  Nothing
// is stored in any batch.
void exact_paired_delta_groups(miso_batch *const *g1, int n1, miso_batch *const *g2, int n2, const double *p, int n_p, const double *z,
                               int n_z, double *out, int64_t out_len, int *was_exact, float *kernel_ms) {
  const std::vector<miso_batch *> all = exact_groups_guard(g1, n1, g2, n2, true, p, n_p, z, n_z, out_len, kernel_ms);
  const int nb = n1 + n2;
  miso_batch &first = *all[0];
  const int n = static_cast<int>(first.events.size());
  const size_t ncol = 2 + static_cast<size_t>(n_p) + 1 + static_cast<size_t>(n_z);
  if (n == 0) return;
  std::vector<int32_t> list;
  for (int i = 0; i < n; i++) {
    bool ok = true;
    for (int r = 0; ok && r < nb; r++) ok = all[r]->event_exact(i);
    if (ok) list.push_back(i);
  }
  const int m = static_cast<int>(list.size());
  std::vector<std::vector<double>> cs(nb, std::vector<double>(static_cast<size_t>(m) * 6));
  std::vector<ExactPairedCmpInput> in;
  for (int r = 0; r < nb; r++) {
    for (int j = 0; j < m; j++) exact_paired_stats6(*all[r], list[j], &cs[r][static_cast<size_t>(j) * 6]);
    in.push_back(exact_paired_resident(*all[r], cs[r].data()));
  }
  std::vector<double> rows(static_cast<size_t>(m) * ncol);
  exact_groups_wait(all);
  exact_paired_delta_groups_run(in.data(), n1, n2, list.data(), m, p, n_p, z, n_z, 0, rows.data(), kernel_ms, first.stream);
  exact_groups_scatter(list, rows, ncol, n, out, was_exact);
}

}  // namespace miso
