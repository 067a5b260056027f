// kernels_exact_delta_groups.hip -- quantiles of delta psi between two GROUPS of replicates from the exact posteriors, without
// a draw (miso_exact_delta_groups, miso_batch_exact_delta_groups): kernels and host driver.
//
// The law of "psi of a replicate of group 1 minus psi of a replicate of group 2", equal weights, is the equal-weight mixture
// of the n1 n2 pairwise laws: H(z) = (sum_a sum_b H_ab(z)) / (double) (n1 n2), the sum from 0.0 with a outer and b inner, one
// division.  H_ab is kernels_exact_delta.hip's, operation for operation: A is the posterior with the narrower window in psi (a
// tie: the group-1 replicate), decided per pair; exact_delta_sweep over A's 2049 points against B's table.  H(z) = p is solved
// by exact_delta.hpp's search on this H: H(0.0), five rounds of eight points, exact_delta_update, exact_delta_interpolate.
//
// TABLES ONCE.  exact_groups_tables, one wavefront per (event, replicate): exact_window and exact_table in the static LDS
// layout of the pairwise kernel, then F, f (all EXACT_PAD doubles each, the exact_idx layout as it stands), the table's
// scalars, the window's width in psi and the ExactStats go to the replicate's row of a global workspace with plain vector
// stores.  n1 + n2 tabulations an event, where n1 n2 pairwise calls make 2 n1 n2.
// ROUNDS AS LAUNCHES.  exact_groups_sweep, one wavefront per (event, pair) in the first launch -- H(0.0), round 1 on (-1, 1)
// and the caller's n_z points (four-wide for up to four of them, eight-wide beyond), up to three sweeps -- and per (event,
// pair, probability) in the four that follow: B's row is
// copied back into LDS (the same image, so exact_cdf_at and its bank-skewed indexing run unchanged), A's scalars come from its
// row and its f is made again from exact_point, the eight H_ab go out with plain stores.  exact_groups_update, one thread per
// (event, probability): the pairs added in the defined order, the division, exact_delta_update, and after the last round the
// interpolation; thread 0 of an event also writes the group means, H(0.0) and H(z_j) after the first launch.
// No workgroup has more than one wavefront: no barrier in divergent control flow, no cooperative launch, no atomics.  f64, no
// contraction, miso_det_exp / miso_det_log, IEEE division, no inline assembly.  tests/_exact_delta_groups_ref.py restates it
// and the two agree bit for bit (tests/test_gpu_exact_delta_groups.py).  This unit holds exact_groups_tables,
// exact_groups_update and the two entry points; the limits, the row's layout, the exact_groups_sweep template (here
// exact_groups_sweep<false>: f made again from scalars), the argument checks, the guards of the batches' route, the driver of
// the launch ranges and the scatter are in exact_delta_groups.hpp, shared with the paired-end unit
// (kernels_exact_paired_delta_groups.hip).
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
#include "hip_host.hpp"

namespace miso {

// One workgroup = one wavefront = one (event, replicate) of the launch's ne events.  stats7: nb rows of {n10, n01, n, e0, e1,
// h0, h1} per event, group 1's first; ws: nb rows of EXACT_GROUPS_ROW doubles per event
__global__ __launch_bounds__(64) void exact_groups_tables(const double *stats7, int nb, int ne, double *ws) {
  __shared__ double F[EXACT_PAD], f[EXACT_PAD], red[256];
  const int lane = threadIdx.x;
  if (static_cast<int>(blockIdx.x) >= ne * nb) return;   // (uniform: the whole workgroup)
  const double *q = stats7 + 7 * static_cast<size_t>(blockIdx.x);
  const ExactStats st = exact_stats(q[0], q[1], q[2], q[3], q[4], q[5] - 1.0, q[6] - 1.0);
  const ExactTable W = exact_window(st, lane);
  const double w = exact_point(st, W.tR).x - exact_point(st, W.tL).x;
  const ExactTable T = exact_table(st, W, F, f, red, lane);
  exact_groups_store_row(ws + static_cast<size_t>(blockIdx.x) * EXACT_GROUPS_ROW, F, f, T, w, st, lane);
}

// the mixture's value from the pairs' column j of slot `slot`: from 0.0, a outer and b inner, divided once
__device__ __forceinline__ double exact_groups_mix(const double *Hp_e, int np_pairs, int n_slots, int slot, int j) {
  double s = 0.0;
  for (int pr = 0; pr < np_pairs; pr++) s = s + Hp_e[(static_cast<size_t>(pr) * n_slots + slot) * EXACT_DELTA_PTS + j];
  return s / static_cast<double>(np_pairs);
}

// One thread per (event, probability): round 0 after the first sweep launch, rounds 1 .. EXACT_DELTA_ROUNDS - 1 after the
// others.  out: 2 + n_p + 1 + n_z doubles per event: m1, m2, q, H(0.0), H(z).
__global__ __launch_bounds__(64) void exact_groups_update(const double *ws, const double *Hp, const double *prob, int n_p, int n_z,
                                                          int n1, int n2, int ne, int n_slots, int round, ExactBracket *br,
                                                          double *out) {
  const int t = static_cast<int>(blockIdx.x) * 64 + static_cast<int>(threadIdx.x);
  if (t >= ne * n_p) return;
  const int e = t / n_p, k = t % n_p;
  const int np_pairs = n1 * n2, nb = n1 + n2;
  const double *Hp_e = Hp + static_cast<size_t>(e) * np_pairs * n_slots * EXACT_DELTA_PTS;
  double *o = out + static_cast<size_t>(e) * (2 + n_p + 1 + n_z);
  const double pk = prob[k];
  ExactBracket b{-1.0, 0.0, 1.0, 1.0};
  if (round > 0) b = br[t];
  double z[EXACT_DELTA_PTS], H[EXACT_DELTA_PTS];
  exact_delta_points(b, z);
#pragma unroll
  for (int j = 0; j < EXACT_DELTA_PTS; j++) H[j] = exact_groups_mix(Hp_e, np_pairs, n_slots, round > 0 ? k : 1, j);
  b = exact_delta_update(b, z, H, pk);
  br[t] = b;
  if (round == EXACT_DELTA_ROUNDS - 1) o[2 + k] = exact_delta_interpolate(b, pk);
  if (round == 0 && k == 0) {
    const double *rows = ws + static_cast<size_t>(e) * nb * EXACT_GROUPS_ROW + 2 * EXACT_PAD + 6;   // (mean0 of replicate 0)
    double m1 = 0.0, m2 = 0.0;
    for (int a = 0; a < n1; a++) m1 = m1 + rows[static_cast<size_t>(a) * EXACT_GROUPS_ROW];
    for (int c = 0; c < n2; c++) m2 = m2 + rows[static_cast<size_t>(n1 + c) * EXACT_GROUPS_ROW];
    o[0] = m1 / static_cast<double>(n1); o[1] = m2 / static_cast<double>(n2);
    o[2 + n_p] = exact_groups_mix(Hp_e, np_pairs, n_slots, 0, 0);
    for (int j = 0; j < n_z; j++) o[3 + n_p + j] = exact_groups_mix(Hp_e, np_pairs, n_slots, 2, j);
  }
}

void exact_groups_update_launch(hipStream_t st, const double *ws, const double *Hp, const double *prob, int n_p, int n_z, int n1, int n2,
                                int ne, int n_slots, int round, ExactBracket *br, double *out) {
  hipLaunchKernelGGL(exact_groups_update, dim3((ne * n_p + 63) / 64), dim3(64), 0, st, ws, Hp, prob, n_p, n_z, n1, n2, ne, n_slots, round,
                     br, out);
  HIP_OK(hipGetLastError());
}

// Rows [event][replicate][7] of the two groups; take (may be null): per event, whether the caller lets it be compared at all.
// An event is comparable when every row is eligible and all rows carry bit-equal (e0, e1); every other event keeps its row of
// out and gets was_exact = 0.  The comparable ones' rows go up and exact_groups_ranges takes them through the device.
void exact_delta_groups_run(const double *stats7_1, int n1, const double *stats7_2, int n2, int n_events, const unsigned char *take,
                            const double *p, int n_p, const double *z, int n_z, int max_events_per_launch, double *out,
                            int *was_exact, float *ms, hipStream_t st) {
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device");
  exact_groups_check_sizes(n1, n2);
  if (n_events < 0) MISO_FAIL(MISO_EINVAL, "Negative event count");
  if (max_events_per_launch < 0) MISO_FAIL(MISO_EINVAL, "Negative max_events_per_launch");
  exact_delta_check_p(p, n_p);
  exact_check_z(z, n_z);
  if (ms) *ms = 0.f;
  const int nb = n1 + n2;
  const size_t ncol = 2 + static_cast<size_t>(n_p) + 1 + static_cast<size_t>(n_z);
  std::vector<int32_t> list;
  std::vector<double> rows;
  for (int i = 0; i < n_events; i++) {
    const double *g1 = stats7_1 + static_cast<size_t>(i) * n1 * 7, *g2 = stats7_2 + static_cast<size_t>(i) * n2 * 7;
    bool ok = !take || take[i];
    for (int r = 0; ok && r < nb; r++) {
      const double *q = r < n1 ? g1 + 7 * r : g2 + 7 * (r - n1);
      ok = exact_eligible(false, 2, q + 3, q + 5) && std::memcmp(q + 3, g1 + 3, 2 * sizeof(double)) == 0;
    }
    if (!ok) continue;
    list.push_back(i);
    rows.insert(rows.end(), g1, g1 + static_cast<size_t>(n1) * 7);
    rows.insert(rows.end(), g2, g2 + static_cast<size_t>(n2) * 7);
  }
  const int m = static_cast<int>(list.size());
  std::vector<double> got(static_cast<size_t>(m) * ncol);
  if (m > 0) {
    HipCall call(st);
    const double *d_rows = call.upload(rows.data(), rows.size() * sizeof(double));
    exact_groups_ranges<false>(call, m, n1, n2, p, n_p, z, n_z, max_events_per_launch, [&](int e0, int ne, double *d_ws) {
      hipLaunchKernelGGL(exact_groups_tables, dim3(ne * nb), dim3(64), 0, call.st, d_rows + static_cast<size_t>(e0) * nb * 7, nb, ne, d_ws);
    }, got.data());
    if (ms) *ms = call.elapsed_ms();
  }
  exact_groups_scatter(list, got, ncol, n_events, out, was_exact);
}

// The batches' route: exact_groups_guard's guards for single-end batches, the rows from exact_stats7 (an event some batch's
// exact mode did not take is not comparable), then the pass above on the first batch's stream.  Nothing is stored in any
// batch.
void exact_delta_groups(miso_batch *const *g1, int n1, miso_batch *const *g2, int n2, const double *p, int n_p, const double *z, int n_z,
                        double *out, int64_t out_len, int *was_exact, float *kernel_ms) {
  const std::vector<miso_batch *> all = exact_groups_guard(g1, n1, g2, n2, false, p, n_p, z, n_z, out_len, kernel_ms);
  miso_batch &r = *all[0];
  const int n = static_cast<int>(r.events.size());
  if (n == 0) return;
  std::vector<double> s1(static_cast<size_t>(n) * n1 * 7), s2(static_cast<size_t>(n) * n2 * 7);
  std::vector<unsigned char> take(n, 1);
  for (int i = 0; i < n; i++)
    for (int c = 0; c < n1 + n2; c++) {
      const miso_batch &b = *all[c];
      if (!b.event_exact(i)) take[i] = 0;
      b.exact_stats7(i, c < n1 ? &s1[(static_cast<size_t>(i) * n1 + c) * 7] : &s2[(static_cast<size_t>(i) * n2 + (c - n1)) * 7]);
    }
  exact_groups_wait(all);
  exact_delta_groups_run(s1.data(), n1, s2.data(), n2, n, take.data(), p, n_p, z, n_z, 0, out, was_exact, kernel_ms, r.stream);
}

}  // namespace miso
