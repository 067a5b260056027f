// exact_delta_groups.hpp -- what the two units that pool the exact quantiles of delta psi over GROUPS of replicates share
// (kernels_exact_delta_groups.hip, single-end; kernels_exact_paired_delta_groups.hip, paired-end, DESIGN.md
// 20b): the limits, the layout of a replicate's row of the global workspace with its stores and loads, the sweep kernel
// (one template, the weight chosen at compile time), and on the host the checks of a call's arguments, the guards of the
// batches' route, the driver of the launch ranges and the rows' scatter.  Each unit keeps its own tables kernel;
// exact_groups_update lives in the single-end unit and only reads rows and the pairs' H.  -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "batch.hpp"
#include "column_pass.hpp"
#include "device.hpp"

#include "exact_delta.hpp"
#include "hip_host.hpp"

namespace miso {

constexpr int EXACT_GROUP_MAX = 8;                                  // replicates a group
// a replicate's row of the workspace, in doubles: F, f, then {tm, gmax, tL, tR, h, Z, mean0, mean1, sf}, the window's width in
// psi, {am1, bm1, a, b, c, n, e0, e1}
constexpr int EXACT_GROUPS_SCALARS = 18;
constexpr int EXACT_GROUPS_ROW = 2 * EXACT_PAD + EXACT_GROUPS_SCALARS;
// the sweeps of the first launch: slot 0 H(0.0), slot 1 round 1, slot 2 the caller's points; later slot k = probability k
constexpr int EXACT_GROUPS_FIRST_SLOTS = 3;
// what one launch range holds on the device at most (workspace, the pairs' H and the brackets)
constexpr size_t EXACT_GROUPS_WORK_BYTES = size_t{256} << 20;

__device__ __forceinline__ void exact_groups_store_scalars(double *s, const ExactTable &T, double w, const ExactStats &st) {
  s[0] = T.tm; s[1] = T.gmax; s[2] = T.tL; s[3] = T.tR; s[4] = T.h; s[5] = T.Z; s[6] = T.mean0; s[7] = T.mean1; s[8] = T.sf;
  s[9] = w;
  s[10] = st.am1; s[11] = st.bm1; s[12] = st.a; s[13] = st.b; s[14] = st.c; s[15] = st.n; s[16] = st.e0; s[17] = st.e1;
}
__device__ __forceinline__ ExactTable exact_groups_load_table(const double *s, const double *F, const double *f) {
  ExactTable T;
  T.tm = s[0]; T.gmax = s[1]; T.tL = s[2]; T.tR = s[3]; T.h = s[4]; T.Z = s[5]; T.mean0 = s[6]; T.mean1 = s[7]; T.sf = s[8];
  T.F = F; T.f = f;
  return T;
}
__device__ __forceinline__ ExactStats exact_groups_load_stats(const double *s) {
  ExactStats st;
  st.am1 = s[10]; st.bm1 = s[11]; st.a = s[12]; st.b = s[13]; st.c = s[14]; st.n = s[15]; st.e0 = s[16]; st.e1 = s[17];
  return st;
}
// the end of a tables kernel: the wavefront's tabulated F, f (LDS) and scalars go to the replicate's row.  All EXACT_PAD
// words, the exact_idx image's unused padding words included: the tabulation never writes those, nothing reads them, and they
// travel LDS -> workspace -> LDS as they are
__device__ __forceinline__ void exact_groups_store_row(double *row, const double *F, const double *f, const ExactTable &T, double w,
                                                       const ExactStats &st, int lane) {
  for (int i = lane; i < EXACT_PAD; i += 64) { row[i] = F[i]; row[EXACT_PAD + i] = f[i]; }
  if (lane == 0) exact_groups_store_scalars(row + 2 * EXACT_PAD, T, w, st);
}

// The sweep of both units.  One workgroup = one wavefront.  first != 0: one per (event, pair), H_ab at 0.0 (slot 0), at round
// 1's points (slot 1) and, n_z > 0, at z[0 .. n_z) (slot 2).  first == 0: one per (event, pair, probability k), H_ab at the
// points of bracket br[event][k] (slot k).  Hp: n_slots rows of eight doubles per (event, pair), the pairs a-major.
// F_FROM_ROW: A's f is read from the f image of A's row (paired-end: the posterior's f needs the pair sum and cannot be made
// again from scalars; the lanes' loads lie 33 doubles apart); otherwise it is made again from exact_point (single-end).
template <bool F_FROM_ROW>
__global__ __launch_bounds__(64) void exact_groups_sweep(const double *ws, const ExactBracket *br, const double *zc, int n_z, int n1,
                                                         int n2, int ne, int n_p, int n_slots, int first, double *Hp) {
  __shared__ double F[EXACT_PAD], f[EXACT_PAD], red[256];
  const int lane = threadIdx.x;
  const int np_pairs = n1 * n2, nb = n1 + n2;
  const int per_event = first ? np_pairs : np_pairs * n_p;
  if (static_cast<int>(blockIdx.x) >= ne * per_event) return;   // (uniform: the whole workgroup)
  const int e = static_cast<int>(blockIdx.x) / per_event, in_e = static_cast<int>(blockIdx.x) % per_event;
  const int pair = first ? in_e : in_e / n_p, k = first ? 0 : in_e % n_p;
  const int a = pair / n2, b = pair % n2;
  const double *row1 = ws + (static_cast<size_t>(e) * nb + a) * EXACT_GROUPS_ROW;
  const double *row2 = ws + (static_cast<size_t>(e) * nb + n1 + b) * EXACT_GROUPS_ROW;
  const bool a2 = row2[2 * EXACT_PAD + 9] < row1[2 * EXACT_PAD + 9];   // A = the group-2 replicate
  const double *rowA = a2 ? row2 : row1, *rowB = a2 ? row1 : row2;
  for (int i = lane; i < EXACT_PAD; i += 64) { F[i] = rowB[i]; f[i] = rowB[EXACT_PAD + i]; }
  const ExactStats stA = exact_groups_load_stats(rowA + 2 * EXACT_PAD);
  const ExactTable TA = exact_groups_load_table(rowA + 2 * EXACT_PAD, nullptr, nullptr);   // (only its scalars are used)
  const ExactTable TB = exact_groups_load_table(rowB + 2 * EXACT_PAD, F, f);
  __syncthreads();
  const auto weight = [&](int, int pt, const ExactPoint &p) __attribute__((always_inline)) {
    if constexpr (F_FROM_ROW) return rowA[EXACT_PAD + exact_idx(pt)];
    else return miso_det_exp(p.g - TA.gmax);
  };
  double *o = Hp + (static_cast<size_t>(e) * np_pairs + pair) * n_slots * EXACT_DELTA_PTS;
  if (first) {
    const double z0[1] = {0.0};
    double H0[1];
    exact_delta_sweep<1>(stA, TA, TB, a2, z0, H0, red, lane, weight);
    if (lane == 0) o[0] = H0[0];
  }
  // (the caller's points: five to eight of them take a second eight-wide sweep, one to four a four-wide one below)
  const int n_sweeps = first && n_z > EXACT_DELTA_PTS / 2 ? 2 : 1;
#pragma unroll 1
  for (int s = 0; s < n_sweeps; s++) {
    double z[EXACT_DELTA_PTS], H[EXACT_DELTA_PTS];
    if (first && s == 1) {
#pragma unroll
      for (int j = 0; j < EXACT_DELTA_PTS; j++) z[j] = j < n_z ? zc[j] : 0.0;
    } else {
      const ExactBracket all{-1.0, 0.0, 1.0, 1.0};
      exact_delta_points(first ? all : br[static_cast<size_t>(e) * n_p + k], z);
    }
    exact_delta_sweep<EXACT_DELTA_PTS>(stA, TA, TB, a2, z, H, red, lane, weight);
    if (lane == 0) {
      double *os = o + static_cast<size_t>(first ? 1 + s : k) * EXACT_DELTA_PTS;
#pragma unroll
      for (int j = 0; j < EXACT_DELTA_PTS; j++) os[j] = H[j];
    }
  }
  if (first && n_z > 0 && n_z <= EXACT_DELTA_PTS / 2) {
    constexpr int HALF = EXACT_DELTA_PTS / 2;
    double z[HALF], H[HALF];
#pragma unroll
    for (int j = 0; j < HALF; j++) z[j] = j < n_z ? zc[j] : 0.0;
    exact_delta_sweep<HALF>(stA, TA, TB, a2, z, H, red, lane, weight);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < HALF; j++) o[2 * EXACT_DELTA_PTS + j] = H[j];
    }
  }
}

// kernels_exact_delta_groups.hip: exact_groups_update on `st` for the ne events of a range, (ne n_p + 63) / 64 workgroups
void exact_groups_update_launch(hipStream_t st, const double *ws, const double *Hp, const double *prob, int n_p, int n_z, int n1, int n2,
                                int ne, int n_slots, int round, ExactBracket *br, double *out);

// A call's arguments: the groups' sizes (at_least_one = false: only their upper limit, where an empty group is
// same_events_groups' to name), then the probabilities and the points.
inline void exact_groups_check_sizes(int n1, int n2, bool at_least_one = true) {
  if ((at_least_one && (n1 < 1 || n2 < 1)) || n1 > EXACT_GROUP_MAX || n2 > EXACT_GROUP_MAX)
    MISO_FAIL(MISO_EINVAL, "The number of replicates of a group must lie in [1, 8]");
}
inline void exact_groups_check(int n1, int n2, const double *p, int n_p, const double *z, int n_z) {
  exact_groups_check_sizes(n1, n2);
  exact_delta_check_p(p, n_p);
  exact_check_z(z, n_z);
}

// The guards of the batches' route: a device, the groups as one list with every batch holding the first one's events, every
// batch of the family (paired-end or single-end) and run with its exact mode, the call's arguments, out long enough for 2 +
// n_p + 1 + n_z doubles per event.  Returns the list; *kernel_ms = 0 from here on.
inline std::vector<miso_batch *> exact_groups_guard(miso_batch *const *g1, int n1, miso_batch *const *g2, int n2, bool paired,
                                                    const double *p, int n_p, const double *z, int n_z, int64_t out_len,
                                                    float *kernel_ms) {
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device: the comparison has no CPU path");
  exact_groups_check_sizes(n1, n2, false);
  std::vector<miso_batch *> all = same_events_groups(g1, n1, g2, n2);
  for (int i = 0; i < n1 + n2; i++) {
    const miso_batch &b = *all[i];
    const std::string who = "group " + std::to_string(i < n1 ? 1 : 2) + " batch " + std::to_string(i < n1 ? i : i - n1) + ": ";
    if (b.p.paired != paired)
      MISO_FAIL(MISO_EINVAL, who + (paired ? "a single-end batch cannot take part in the paired exact group comparison"
                                           : "a paired-end batch cannot take part in the exact group comparison"));
    const bool mode = paired ? b.exact_paired : b.exact;
    if (!mode || b.slots_exact != mode)
      MISO_FAIL(MISO_EINVAL, who + "the batch has not run with the " + (paired ? "paired " : "") + "exact-posterior mode");
  }
  exact_groups_check(n1, n2, p, n_p, z, n_z);
  const size_t ncol = 2 + static_cast<size_t>(n_p) + 1 + static_cast<size_t>(n_z);
  if (out_len < 0 || static_cast<uint64_t>(out_len) < static_cast<uint64_t>(all[0]->events.size()) * ncol)
    MISO_FAIL(MISO_EINVAL, "out is too short for 2 + n_p + 1 + n_z doubles per event");
  if (kernel_ms) *kernel_ms = 0.f;
  return all;
}
// ... and before the run on the first batch's stream: its device current, every batch's stream waited for
inline void exact_groups_wait(const std::vector<miso_batch *> &all) {
  HIP_OK(hipSetDevice(all[0]->device));
  for (miso_batch *b : all) HIP_OK(hipStreamSynchronize(b->stream));
}

// The device part of a call over m > 0 comparable events.  The caller has uploaded on `call` what its tables kernel reads;
// tables(e0, ne, d_ws) launches that kernel for the events e0 .. e0 + ne into the workspace.  The events go in ranges of at
// most `per_launch` -- what EXACT_GROUPS_WORK_BYTES holds, max_events_per_launch > 0 a lower cap --, eleven launches a range
// in one stream: the tables, then five times exact_groups_sweep<F_FROM_ROW> and exact_groups_update; one pair of HIP events
// around them all (call.elapsed_ms()).  rows: 2 + n_p + 1 + n_z doubles per event, on the host once this returns.
template <bool F_FROM_ROW, class Tables>
void exact_groups_ranges(HipCall &call, int m, int n1, int n2, const double *p, int n_p, const double *z, int n_z,
                         int max_events_per_launch, Tables &&tables, double *rows) {
  const int nb = n1 + n2, np_pairs = n1 * n2;
  const size_t ncol = 2 + static_cast<size_t>(n_p) + 1 + static_cast<size_t>(n_z);
  const int n_slots = std::max(n_p, EXACT_GROUPS_FIRST_SLOTS);
  const size_t ws_ev = static_cast<size_t>(nb) * EXACT_GROUPS_ROW, hp_ev = static_cast<size_t>(np_pairs) * n_slots * EXACT_DELTA_PTS;
  const size_t bytes_ev = (ws_ev + hp_ev) * sizeof(double) + static_cast<size_t>(n_p) * sizeof(ExactBracket);
  int per_launch = static_cast<int>(std::min<size_t>(m, std::max<size_t>(1, EXACT_GROUPS_WORK_BYTES / bytes_ev)));
  if (max_events_per_launch > 0) per_launch = std::min(per_launch, max_events_per_launch);

  const double *d_p = call.upload(p, static_cast<size_t>(n_p) * sizeof(double));
  const double *d_z = call.upload(z, static_cast<size_t>(n_z) * sizeof(double));
  double *d_ws = call.alloc(ws_ev * per_launch * sizeof(double));
  double *d_hp = call.alloc(hp_ev * per_launch * sizeof(double));
  ExactBracket *d_br = call.alloc<ExactBracket>(static_cast<size_t>(per_launch) * n_p * sizeof(ExactBracket));
  double *d_out = call.alloc(static_cast<size_t>(m) * ncol * sizeof(double));
  call.start();
  // (the ranges follow one another in the stream, each with the whole workspace: one pair of events times their sum)
  for (int e0 = 0; e0 < m; e0 += per_launch) {
    const int ne = std::min(per_launch, m - e0);
    double *d_o = d_out + static_cast<size_t>(e0) * ncol;
    tables(e0, ne, d_ws);
    HIP_OK(hipGetLastError());
    for (int round = 0; round < EXACT_DELTA_ROUNDS; round++) {
      const int first = round == 0 ? 1 : 0;
      hipLaunchKernelGGL(exact_groups_sweep<F_FROM_ROW>, dim3(ne * np_pairs * (first ? 1 : n_p)), dim3(64), 0, call.st, d_ws, d_br, d_z,
                         n_z, n1, n2, ne, n_p, n_slots, first, d_hp);
      HIP_OK(hipGetLastError());
      exact_groups_update_launch(call.st, d_ws, d_hp, d_p, n_p, n_z, n1, n2, ne, n_slots, round, d_br, d_o);
    }
  }
  call.stop();
  HIP_OK(hipMemcpyAsync(rows, d_out, static_cast<size_t>(m) * ncol * sizeof(double), hipMemcpyDeviceToHost, call.st));
  HIP_OK(hipStreamSynchronize(call.st));
}

// the rows' scatter: event list[j] gets row j of `rows` and was_exact = 1, every other event keeps its row of out and gets 0
inline void exact_groups_scatter(const std::vector<int32_t> &list, const std::vector<double> &rows, size_t ncol, int n_events, double *out,
                                 int *was_exact) {
  for (int i = 0; i < n_events; i++) was_exact[i] = 0;
  for (size_t j = 0; j < list.size(); j++) {
    std::memcpy(out + static_cast<size_t>(list[j]) * ncol, &rows[j * ncol], ncol * sizeof(double));
    was_exact[list[j]] = 1;
  }
}

}  // namespace miso
