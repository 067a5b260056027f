// kernels_exact_paired_compare.hip -- two paired-end exact-mode posteriors of one event compared without a draw
// (miso_batch_compare_exact_paired).
//
// Sample s has the density of kernels_exact_paired.hip,
//     log p_s(x) = (n10_s + h0_s - 1) log x + (n01_s + h1_s - 1) log y + P_s(x) - n_s log(x A0_s + y A1_s),
// P_s the sum over that sample's drawing pairs.  kernels_exact_compare.hip's reduction to five pooled numbers does not
// apply: the A differ between the samples (each sample has its own fragment-length law), and the pair sums do not pool.
// But p_1 p_2 is again an explicit density -- ExactSecondSegment in exact_paired.hpp: pooled exponents, hyperparameters
// h1 + h2 - 1, both pair sums, both denominators -- with g'' >= -(n1 + n2 + h0p + h1p) / 4, so the two-pass window and the
// fourth-order table of the paired mode tabulate it as they tabulate one sample's.  From there on everything is the
// single-end comparison's, and the same code (exact_compare.hpp):
//     log_d0 = (lZ12 - lZ1) - lZ2,  log Z = gref + log(F[G]);  log_bf = log_prior0 - log_d0 (log_prior0 from the host);
//     H(z) = P(psi_1 - psi_2 <= z): the trapezoid sum over the 2049 points of A, the posterior with the narrower window in
//     psi (a tie: sample 1), of w f_A / sum w f_A times B's tabulated CDF at the shifted argument (exact_cdf_at).
// One thing differs: A's f cannot be made again from scalars, it needs A's pair sum.  After A's table every lane writes the f
// of its own 32 points (33: lane 63) to the workgroup's row of a global buffer, point j of lane l at [64 j + l] so that the
// wavefront's accesses are contiguous, and reads them back in the quadrature; x and 1 - x there come from exact_point.
//
// ONE WAVEFRONT = one workgroup per pair, ExactPairedLds's 37 KB holding one F / f pair at a time: windows of both samples,
// table of A (scalars and own f kept), window and table of the pooled density (Z12, gref12), table of B, which stays for
// the n_z quadratures.  f64, no contraction, miso_det_exp / miso_det_log, IEEE division, no atomics;
// tests/_exact_paired_compare_ref.py restates it operation by operation (tests/test_gpu_exact_paired_compare.py).
//
// WHERE THE PIECES LIVE.  B's CDF at an argument, the lane-order sum, the verdict o[0 .. 4], the end of a quadrature, the
// host's prior term and check of z: exact_compare.hpp, shared with kernels_exact_compare.hip.  Windows, tables, the LDS
// layout, c8 and the loader of an element: exact_paired.hpp.  The check of caller-given elements: kernels_exact_paired.hip
// (exact_paired_check).  The driver's stream, buffers and events: hip_host.hpp.  exact_uni, a pair's side and the rows' sizes:
// exact_paired_pair.hpp, shared with kernels_exact_paired_delta.hip.  Here: the pooled density's statistics, the order of the
// tables, the quadrature loop (one z at a time, A's f read from its global row) and the driver.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "batch.hpp"
#include "device.hpp"
#include "miso_amd.h"
#include "miso_detmath.h"

#include "exact_compare.hpp"
#include "exact_paired.hpp"
#include "exact_paired_pair.hpp"
#include "hip_host.hpp"

namespace miso {

// One workgroup = one wavefront = pair first + blockIdx.x.  out: 5 + n_z doubles per pair; frow: EXPC_ROW doubles per
// workgroup of the launch (unused, and may be null, when n_z = 0).
__global__ __launch_bounds__(64) void exact_paired_compare(const ExactPairedCmpSide s1, const ExactPairedCmpSide s2, const int32_t *list,
                                                           const double *log_prior0, int first, int n, const double *z, int n_z,
                                                           double *out, double *frow) {
  __shared__ ExactPairedLds L;
  const int lane = threadIdx.x;
  const int i = first + static_cast<int>(blockIdx.x);
  if (i >= n) return;   // (uniform: the whole workgroup)
  ExactStats st1, st2; double c81, c82; ExactPairs pr1, pr2;
  exact_paired_cmp_side(s1, list, i, st1, c81, pr1);
  exact_paired_cmp_side(s2, list, i, st2, c82, pr2);
  const double *q1 = s1.stats6 + 6 * static_cast<size_t>(i), *q2 = s2.stats6 + 6 * static_cast<size_t>(i);
  // the pooled density: exponents, hyperparameters h1 + h2 - 1 and c = (a + b) - (n1 + n2) in st12, whose n, e0, e1 are sample
  // 1's; sample 2's pair count, A and pairs are the second segment
  const double hm0 = ((q1[4] + q2[4]) - 1.0) - 1.0, hm1 = ((q1[5] + q2[5]) - 1.0) - 1.0;
  const double n12 = st1.n + st2.n;
  ExactStats st12 = exact_stats(q1[0] + q2[0], q1[1] + q2[1], n12, st1.e0, st1.e1, hm0, hm1);
  st12.n = st1.n;
  st12 = exact_uni(st12);
  const ExactSecondSegment seg2{st2.n, st2.e0, st2.e1, pr2};
  const double c812 = exact_uni(exact_paired_c8(n12, hm0, hm1));

  const ExactTable W1 = exact_uni(exact_paired_window(st1, c81, pr1, L.mbuf, L.red, L.redi, lane));
  const ExactTable W2 = exact_uni(exact_paired_window(st2, c82, pr2, L.mbuf, L.red, L.redi, lane));
  const double w1 = exact_point(st1, W1.tR).x - exact_point(st1, W1.tL).x;
  const double w2 = exact_point(st2, W2.tR).x - exact_point(st2, W2.tL).x;
  const bool a2 = exact_uni(w2) < exact_uni(w1);   // A = sample 2
  const ExactStats stA = a2 ? st2 : st1, stB = a2 ? st1 : st2;
  const ExactPairs prA = a2 ? pr2 : pr1, prB = a2 ? pr1 : pr2;
  const ExactTable TA = exact_uni(exact_paired_table(stA, a2 ? W2 : W1, prA, L.mbuf, L.F, L.f, L.fext, L.red, lane));   // (its scalars and f are used from here on)
  const int i0 = EXACT_CELLS * lane;
  double *row = frow + static_cast<size_t>(EXPC_ROW) * blockIdx.x;
  if (n_z > 0) {
    for (int j = 0; j < EXACT_CELLS; j++) row[64 * j + lane] = L.f[exact_idx(i0 + j)];
    if (lane == 63) row[EXACT_G] = L.f[exact_idx(EXACT_G)];
  }
  __syncthreads();
  const ExactTable W12 = exact_uni(exact_paired_window(st12, c812, pr1, L.mbuf, L.red, L.redi, lane, seg2));
  const ExactTable T12 = exact_uni(exact_paired_table(st12, W12, pr1, L.mbuf, L.F, L.f, L.fext, L.red, lane, seg2));
  __syncthreads();
  const ExactTable TB = exact_paired_table(stB, a2 ? W1 : W2, prB, L.mbuf, L.F, L.f, L.fext, L.red, lane);
  const ExactVerdict V = exact_verdict(TA, TB, T12, a2, log_prior0 + i);
  double *o = out + static_cast<size_t>(5 + n_z) * static_cast<size_t>(i);
  if (lane == 0) exact_verdict_store(V, TA, TB, a2, o);
  if (n_z <= 0) return;
  // the quadratures on A's grid, one z after the other (no unrolling over z: the tables' stages set this kernel's registers,
  // the quadratures are a hundredth of its time)
  const int n_own = EXACT_CELLS + (lane == 63 ? 1 : 0);   // the last lane owns the grid's last point too
#pragma unroll 1
  for (int k = 0; k < n_z; k++) {
    const double zk = z[k];
    double acc = 0.0;
#pragma unroll 1
    for (int j = 0; j < n_own; j++) {
      const int pt = i0 + j;
      const ExactPoint p = exact_point(stA, TA.tL + TA.h * static_cast<double>(pt));
      const double fa = j < EXACT_CELLS ? row[64 * j + lane] : row[EXACT_G];
      const double wf = ((pt == 0 || pt == EXACT_G) ? 0.5 : 1.0) * fa;
      const double val = a2 ? exact_cdf_at(TB, p.x + zk, p.y - zk) : exact_cdf_at(TB, p.x - zk, p.y + zk);
      acc = acc + wf * (val / TB.Z);
    }
    exact_delta_cdf(acc, TA, a2, L.red, lane, o + 5 + k);
  }
}

// side[s]: stats6 (host), n rows; then EITHER m / offs (host: the selftest's caller-given probabilities, validated here) OR
// src (device pointers of a batch) with list (host, n event indices, the same for both samples).
void exact_paired_compare_run(const ExactPairedCmpInput &in1, const ExactPairedCmpInput &in2, const int32_t *list, int n, const double *z,
                              int n_z, double *out, hipStream_t st, float *ms) {
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device");
  if (n < 0) MISO_FAIL(MISO_EINVAL, "Negative pair count");
  exact_check_z(z, n_z);
  const ExactPairedCmpInput *in[2] = {&in1, &in2};
  int64_t n_pairs[2];
  for (int s = 0; s < 2; s++) n_pairs[s] = exact_paired_check(in[s]->stats6, in[s]->m, in[s]->m ? in[s]->offs : nullptr, n);
  std::vector<double> lp(std::max(n, 1));
  for (int i = 0; i < n; i++) lp[i] = exact_log_prior0(in1.stats6 + 6 * static_cast<size_t>(i) + 4, in2.stats6 + 6 * static_cast<size_t>(i) + 4);
  if (ms) *ms = 0.f;
  if (n == 0) return;
  HipCall call(st);
  ExactPairedCmpSide side[2];
  for (int s = 0; s < 2; s++) side[s] = exact_paired_cmp_upload(call, *in[s], n, n_pairs[s]);
  const int32_t *d_list = (in1.m && in2.m) ? nullptr : call.upload(list, static_cast<size_t>(n) * 4);
  const double *d_lp = call.upload(lp.data(), static_cast<size_t>(n) * 8), *d_z = call.upload(z, static_cast<size_t>(n_z) * 8);
  const size_t ob = static_cast<size_t>(n) * (5 + n_z) * 8;
  double *d_o = call.alloc(ob);
  double *d_row = n_z ? call.alloc(static_cast<size_t>(std::min(n, EXPC_LAUNCH)) * EXPC_ROW * 8) : nullptr;
  call.start();
  for (int first = 0; first < n; first += EXPC_LAUNCH) {   // (one stream: a launch's rows are free when the next begins)
    const int cnt = std::min(n - first, EXPC_LAUNCH);
    hipLaunchKernelGGL(exact_paired_compare, dim3(cnt), dim3(64), 0, call.st, side[0], side[1], d_list, d_lp, first, n, d_z, n_z, d_o, d_row);
    HIP_OK(hipGetLastError());
  }
  call.stop();
  HIP_OK(hipMemcpyAsync(out, d_o, ob, hipMemcpyDeviceToHost, call.st));
  HIP_OK(hipStreamSynchronize(call.st));
  if (ms) *ms = call.elapsed_ms();
}

}  // namespace miso
