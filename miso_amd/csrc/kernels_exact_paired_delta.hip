// kernels_exact_paired_delta.hip -- quantiles of delta psi = psi_1 - psi_2 of two paired-end exact-mode posteriors of one
// event, from the exact CDF and without a draw (miso_batch_exact_delta_quantiles on paired-end batches).
//
// H(z) = P(psi_1 - psi_2 <= z) is kernels_exact_paired_compare.hip's: A is the posterior with the narrower window in psi (a
// tie: sample 1), the trapezoid sum over A's 2049 points of w f_A / sum w f_A times B's tabulated CDF at the shifted argument,
// A's f kept in the workgroup's row of a global buffer (point j of lane l at [64 j + l]) -- the same operations in the same
// order, so the same bits as exact_paired_compare's cdf at the same z.  The points are this kernel's own (exact_delta.hpp):
// H(0.0), then five rounds of eight inside the bracket, the first round once for all probabilities, then one linear
// interpolation.  Eight points share one sweep over A's points: exact_point and the row's read are made once for the eight.
//
// ONE WAVEFRONT = one workgroup per pair, ExactPairedLds's 37 KB holding one F / f pair at a time: windows of both samples,
// table of A (scalars kept, own f to the row), table of B, which stays in LDS.  No pooled density: the Bayes factor is
// exact_paired_compare's business.  f64, no contraction, miso_det_exp / miso_det_log, IEEE division, no atomics;
// tests/_exact_delta_ref.py restates it operation by operation (tests/test_gpu_exact_paired_delta.py).
//
// WHERE THE PIECES LIVE.  The sweep, the bracket's update, the interpolation, the host's check of p: exact_delta.hpp, shared
// with kernels_exact_delta.hip.  B's CDF at an argument and the lane-order sum: exact_compare.hpp.  Windows, tables, the LDS
// layout: exact_paired.hpp.  exact_uni, a pair's side, the rows' sizes: exact_paired_pair.hpp.  The check of caller-given
// elements: kernels_exact_paired.hip (exact_paired_check).  Here: the order of the tables and the driver.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "batch.hpp"
#include "device.hpp"
#include "miso_amd.h"
#include "miso_detmath.h"

#include "exact_delta.hpp"
#include "exact_paired.hpp"
#include "exact_paired_pair.hpp"
#include "hip_host.hpp"

namespace miso {

// One workgroup = one wavefront = pair first + blockIdx.x.  out: n_p + 1 doubles per pair; frow: EXPC_ROW doubles per
// workgroup of the launch.
__global__ __launch_bounds__(64) void exact_paired_delta_quantiles(const ExactPairedCmpSide s1, const ExactPairedCmpSide s2,
                                                                   const int32_t *list, int first, int n, const double *prob, int n_p,
                                                                   double *out, double *frow) {
  __shared__ ExactPairedLds L;
  const int lane = threadIdx.x;
  const int i = first + static_cast<int>(blockIdx.x);
  if (i >= n) return;   // (uniform: the whole workgroup)
  ExactStats st1, st2; double c81, c82; ExactPairs pr1, pr2;
  exact_paired_cmp_side(s1, list, i, st1, c81, pr1);
  exact_paired_cmp_side(s2, list, i, st2, c82, pr2);
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
  for (int j = 0; j < EXACT_CELLS; j++) row[64 * j + lane] = L.f[exact_idx(i0 + j)];
  if (lane == 63) row[EXACT_G] = L.f[exact_idx(EXACT_G)];
  __syncthreads();
  const ExactTable TB = exact_paired_table(stB, a2 ? W1 : W2, prB, L.mbuf, L.F, L.f, L.fext, L.red, lane);
  // (a lane reads back what it wrote itself: no fence between the row's stores and its loads)
  const auto weight = [&](int j, int, const ExactPoint &) __attribute__((always_inline)) { return j < EXACT_CELLS ? row[64 * j + lane] : row[EXACT_G]; };
  exact_delta_search(
      prob, n_p, out + static_cast<size_t>(n_p + 1) * static_cast<size_t>(i), lane,
      [&](const double (&z)[1], double (&H)[1]) __attribute__((always_inline)) { exact_delta_sweep<1>(stA, TA, TB, a2, z, H, L.red, lane, weight); },
      [&](const double (&z)[EXACT_DELTA_PTS], double (&H)[EXACT_DELTA_PTS]) __attribute__((always_inline)) {
        exact_delta_sweep<EXACT_DELTA_PTS>(stA, TA, TB, a2, z, H, L.red, lane, weight);
      });
}

// in1, in2, list: as exact_paired_compare_run's.  out: n_p + 1 doubles per pair
void exact_paired_delta_run(const ExactPairedCmpInput &in1, const ExactPairedCmpInput &in2, const int32_t *list, int n, const double *p,
                            int n_p, double *out, hipStream_t st, float *ms) {
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device");
  if (n < 0) MISO_FAIL(MISO_EINVAL, "Negative pair count");
  exact_delta_check_p(p, n_p);
  const ExactPairedCmpInput *in[2] = {&in1, &in2};
  int64_t n_pairs[2];
  for (int s = 0; s < 2; s++) n_pairs[s] = exact_paired_check(in[s]->stats6, in[s]->m, in[s]->m ? in[s]->offs : nullptr, n);
  if (ms) *ms = 0.f;
  if (n == 0) return;
  HipCall call(st);
  ExactPairedCmpSide side[2];
  for (int s = 0; s < 2; s++) side[s] = exact_paired_cmp_upload(call, *in[s], n, n_pairs[s]);
  const int32_t *d_list = (in1.m && in2.m) ? nullptr : call.upload(list, static_cast<size_t>(n) * 4);
  const double *d_p = call.upload(p, static_cast<size_t>(n_p) * 8);
  const size_t ob = static_cast<size_t>(n) * (n_p + 1) * 8;
  double *d_o = call.alloc(ob);
  double *d_row = call.alloc(static_cast<size_t>(std::min(n, EXPC_LAUNCH)) * EXPC_ROW * 8);
  call.start();
  for (int first = 0; first < n; first += EXPC_LAUNCH) {   // (one stream: a launch's rows are free when the next begins)
    const int cnt = std::min(n - first, EXPC_LAUNCH);
    hipLaunchKernelGGL(exact_paired_delta_quantiles, dim3(cnt), dim3(64), 0, call.st, side[0], side[1], d_list, first, n, d_p, n_p, d_o, d_row);
    HIP_OK(hipGetLastError());
  }
  call.stop();
  HIP_OK(hipMemcpyAsync(out, d_o, ob, hipMemcpyDeviceToHost, call.st));
  HIP_OK(hipStreamSynchronize(call.st));
  if (ms) *ms = call.elapsed_ms();
}

}  // namespace miso
