// kernels_exact_delta.hip -- quantiles of delta psi = psi_1 - psi_2 of two exact-mode posteriors of one event, from the exact
// CDF and without a draw (miso_batch_exact_delta_quantiles).
//
// H(z) = P(psi_1 - psi_2 <= z) is kernels_exact_compare.hip's: A is the posterior with the narrower window in psi (a tie:
// sample 1), the trapezoid sum over A's 2049 points of w f_A / sum w f_A times B's tabulated CDF at the shifted argument
// (exact_cdf_at), the lanes added in lane order (exact_lanes_sum) over TA.sf, a2 ? s : 1 - s -- the same operations in the same
// order, so the same bits as exact_compare's cdf at the same z.  That kernel takes its points from the caller; this one chooses
// them itself until H(z) = p is solved (exact_delta.hpp): H(0.0), then five rounds of eight points inside the bracket -- the
// first round, on (-1, 1), once for all probabilities --, then one linear interpolation.  1 + 8 + 32 n_p evaluations of H.
//
// ONE WAVEFRONT = one workgroup per pair: windows of both samples, table of A (its scalars are kept, its f is made again from
// exact_point in every sweep), table of B, which stays in LDS -- one F / f pair at a time, and no pooled table: the Bayes factor
// is exact_compare's business.  f64, no contraction, miso_det_exp / miso_det_log, IEEE division, no atomics;
// tests/_exact_delta_ref.py restates it operation by operation and the two agree bit for bit (tests/test_gpu_exact_delta.py).
//
// WHERE THE PIECES LIVE.  The sweep, the bracket's update, the interpolation, the host's check of p: exact_delta.hpp, shared
// with kernels_exact_paired_delta.hip.  B's CDF at an argument and the lane-order sum: exact_compare.hpp.  The tables:
// exact_posterior.hpp.  The driver's stream, buffers and events: hip_host.hpp.  Here: the order of the tables and the driver.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "batch.hpp"
#include "device.hpp"
#include "miso_amd.h"
#include "miso_detmath.h"

#include "exact_delta.hpp"
#include "hip_host.hpp"

namespace miso {

// One workgroup = one wavefront = one pair.  stats7_i: {n10, n01, n, e0, e1, h0, h1} of sample i; out: n_p + 1 doubles per pair
__global__ __launch_bounds__(64) void exact_delta_quantiles(const double *stats7_1, const double *stats7_2, int n, const double *prob,
                                                            int n_p, double *out) {
  __shared__ double F[EXACT_PAD], f[EXACT_PAD], red[256];
  const int lane = threadIdx.x;
  const int i = blockIdx.x;
  if (i >= n) return;   // (uniform: the whole workgroup)
  const double *q1 = stats7_1 + 7 * static_cast<size_t>(i), *q2 = stats7_2 + 7 * static_cast<size_t>(i);
  const ExactStats st1 = exact_stats(q1[0], q1[1], q1[2], q1[3], q1[4], q1[5] - 1.0, q1[6] - 1.0);
  const ExactStats st2 = exact_stats(q2[0], q2[1], q2[2], q1[3], q1[4], q2[5] - 1.0, q2[6] - 1.0);
  const ExactTable W1 = exact_window(st1, lane), W2 = exact_window(st2, lane);
  const double w1 = exact_point(st1, W1.tR).x - exact_point(st1, W1.tL).x;
  const double w2 = exact_point(st2, W2.tR).x - exact_point(st2, W2.tL).x;
  const bool a2 = w2 < w1;   // A = sample 2
  const ExactStats stA = a2 ? st2 : st1, stB = a2 ? st1 : st2;
  const ExactTable TA = exact_table(stA, a2 ? W2 : W1, F, f, red, lane);   // (only its scalars are used from here on)
  __syncthreads();
  const ExactTable TB = exact_table(stB, a2 ? W1 : W2, F, f, red, lane);
  const auto weight = [&](int, int, const ExactPoint &p) __attribute__((always_inline)) { return miso_det_exp(p.g - TA.gmax); };
  exact_delta_search(
      prob, n_p, out + static_cast<size_t>(n_p + 1) * static_cast<size_t>(i), lane,
      [&](const double (&z)[1], double (&H)[1]) __attribute__((always_inline)) { exact_delta_sweep<1>(stA, TA, TB, a2, z, H, red, lane, weight); },
      [&](const double (&z)[EXACT_DELTA_PTS], double (&H)[EXACT_DELTA_PTS]) __attribute__((always_inline)) {
        exact_delta_sweep<EXACT_DELTA_PTS>(stA, TA, TB, a2, z, H, red, lane, weight);
      });
}

// (st: the stream to work on -- a batch's own; null: one of this call's.  ms, may be null: the kernel's HIP-event time)
void exact_delta_run(const double *stats7_1, const double *stats7_2, int n, const double *p, int n_p, double *out, hipStream_t st,
                     float *ms) {
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device");
  if (n < 0) MISO_FAIL(MISO_EINVAL, "Negative pair count");
  exact_delta_check_p(p, n_p);
  for (int i = 0; i < n; i++) {
    const double *q1 = stats7_1 + 7 * static_cast<size_t>(i), *q2 = stats7_2 + 7 * static_cast<size_t>(i);
    if (std::memcmp(q1 + 3, q2 + 3, 2 * sizeof(double)) != 0)
      MISO_FAIL(MISO_EINVAL, "The effective lengths of a pair to compare differ between its samples");
    if (!exact_eligible(false, 2, q1 + 3, q1 + 5) || !exact_eligible(false, 2, q2 + 3, q2 + 5))
      MISO_FAIL(MISO_EINVAL, "A pair to compare is not eligible for the exact-posterior mode");
  }
  if (ms) *ms = 0.f;
  if (n == 0) return;
  HipCall call(st);
  const size_t sb = static_cast<size_t>(n) * 7 * 8, ob = static_cast<size_t>(n) * (n_p + 1) * 8;
  const double *d_1 = call.upload(stats7_1, sb), *d_2 = call.upload(stats7_2, sb);
  const double *d_p = call.upload(p, static_cast<size_t>(n_p) * 8);
  double *d_o = call.alloc(ob);
  call.start();
  hipLaunchKernelGGL(exact_delta_quantiles, dim3(n), dim3(64), 0, call.st, d_1, d_2, n, d_p, n_p, d_o);
  HIP_OK(hipGetLastError());
  call.stop();
  HIP_OK(hipMemcpyAsync(out, d_o, ob, hipMemcpyDeviceToHost, call.st));
  HIP_OK(hipStreamSynchronize(call.st));
  if (ms) *ms = call.elapsed_ms();
}

}  // namespace miso
