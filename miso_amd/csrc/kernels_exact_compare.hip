// kernels_exact_compare.hip -- two exact-mode posteriors of one event compared without a draw (miso_batch_compare_exact,
// DESIGN.md 16).
//
// Sample i's posterior of x = psi_0 is p_i(x) = x^am1_i (1 - x)^bm1_i / (x e0 + (1 - x) e1)^n_i / Z_i (kernels_exact.hip).  The
// effective lengths are the gene's, the same in both samples, so p_1 p_2 is of the same family: the POOLED statistics
// n10 = n10_1 + n10_2, n01 = n01_1 + n01_2, n = n_1 + n_2, h = h_1 + h_2 - 1 (again >= 1).  The density of
// delta = psi_1 - psi_2 at 0 is a ratio of three normalisers the table stage already computes,
//     d0 = Z12 / (Z1 Z2),   log Z = gmax + log(F[G]),   log_d0 = ((lZ12 - lZ1) - lZ2),
// and the Savage-Dickey Bayes factor is prior0 / d0, log prior0 from the host (std::lgamma of the hyperparameters; 0 at
// MISO's default h = (1, 1)): log_bf = log_prior0 - log_d0, bayes_factor = min(exp(log_bf), 1e12), log10_bf uncapped.
//
// THE CDF OF DELTA at z: H(z) = P(psi_1 - psi_2 <= z) = integral of p_A(x) (CDF of the other posterior, B, at the shifted
// argument) dx.  A is the posterior with the NARROWER window in psi, x(tR) - x(tL); a tie goes to sample 1 (on the wider
// one's grid the narrow CDF is a step between two points).  The integral is the trapezoid sum over A's 2049 points with the
// weights w_k f_A(t_k) / sum w f_A in the mean's summation order -- a lane's own points in order, then the lanes in
// order --, A's f recomputed from exact_point, so that ONE table is in LDS at a time: B's, read through the cubic
// Hermite interpolant of F on the cell of logit(argument) (exact_invert solves the same cubic), 0 / Z where the argument
// leaves (0, 1) or B's window.  The argument and one minus it are both formed from exact_point's x and 1 - x, each with
// its own relative precision.  A = sample 2: H = sum w F_1(y + z) / Z_1; A = sample 1: H = 1 - sum w F_2(x - z) / Z_2.
//
// ONE WAVEFRONT = one workgroup per pair: windows of both, table of A (its scalars are kept), table of the pooled
// posterior (Z12, gmax12), table of B, which stays for the n_z quadratures.  f64, no contraction, miso_det_exp /
// miso_det_log, IEEE division; tests/_exact_compare_ref.py restates it operation by operation and the two agree bit for bit
// (tests/test_gpu_exact_compare.py).
//
// WHERE THE PIECES LIVE.  What this comparison and the paired-end one (kernels_exact_paired_compare.hip) do alike -- B's CDF
// at an argument, the lane-order sum, the verdict o[0 .. 4], the end of a quadrature, the host's prior term and check of z --
// is exact_compare.hpp; the tables are exact_posterior.hpp's; the driver's stream, buffers and events hip_host.hpp's.  Here:
// the order of the three tables, the quadrature loop (unrolled over z, A's f made again from scalars) and the driver.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "batch.hpp"
#include "device.hpp"
#include "miso_amd.h"
#include "miso_detmath.h"

#include "exact_compare.hpp"
#include "hip_host.hpp"

namespace miso {

// One workgroup = one wavefront = one pair.  stats7_i: {n10, n01, n, e0, e1, h0, h1} of sample i; out: 5 + n_z doubles per pair
__global__ __launch_bounds__(64) void exact_compare(const double *stats7_1, const double *stats7_2, const double *log_prior0, int n,
                                                    const double *z, int n_z, double *out) {
  __shared__ double F[EXACT_PAD], f[EXACT_PAD], red[256];
  const int lane = threadIdx.x;
  const int i = blockIdx.x;
  if (i >= n) return;   // (uniform: the whole workgroup)
  const double *q1 = stats7_1 + 7 * static_cast<size_t>(i), *q2 = stats7_2 + 7 * static_cast<size_t>(i);
  const ExactStats st1 = exact_stats(q1[0], q1[1], q1[2], q1[3], q1[4], q1[5] - 1.0, q1[6] - 1.0);
  const ExactStats st2 = exact_stats(q2[0], q2[1], q2[2], q1[3], q1[4], q2[5] - 1.0, q2[6] - 1.0);
  const ExactStats st12 = exact_stats(q1[0] + q2[0], q1[1] + q2[1], q1[2] + q2[2], q1[3], q1[4],
                                      ((q1[5] + q2[5]) - 1.0) - 1.0, ((q1[6] + q2[6]) - 1.0) - 1.0);
  const ExactTable W1 = exact_window(st1, lane), W2 = exact_window(st2, lane);
  const double w1 = exact_point(st1, W1.tR).x - exact_point(st1, W1.tL).x;
  const double w2 = exact_point(st2, W2.tR).x - exact_point(st2, W2.tL).x;
  const bool a2 = w2 < w1;   // A = sample 2
  const ExactStats stA = a2 ? st2 : st1, stB = a2 ? st1 : st2;
  const ExactTable TA = exact_table(stA, a2 ? W2 : W1, F, f, red, lane);   // (only its scalars are used from here on)
  __syncthreads();
  const ExactTable T12 = exact_tabulate(st12, F, f, red, lane);
  __syncthreads();
  const ExactTable TB = exact_table(stB, a2 ? W1 : W2, F, f, red, lane);
  const ExactVerdict V = exact_verdict(TA, TB, T12, a2, log_prior0 + i);
  double *o = out + static_cast<size_t>(5 + n_z) * static_cast<size_t>(i);
  if (lane == 0) exact_verdict_store(V, TA, TB, a2, o);
  if (n_z <= 0) return;
  // the quadratures on A's grid, all n_z of them from one evaluation of A's points
  double acc[EXACT_MAX_Z];
#pragma unroll
  for (int k = 0; k < EXACT_MAX_Z; k++) acc[k] = 0.0;
  const int i0 = EXACT_CELLS * lane;
  const int n_own = EXACT_CELLS + (lane == 63 ? 1 : 0);   // the last lane owns the grid's last point too
  for (int j = 0; j < n_own; j++) {
    const int pt = i0 + j;
    const ExactPoint p = exact_point(stA, TA.tL + TA.h * static_cast<double>(pt));
    const double wf = ((pt == 0 || pt == EXACT_G) ? 0.5 : 1.0) * miso_det_exp(p.g - TA.gmax);
#pragma unroll
    for (int k = 0; k < EXACT_MAX_Z; k++) {
      if (k < n_z) {
        const double zk = z[k];
        const double val = a2 ? exact_cdf_at(TB, p.x + zk, p.y - zk) : exact_cdf_at(TB, p.x - zk, p.y + zk);
        acc[k] = acc[k] + wf * (val / TB.Z);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < EXACT_MAX_Z; k++) {
    if (k < n_z) exact_delta_cdf(acc[k], TA, a2, red, lane, o + 5 + k);
  }
}

// (st: the stream to work on -- a batch's own; null: one of this call's.  ms, may be null: the kernel's HIP-event time)
void exact_compare_run(const double *stats7_1, const double *stats7_2, int n, const double *z, int n_z, double *out, hipStream_t st,
                       float *ms) {
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device");
  if (n < 0) MISO_FAIL(MISO_EINVAL, "Negative pair count");
  exact_check_z(z, n_z);
  std::vector<double> lp(std::max(n, 1));
  for (int i = 0; i < n; i++) {
    const double *q1 = stats7_1 + 7 * static_cast<size_t>(i), *q2 = stats7_2 + 7 * static_cast<size_t>(i);
    if (std::memcmp(q1 + 3, q2 + 3, 2 * sizeof(double)) != 0)
      MISO_FAIL(MISO_EINVAL, "The effective lengths of a pair to compare differ between its samples");
    if (!exact_eligible(false, 2, q1 + 3, q1 + 5) || !exact_eligible(false, 2, q2 + 3, q2 + 5))
      MISO_FAIL(MISO_EINVAL, "A pair to compare is not eligible for the exact-posterior mode");
    lp[i] = exact_log_prior0(q1 + 5, q2 + 5);
  }
  if (ms) *ms = 0.f;
  if (n == 0) return;
  HipCall call(st);
  const size_t sb = static_cast<size_t>(n) * 7 * 8, ob = static_cast<size_t>(n) * (5 + n_z) * 8;
  const double *d_1 = call.upload(stats7_1, sb), *d_2 = call.upload(stats7_2, sb);
  const double *d_lp = call.upload(lp.data(), static_cast<size_t>(n) * 8), *d_z = call.upload(z, static_cast<size_t>(n_z) * 8);
  double *d_o = call.alloc(ob);
  call.start();
  hipLaunchKernelGGL(exact_compare, dim3(n), dim3(64), 0, call.st, d_1, d_2, d_lp, n, d_z, n_z, d_o);
  HIP_OK(hipGetLastError());
  call.stop();
  HIP_OK(hipMemcpyAsync(out, d_o, ob, hipMemcpyDeviceToHost, call.st));
  HIP_OK(hipStreamSynchronize(call.st));
  if (ms) *ms = call.elapsed_ms();
}

}  // namespace miso
