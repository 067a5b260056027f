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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "batch.hpp"
#include "device.hpp"
#include "miso_amd.h"
#include "miso_detmath.h"

#include "exact_posterior.hpp"

namespace miso {

constexpr int EXACT_MAX_Z = 8;
constexpr double EXACT_BF_CAP = 1e12;
constexpr double EXACT_LN10 = 2.302585092994046;

// the tabulated, unnormalised CDF at psi = u; v = 1 - psi, computed on its own
__device__ __forceinline__ double exact_cdf_at(const ExactTable &T, double u, double v) {
  const bool uin = u > 0.0, vin = v > 0.0;
  const double t = miso_det_log(uin ? u : 1.0) - miso_det_log(vin ? v : 1.0);
  double s = (t - T.tL) / T.h;
  s = s > 0.0 ? s : 0.0;
  s = s < static_cast<double>(EXACT_G) ? s : static_cast<double>(EXACT_G);
  int j = static_cast<int>(s);
  j = j < EXACT_G - 1 ? j : EXACT_G - 1;   // 0 .. G - 1
  const double fr = s - static_cast<double>(j);
  const double F0 = T.F[exact_idx(j)], F1 = T.F[exact_idx(j + 1)];
  const double m0 = T.h * T.f[exact_idx(j)], m1 = T.h * T.f[exact_idx(j + 1)];
  const double dF = F1 - F0;
  const double c2 = (3.0 * dF - 2.0 * m0) - m1, c3 = (m0 + m1) - 2.0 * dF;
  double val = F0 + (m0 + fr * (c2 + fr * c3)) * fr;
  val = val > T.Z ? T.Z : val;
  val = val < 0.0 ? 0.0 : val;
  val = t >= T.tR ? T.Z : val;
  val = uin ? val : 0.0;
  val = vin ? val : T.Z;
  return val;
}

// the 64 lanes' values added in lane order (red: 64 doubles of LDS)
__device__ __forceinline__ double exact_lanes_sum(double v, double *red, int lane) {
  red[lane] = v;
  __syncthreads();
  double s = 0.0;
  for (int m = 0; m < 64; m++) s = s + red[m];
  __syncthreads();
  return s;
}

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
  const double lzA = TA.gmax + miso_det_log(TA.Z), lzB = TB.gmax + miso_det_log(TB.Z), lz12 = T12.gmax + miso_det_log(T12.Z);
  const double lz1 = a2 ? lzB : lzA, lz2 = a2 ? lzA : lzB;
  const double log_d0 = (lz12 - lz1) - lz2;
  const double log_bf = log_prior0[i] - log_d0;
  double bf = miso_det_exp(log_bf);
  bf = bf > EXACT_BF_CAP ? EXACT_BF_CAP : bf;
  double *o = out + static_cast<size_t>(5 + n_z) * static_cast<size_t>(i);
  if (lane == 0) {
    o[0] = a2 ? TB.mean0 : TA.mean0; o[1] = a2 ? TA.mean0 : TB.mean0;
    o[2] = log_d0; o[3] = bf; o[4] = log_bf / EXACT_LN10;
  }
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
    if (k < n_z) {
      const double s = exact_lanes_sum(acc[k], red, lane) / TA.sf;
      if (lane == 0) o[5 + k] = a2 ? s : 1.0 - s;
    }
  }
}

#define HIP_OK(call)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess)                                                                  \
      MISO_FAIL(MISO_ENODEVICE, std::string(#call) + ": " + hipGetErrorString(e_));        \
  } while (0)

// log of the prior density of psi_1 - psi_2 at 0: the Beta normalisers of the pooled hyperparameters over the two samples'
static double exact_log_prior0(const double *q1, const double *q2) {
  const double h0p = (q1[5] + q2[5]) - 1.0, h1p = (q1[6] + q2[6]) - 1.0;
  double lp = (std::lgamma(h0p) + std::lgamma(h1p)) - std::lgamma(h0p + h1p);
  for (const double *q : {q1, q2}) lp = lp - ((std::lgamma(q[5]) + std::lgamma(q[6])) - std::lgamma(q[5] + q[6]));
  return lp;
}

// (st: the stream to work on -- a batch's own; null: one of this call's.  ms, may be null: the kernel's HIP-event time)
void exact_compare_run(const double *stats7_1, const double *stats7_2, int n, const double *z, int n_z, double *out, hipStream_t st,
                       float *ms) {
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device");
  if (n < 0) MISO_FAIL(MISO_EINVAL, "Negative pair count");
  if (n_z < 0 || n_z > EXACT_MAX_Z) MISO_FAIL(MISO_EINVAL, "The number of delta psi points must lie in [0, 8]");
  for (int j = 0; j < n_z; j++) if (!(z[j] > -1.0 && z[j] < 1.0)) MISO_FAIL(MISO_EINVAL, "A delta psi point must lie inside (-1, 1)");
  std::vector<double> lp(std::max(n, 1));
  for (int i = 0; i < n; i++) {
    const double *q1 = stats7_1 + 7 * static_cast<size_t>(i), *q2 = stats7_2 + 7 * static_cast<size_t>(i);
    if (std::memcmp(q1 + 3, q2 + 3, 2 * sizeof(double)) != 0)
      MISO_FAIL(MISO_EINVAL, "The effective lengths of a pair to compare differ between its samples");
    if (!exact_eligible(false, 2, q1 + 3, q1 + 5) || !exact_eligible(false, 2, q2 + 3, q2 + 5))
      MISO_FAIL(MISO_EINVAL, "A pair to compare is not eligible for the exact-posterior mode");
    lp[i] = exact_log_prior0(q1, q2);
  }
  if (ms) *ms = 0.f;
  if (n == 0) return;
  struct Held {   // freed on every way out, a failed call's included
    double *p[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipStream_t own = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Held() {
      for (double *q : p) if (q) (void) hipFree(q);
      if (e0) (void) hipEventDestroy(e0);
      if (e1) (void) hipEventDestroy(e1);
      if (own) (void) hipStreamDestroy(own);
    }
  } held;
  if (!st) { HIP_OK(hipStreamCreateWithFlags(&held.own, hipStreamNonBlocking)); st = held.own; }
  double *&d_1 = held.p[0], *&d_2 = held.p[1], *&d_lp = held.p[2], *&d_z = held.p[3], *&d_o = held.p[4];
  const size_t sb = static_cast<size_t>(n) * 7 * 8, ob = static_cast<size_t>(n) * (5 + n_z) * 8;
  HIP_OK(hipMalloc(reinterpret_cast<void **>(&d_1), sb));
  HIP_OK(hipMalloc(reinterpret_cast<void **>(&d_2), sb));
  HIP_OK(hipMalloc(reinterpret_cast<void **>(&d_lp), static_cast<size_t>(n) * 8));
  HIP_OK(hipMalloc(reinterpret_cast<void **>(&d_z), EXACT_MAX_Z * 8));
  HIP_OK(hipMalloc(reinterpret_cast<void **>(&d_o), ob));
  HIP_OK(hipMemcpyAsync(d_1, stats7_1, sb, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_2, stats7_2, sb, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_lp, lp.data(), static_cast<size_t>(n) * 8, hipMemcpyHostToDevice, st));
  if (n_z) HIP_OK(hipMemcpyAsync(d_z, z, static_cast<size_t>(n_z) * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipEventCreate(&held.e0));
  HIP_OK(hipEventCreate(&held.e1));
  HIP_OK(hipEventRecord(held.e0, st));
  hipLaunchKernelGGL(exact_compare, dim3(n), dim3(64), 0, st, d_1, d_2, d_lp, n, d_z, n_z, d_o);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(held.e1, st));
  HIP_OK(hipMemcpyAsync(out, d_o, ob, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (ms) HIP_OK(hipEventElapsedTime(ms, held.e0, held.e1));
}

}  // namespace miso
