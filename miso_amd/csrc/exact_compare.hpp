// exact_compare.hpp -- "two exact posteriors compared" (DESIGN.md 16, 18): what kernels_exact_compare.hip (single-end) and
// kernels_exact_paired_compare.hip (paired-end) do alike once each has its three tables -- A's (the narrower window in psi),
// B's and the pooled density's.  Device part: B's tabulated CDF at an argument, the lane-order sum, the verdict (means, density
// of delta psi at 0, Bayes factor) and the end of one delta psi quadrature.  Host part: the prior term and the check of the
// delta psi points.  The quadrature loops themselves differ and stay in their units.  -ffp-contract=off; every operation in
// a fixed order: tests/_exact_compare_ref.py restates these functions, tests/_exact_paired_compare_ref.py imports them from
// there.  exact_delta.hpp (the quantiles of delta psi) builds its sweeps on exact_cdf_at and on exact_lanes_sum's
// order.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <initializer_list>

#include "host.hpp"
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

// The verdict from the three tables' scalars -- a2: A is sample 2; log_prior0: the pair's entry of the host's array --:
// log_d0 = (lZ12 - lZ1) - lZ2 with log Z = gmax + log(F[G]), log_bf = log_prior0 - log_d0, the Bayes factor capped.  Every
// lane computes it; lane 0 then writes o[0 .. 4] of the pair's output row with exact_verdict_store: the two means, log_d0, the
// capped Bayes factor, its log10 uncapped.  (Two functions and a pointer, not one function and a value: the compiler gives the
// single-end kernel other registers when the stores, or the prior's load, move ahead of the logarithms.)
struct ExactVerdict { double log_d0, bf, log_bf; };
__device__ __forceinline__ ExactVerdict exact_verdict(const ExactTable &TA, const ExactTable &TB, const ExactTable &T12, bool a2,
                                                      const double *log_prior0) {
  const double lzA = TA.gmax + miso_det_log(TA.Z), lzB = TB.gmax + miso_det_log(TB.Z), lz12 = T12.gmax + miso_det_log(T12.Z);
  const double lz1 = a2 ? lzB : lzA, lz2 = a2 ? lzA : lzB;
  const double log_d0 = (lz12 - lz1) - lz2;
  const double log_bf = *log_prior0 - log_d0;
  double bf = miso_det_exp(log_bf);
  bf = bf > EXACT_BF_CAP ? EXACT_BF_CAP : bf;
  return ExactVerdict{log_d0, bf, log_bf};
}
__device__ __forceinline__ void exact_verdict_store(const ExactVerdict &V, const ExactTable &TA, const ExactTable &TB, bool a2, double *o) {
  o[0] = a2 ? TB.mean0 : TA.mean0; o[1] = a2 ? TA.mean0 : TB.mean0;
  o[2] = V.log_d0; o[3] = V.bf; o[4] = V.log_bf / EXACT_LN10;
}

// The end of one quadrature on A's grid: acc, the lane's sum of w f_A (F_B(argument) / Z_B), to H(z) = P(psi_1 - psi_2 <= z) at *h
__device__ __forceinline__ void exact_delta_cdf(double acc, const ExactTable &TA, bool a2, double *red, int lane, double *h) {
  const double s = exact_lanes_sum(acc, red, lane) / TA.sf;
  if (lane == 0) *h = a2 ? s : 1.0 - s;
}

// log of the prior density of psi_1 - psi_2 at 0: the Beta normalisers of the pooled hyperparameters over the two samples'
// (h_i: {h0, h1} of sample i)
inline double exact_log_prior0(const double *h_1, const double *h_2) {
  const double h0p = (h_1[0] + h_2[0]) - 1.0, h1p = (h_1[1] + h_2[1]) - 1.0;
  double lp = (std::lgamma(h0p) + std::lgamma(h1p)) - std::lgamma(h0p + h1p);
  for (const double *h : {h_1, h_2}) lp = lp - ((std::lgamma(h[0]) + std::lgamma(h[1])) - std::lgamma(h[0] + h[1]));
  return lp;
}

// the delta psi points of a comparison
inline void exact_check_z(const double *z, int n_z) {
  if (n_z < 0 || n_z > EXACT_MAX_Z) MISO_FAIL(MISO_EINVAL, "The number of delta psi points must lie in [0, 8]");
  for (int j = 0; j < n_z; j++) if (!(z[j] > -1.0 && z[j] < 1.0)) MISO_FAIL(MISO_EINVAL, "A delta psi point must lie inside (-1, 1)");
}

}  // namespace miso
