// compare_column.hpp -- the two-sample comparison of one (event, isoform) column pair, shared by compare_kernel
// (kernels_summary.hip) and compare_groups_kernel (kernels_compare_groups.hip): one text, so that the group pass gives the
// pairwise call's bits.
//
// compare_miso per (event, isoform) (misopy/hypothesis_test.py:89-179, 348-380): index-paired
// delta_s = psi1_s - psi2_s; if mean|delta| <= 0.009 or all deltas are identical the posterior is
// "null peaked" (density inf at 0 -> Bayes factor 0); otherwise a Gaussian kernel density estimate
// with covariance factor 0.3 (bandwidth^2 = 0.09 * unbiased variance, scipy.stats.gaussian_kde
// evaluated at 0) and Savage-Dickey BF = prior(0) / posterior(0) = 1 / posterior(0), 1e12 when the
// posterior density underflows to 0, capped at 1e12.  All sums use the fixed 256-strided + binary
// tree order of summarize_column so a CPU checker can reproduce them.
#pragma once
#include <hip/hip_runtime.h>

#include "miso_detmath.h"

namespace miso {

constexpr int SUMMARY_CACHE = 32;   // samples per thread held in registers (S <= 8192)

__device__ __forceinline__ double block_tree_sum(double v, double *part) {
  const int t = threadIdx.x;
  __syncthreads();
  part[t] = v;
  __syncthreads();
  for (int stride = 128; stride >= 1; stride >>= 1) {
    if (t < stride) part[t] = part[t] + part[t + stride];
    __syncthreads();
  }
  return part[0];
}

// four sums at once, each in block_tree_sum's order (same bits), one set of barriers
__device__ __forceinline__ void block_tree_sum4(double (&v)[4], double (*part4)[256]) {
  const int t = threadIdx.x;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; q++) part4[q][t] = v[q];
  __syncthreads();
  for (int stride = 128; stride >= 1; stride >>= 1) {
    if (t < stride) {
#pragma unroll
      for (int q = 0; q < 4; q++) part4[q][t] = part4[q][t] + part4[q][t + stride];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 4; q++) v[q] = part4[q][0];
}

// A column known to lie in global memory: a pointer that was itself loaded from memory is a flat one to the compiler, and
// 64 flat loads in flight keep 64 full addresses in registers.
using GlobalColumn = const __attribute__((address_space(1))) double *;

// The workgroup's scratch: the caller declares ONE (a kernel that instantiates compare_column several times would
// otherwise carry one copy per instantiation).
struct CompareScratch {
  double part4[4][256];
  int diff;
};

// Sample s of column 1 is x1[s * k1], of column 2 x2[s * k2]: k = the event's isoforms for a column in the samples pool
// (rows of K values), 1 for a column staged contiguously in LDS.
// CACHED (S <= 256 * SUMMARY_CACHE): the paired differences stay in registers, so the two sample
// columns are read once instead of three times.
// Called again by the same workgroup (the group pass): a __syncthreads() between the calls, `diff` is read up to the end.
// P1, P2: `const double *`, or a pointer the caller has cast to its address space (GlobalColumn).
template <bool CACHED, class P1, class P2>
__device__ __forceinline__ void compare_column(P1 x1, int k1, P2 x2, int k2, int S,
                                               double smoothing, double *o, CompareScratch &sc) {
  double (*part4)[256] = sc.part4;
  const int t = threadIdx.x;
  double *part = part4[0];
  const double n = static_cast<double>(S);

  if (t == 0) sc.diff = 0;
  const double d0 = x1[0] - x2[0];
  double acc[4] = {0, 0, 0, 0};   // sum psi1, sum psi2, sum d, sum |d|
  double dv[CACHED ? SUMMARY_CACHE : 1];
  int differs = 0;
  if (CACHED) {
#pragma unroll
    for (int j = 0; j < SUMMARY_CACHE; j++) {
      const int s = t + 256 * j;
      dv[j] = 0.0;
      if (s < S) {
        const double u = x1[static_cast<size_t>(s) * k1], v = x2[static_cast<size_t>(s) * k2];
        const double d = u - v;
        acc[0] = acc[0] + u; acc[1] = acc[1] + v; acc[2] = acc[2] + d; acc[3] = acc[3] + fabs(d);
        differs |= (d - d0 != 0.0);
        dv[j] = d;
      }
    }
  } else {
    for (int s = t; s < S; s += 256) {
      const double u = x1[static_cast<size_t>(s) * k1], v = x2[static_cast<size_t>(s) * k2];
      const double d = u - v;
      acc[0] = acc[0] + u; acc[1] = acc[1] + v; acc[2] = acc[2] + d; acc[3] = acc[3] + fabs(d);
      differs |= (d - d0 != 0.0);
    }
  }
  block_tree_sum4(acc, part4);
  const double sum1 = acc[0], sum2 = acc[1], sumd = acc[2], sumabs = acc[3];
  if (differs) atomicOr(&sc.diff, 1);
  __syncthreads();
  const bool all_same = sc.diff == 0;
  const double mean_d = sumd / n, mad = sumabs / n;

  double bf, post = 0.0;
  if (mad <= 0.009 || all_same) {       // block-uniform: every thread sees the same sums
    bf = 0.0;
    post = __longlong_as_double(0x7FF0000000000000ull);
  } else {
    double av = 0;
    if (CACHED) {
#pragma unroll
      for (int j = 0; j < SUMMARY_CACHE; j++)
        if (t + 256 * j < S) { const double d = dv[j] - mean_d; av = av + d * d; }
    } else {
      for (int s = t; s < S; s += 256) {
        const double d = (x1[static_cast<size_t>(s) * k1] - x2[static_cast<size_t>(s) * k2]) - mean_d;
        av = av + d * d;
      }
    }
    const double var = block_tree_sum(av, part) / (n - 1.0);
    const double cov = var * (smoothing * smoothing);
    const double inv2 = 1.0 / (2.0 * cov);
    double ae = 0;
    if (CACHED) {
#pragma unroll
      for (int j = 0; j < SUMMARY_CACHE; j++)
        if (t + 256 * j < S) ae = ae + miso_det_exp(-(dv[j] * dv[j]) * inv2);
    } else {
      for (int s = t; s < S; s += 256) {
        const double d = x1[static_cast<size_t>(s) * k1] - x2[static_cast<size_t>(s) * k2];
        ae = ae + miso_det_exp(-(d * d) * inv2);
      }
    }
    const double se = block_tree_sum(ae, part);
    post = se / (n * miso_det_sqrt(6.283185307179586 * cov));
    if (post == 0.0) bf = 1e12;
    else { bf = 1.0 / post; if (bf > 1e12) bf = 1e12; }
  }
  if (t == 0) { o[0] = sum1 / n; o[1] = sum2 / n; o[2] = bf; o[3] = post; }
}

}  // namespace miso
