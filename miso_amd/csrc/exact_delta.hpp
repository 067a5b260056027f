// exact_delta.hpp -- "the quantiles of delta psi from the exact CDF" (DESIGN.md 20): what kernels_exact_delta.hip (single-end)
// and kernels_exact_paired_delta.hip (paired-end) do alike once A's and B's tables stand.  H(z) = P(psi_1 - psi_2 <= z) is
// exact_compare.hpp's quadrature, here with the value in every lane; H(z) = p is solved by EXACT_DELTA_ROUNDS rounds of
// eight points inside the bracket and one linear interpolation.  Device part: a sweep over A's points for NZ values of z at
// once, the bracket's update, the interpolation.  Host part: the check of the probabilities.  -ffp-contract=off; every
// operation in a fixed order: tests/_exact_delta_ref.py restates these functions.
#pragma once
#include <hip/hip_runtime.h>

#include "host.hpp"
#include "miso_detmath.h"

#include "exact_compare.hpp"

namespace miso {

constexpr int EXACT_DELTA_MAX_P = 4;    // probabilities per call
constexpr int EXACT_DELTA_PTS = 8;      // points per round, inside the bracket
constexpr int EXACT_DELTA_ROUNDS = 5;   // the first one, on (-1, 1), is the same for every probability

// lo < q <= hi with Hlo = H(lo) < p <= Hhi = H(hi); the ends of (-1, 1, 0, 1) are by definition, not evaluated
struct ExactBracket { double lo, Hlo, hi, Hhi; };

// the round's points: lo + j (hi - lo) / 9, j = 1 .. 8
__device__ __forceinline__ void exact_delta_points(const ExactBracket &b, double (&z)[EXACT_DELTA_PTS]) {
  const double step = (b.hi - b.lo) / static_cast<double>(EXACT_DELTA_PTS + 1);
#pragma unroll
  for (int j = 1; j <= EXACT_DELTA_PTS; j++) z[j - 1] = b.lo + static_cast<double>(j) * step;
}

// The round's end: j* is the smallest j with H_j >= p (9: none); the point before it is the new low end, the point itself
// the new high end, and an end without such a point keeps its value.  (Selects, no indexed register array.)
__device__ __forceinline__ ExactBracket exact_delta_update(ExactBracket b, const double (&z)[EXACT_DELTA_PTS],
                                                           const double (&H)[EXACT_DELTA_PTS], double p) {
  bool found = false;
#pragma unroll
  for (int j = 0; j < EXACT_DELTA_PTS; j++) {
    const bool ge = H[j] >= p;
    const bool up = !found && ge, dn = !found && !ge;
    b.hi = up ? z[j] : b.hi; b.Hhi = up ? H[j] : b.Hhi;
    b.lo = dn ? z[j] : b.lo; b.Hlo = dn ? H[j] : b.Hlo;
    found = found || ge;
  }
  return b;
}

// the quantile from the last bracket (Hlo < p <= Hhi: the divisor is positive)
__device__ __forceinline__ double exact_delta_interpolate(const ExactBracket &b, double p) {
  return b.lo + (b.hi - b.lo) * ((p - b.Hlo) / (b.Hhi - b.Hlo));
}

// H at NZ points from one sweep over A's 2049 points, in every lane: exact_compare's quadrature body, the accumulators
// unrolled over z.  weight(j, pt, p): f_A at point pt = 32 lane + j, p = exact_point there -- made again from scalars
// (single-end) or read from the workgroup's row (paired-end).  red: 256 doubles of LDS.  Every z lies inside (-1, 1).
template <int NZ, class Weight>
__device__ __forceinline__ void exact_delta_sweep(const ExactStats &stA, const ExactTable &TA, const ExactTable &TB, bool a2,
                                                  const double (&z)[NZ], double (&H)[NZ], double *red, int lane, Weight weight) {
  double acc[NZ];
#pragma unroll
  for (int k = 0; k < NZ; k++) acc[k] = 0.0;
  const int i0 = EXACT_CELLS * lane;
  const int n_own = EXACT_CELLS + (lane == 63 ? 1 : 0);   // the last lane owns the grid's last point too
#pragma unroll 1
  for (int j = 0; j < n_own; j++) {
    const int pt = i0 + j;
    const ExactPoint p = exact_point(stA, TA.tL + TA.h * static_cast<double>(pt));
    const double wf = ((pt == 0 || pt == EXACT_G) ? 0.5 : 1.0) * weight(j, pt, p);
#pragma unroll
    for (int k = 0; k < NZ; k++) {
      const double zk = z[k];
      const double val = a2 ? exact_cdf_at(TB, p.x + zk, p.y - zk) : exact_cdf_at(TB, p.x - zk, p.y + zk);
      acc[k] = acc[k] + wf * (val / TB.Z);
    }
  }
  // exact_lanes_sum's sums -- from 0.0, the lanes in order --, four values of z side by side in red's four columns
#pragma unroll
  for (int k0 = 0; k0 < NZ; k0 += 4) {
    constexpr int NB = NZ < 4 ? NZ : 4;
#pragma unroll
    for (int k = 0; k < NB; k++) red[64 * k + lane] = acc[k0 + k];
    __syncthreads();
    double s[NB];
#pragma unroll
    for (int k = 0; k < NB; k++) s[k] = 0.0;
#pragma unroll 4
    for (int m = 0; m < 64; m++) {
#pragma unroll
      for (int k = 0; k < NB; k++) s[k] = s[k] + red[64 * k + m];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NB; k++) {
      const double v = s[k] / TA.sf;
      H[k0 + k] = a2 ? v : 1.0 - v;
    }
  }
}

// The whole search of one pair, tables standing: o[0 .. n_p) the quantiles at prob[0 .. n_p), o[n_p] = H(0.0).  sweep1(z, H)
// and sweep8(z, H) are the unit's sweeps at one and at eight points.  Wavefront-uniform: every lane holds every value.
template <class Sweep1, class Sweep8>
__device__ __forceinline__ void exact_delta_search(const double *prob, int n_p, double *o, int lane, Sweep1 sweep1, Sweep8 sweep8) {
  {
    const double z0[1] = {0.0};
    double H0[1];
    sweep1(z0, H0);
    if (lane == 0) o[n_p] = H0[0];
  }
  const ExactBracket all{-1.0, 0.0, 1.0, 1.0};
  double z1[EXACT_DELTA_PTS], H1[EXACT_DELTA_PTS];
  exact_delta_points(all, z1);
  sweep8(z1, H1);
#pragma unroll 1
  for (int k = 0; k < n_p; k++) {
    const double pk = prob[k];
    ExactBracket b = exact_delta_update(all, z1, H1, pk);
#pragma unroll 1
    for (int r = 1; r < EXACT_DELTA_ROUNDS; r++) {
      double z[EXACT_DELTA_PTS], H[EXACT_DELTA_PTS];
      exact_delta_points(b, z);
      sweep8(z, H);
      b = exact_delta_update(b, z, H, pk);
    }
    if (lane == 0) o[k] = exact_delta_interpolate(b, pk);
  }
}

// the probabilities of a call
inline void exact_delta_check_p(const double *p, int n_p) {
  if (n_p < 1 || n_p > EXACT_DELTA_MAX_P) MISO_FAIL(MISO_EINVAL, "The number of probabilities must lie in [1, 4]");
  for (int k = 0; k < n_p; k++) if (!(p[k] > 0.0 && p[k] < 1.0)) MISO_FAIL(MISO_EINVAL, "A probability must lie inside (0, 1)");
}

}  // namespace miso
