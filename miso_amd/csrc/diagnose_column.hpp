// diagnose_column.hpp -- the split-sequence layout and the moments-and-Geyer stage of the chain diagnostics, shared by
// kernels_diagnose.hip (the raw column) and kernels_diagnose_rank.hip (the rank-normalised columns); DESIGN.md 14, 14a.
//
// Input: a column x[0..S) (column s from chain s % C), C chains.  n = S / C draws per chain (the trailing S - n C
// columns are ignored), h = n / 2, M = 2 C sequences of h draws, N = M h.  Sequence j = 2 c + half is chain c's first
// (half = 0: draws 0 .. h-1) or last (half = 1: draws n-h .. n-1) h draws; the middle draw of an odd n is in neither.
// Element (j, i) is sample ((half ? n - h : 0) + i) C + c and has the flat index e = j h + i.
//
// One 256-thread workgroup (four wavefronts) per column.  THE ORDER OF EVERY OPERATION, which tests/_diag_ref.py
// restates bit for bit (all arithmetic IEEE double, no contraction, `/` the IEEE division):
//
//   wave sum of a sequence's terms u_0 .. u_{h'-1}:  lane l adds u_l, u_{l+64}, u_{l+128}, ... in that order onto +0.0;
//       then the 64 partial sums p_l go through the tree  p_l = p_l + p_{l+off}  (l < off)  for off = 32, 16, 8, 4, 2, 1;
//       the sum is p_0.
//   per sequence j (wavefront j % 4 takes it):
//       m_j   = wavesum(x_{j,i}) / h
//       d_j,i = x_{j,i} - m_j
//       s2_j  = wavesum(d_j,i * d_j,i) / (h - 1)
//   thread 0, every sum over ascending j onto +0.0:
//       W  = (sum_j s2_j) / M          mm = (sum_j m_j) / M
//       Bh = (sum_j (m_j - mm) * (m_j - mm)) / (M - 1)
//       V  = (W * (h - 1)) / h + Bh
//       degenerate = !(W > 0) || V is not finite  ->  rhat = ess = mcse = NaN, lag = 0, done
//   lags, one pair k = 0, 1, ... per trip (t = 2k, 2k+1; rho_0 = 1 is not computed):  unit u = 2 j + (t & 1) goes to
//   wavefront u % 4:
//       a_j(t) = wavesum(d_j,i * d_j,i+t, i = 0 .. h-1-t) / h
//   thread 0:
//       A_t   = (sum_j a_j(t)) / M     rho_t = 1 - (W - A_t) / V
//       P_k   = rho_2k + rho_2k+1
//       k = 0: taken.  k >= 1: taken if P_k > 0 (a NaN is not), then P_k = min(P_k, P_k-1 as adjusted) = (P_k < prev ? P_k
//       : prev).  sumP = sumP + P_k in the order taken.  The loop goes on to pair k + 1 only if pair k was taken and
//       2 (k + 1) + 1 <= h - 1: the decision is thread 0's, handed to the workgroup through LDS behind a barrier.
//   thread 0:
//       tau  = -1 + 2 sumP;  floor = 1 / log10(N) (log10(N) comes from the host);  tau = tau > floor ? tau : floor
//       ess  = N / tau       mcse = miso_det_sqrt(V / ess)      rhat = miso_det_sqrt(V / W)      lag = 2 * pairs taken
//
// CACHED: the column is read from HBM once, in sample order (a wavefront's loads walk the column's rows), and scattered
// to LDS at e = j h + i: a sequence is contiguous, so a wavefront's two ds_read_b64 of a lag product (d_e and d_{e+t},
// lane l at e = j h + l + 64 q) each walk 64 consecutive doubles -- 512 consecutive bytes, each 32-lane half one full
// 256-byte bank row, whatever the parity of t (a double's address is a multiple of 8: an odd lag shifts the row by 8
// bytes, not onto shared banks).  The centred values replace the raw ones in place.  Uncached: the same sums read x from
// global memory (the column is L2-resident for its one workgroup) and subtract m_j on the fly -- the same subtraction,
// the same bits.
//
// Cost: the moments O(N); each lag pair 2 N multiply-adds in 2M units over four wavefronts and two barriers.  A mixed
// column stops after a handful of pairs; a trending one runs all (h - 1) / 2 of them: O(M h^2) multiply-adds.
#pragma once
#include <hip/hip_runtime.h>

#include "miso_detmath.h"

namespace miso {

__device__ __forceinline__ double diag_wave_tree(double p) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) p = p + __shfl_down(p, off);
  return __shfl(p, 0);
}

// What one column needs to know about its split sequences.
struct DiagShape {
  int C, n, h, K;
  // sample index of element (j, i)
  __device__ __forceinline__ size_t sample(int j, int i) const {
    const int c = j >> 1;
    const int draw = (j & 1) ? n - h + i : i;
    return static_cast<size_t>(draw) * C + c;
  }
};

// One pass over the column in sample order into D[N] at e = j h + i; the middle draw of an odd n and the trailing columns
// are not kept.  Returns whether every value this thread stored is finite.  The caller's barrier publishes D.
__device__ __forceinline__ bool diag_load(const double *x, const DiagShape sh, double *D) {
  const int h = sh.h, used = sh.n * sh.C;
  bool finite = true;
  for (int s = threadIdx.x; s < used; s += 256) {
    const int draw = s / sh.C, c = s - draw * sh.C;
    int j = -1, i = 0;
    if (draw < h) { j = 2 * c; i = draw; }
    else if (draw >= sh.n - h) { j = 2 * c + 1; i = draw - (sh.n - h); }
    if (j >= 0) {
      const double v = x[static_cast<size_t>(s) * sh.K];
      D[j * h + i] = v;
      finite = finite && (v - v) == 0.0;               // false for NaN and +-inf
    }
  }
  return finite;
}

// The moments-and-Geyer stage: o[0..4) = {rhat, ess, mcse, lag}, written by thread 0.  CACHED: the column is D[N] in LDS
// (published by a barrier) and is centred in place; else it is read from x.  m: 3 M doubles of LDS (m[M], a0[M], a1[M]).
// Every thread of the workgroup calls it; its barriers sit in workgroup-uniform control flow.  A second call may follow
// at once: the first barrier of a call orders the reuse of the shared words after the last reads of the call before.
template <bool CACHED>
__device__ __forceinline__ void diag_moments(const double *x, const DiagShape sh, double log10N, double *o, double *D,
                                             double *m) {
  __shared__ double s_W, s_V;
  __shared__ int s_go;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h = sh.h, M = 2 * sh.C, N = M * h;
  double *a0 = m + M, *a1 = a0 + M;

  // per-sequence mean and variance; the cached values are centred in place (a sequence belongs to one wavefront)
  for (int j = wave; j < M; j += 4) {
    double acc = 0.0;
    for (int i = lane; i < h; i += 64) acc = acc + (CACHED ? D[j * h + i] : x[sh.sample(j, i) * sh.K]);
    const double mj = diag_wave_tree(acc) / static_cast<double>(h);
    double q = 0.0;
    for (int i = lane; i < h; i += 64) {
      const double d = (CACHED ? D[j * h + i] : x[sh.sample(j, i) * sh.K]) - mj;
      if (CACHED) D[j * h + i] = d;
      q = q + d * d;
    }
    const double s2 = diag_wave_tree(q) / static_cast<double>(h - 1);
    if (lane == 0) { m[j] = mj; a0[j] = s2; }
  }
  __syncthreads();

  if (t == 0) {
    double sw = 0.0, sm = 0.0;
    for (int j = 0; j < M; j++) { sw = sw + a0[j]; sm = sm + m[j]; }
    const double W = sw / static_cast<double>(M), mm = sm / static_cast<double>(M);
    double sb = 0.0;
    for (int j = 0; j < M; j++) { const double dm = m[j] - mm; sb = sb + dm * dm; }
    const double Bh = sb / static_cast<double>(M - 1);
    const double V = (W * static_cast<double>(h - 1)) / static_cast<double>(h) + Bh;
    const bool finite = (V - V) == 0.0;              // false for NaN and +-inf
    s_W = W; s_V = V;
    s_go = (W > 0.0 && finite) ? 1 : 0;
    if (!s_go) {
      const double nan = __longlong_as_double(0x7FF8000000000000ll);
      o[0] = nan; o[1] = nan; o[2] = nan; o[3] = 0.0;
    }
  }
  __syncthreads();
  if (!s_go) return;                                  // workgroup-uniform
  const double W = s_W, V = s_V;

  double sumP = 0.0, prev = 0.0;                      // thread 0's
  int pairs = 0;
  for (int k = 0;; k++) {
    // units u = 2 j + which: a_j(2k + which); rho_0 is 1 by definition, so pair 0 has the odd units only
    for (int u = wave; u < 2 * M; u += 4) {
      const int j = u >> 1, which = u & 1;
      if (k == 0 && which == 0) continue;             // (wavefront-uniform: u is)
      const int lag = 2 * k + which;
      const double mj = CACHED ? 0.0 : m[j];
      double acc = 0.0;
      for (int i = lane; i + lag < h; i += 64) {
        const double d0 = CACHED ? D[j * h + i] : x[sh.sample(j, i) * sh.K] - mj;
        const double d1 = CACHED ? D[j * h + i + lag] : x[sh.sample(j, i + lag) * sh.K] - mj;
        acc = acc + d0 * d1;
      }
      const double a = diag_wave_tree(acc) / static_cast<double>(h);
      if (lane == 0) (which ? a1 : a0)[j] = a;
    }
    __syncthreads();
    if (t == 0) {
      double rho[2];
      rho[0] = 1.0;
      for (int which = (k == 0 ? 1 : 0); which < 2; which++) {
        const double *a = which ? a1 : a0;
        double sa = 0.0;
        for (int j = 0; j < M; j++) sa = sa + a[j];
        const double A = sa / static_cast<double>(M);
        rho[which] = 1.0 - (W - A) / V;
      }
      double P = rho[0] + rho[1];
      bool taken = true;
      if (k >= 1) {
        taken = P > 0.0;
        if (taken) P = (P < prev) ? P : prev;
      }
      if (taken) { sumP = sumP + P; prev = P; pairs++; }
      s_go = (taken && 2 * (k + 1) + 1 <= h - 1) ? 1 : 0;
    }
    __syncthreads();
    if (!s_go) break;                                 // workgroup-uniform; the next trip's first barrier orders the reuse of s_go
  }

  if (t == 0) {
    double tau = -1.0 + 2.0 * sumP;
    const double floor_tau = 1.0 / log10N;
    tau = (tau > floor_tau) ? tau : floor_tau;
    const double ess = static_cast<double>(N) / tau;
    o[0] = miso_det_sqrt(V / W);
    o[1] = ess;
    o[2] = miso_det_sqrt(V / ess);
    o[3] = static_cast<double>(2 * pairs);
  }
}

}  // namespace miso
