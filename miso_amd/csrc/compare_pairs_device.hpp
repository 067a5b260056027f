// compare_pairs_device.hpp -- the device routines compare_pairs_kernel (kernels_compare_pairs.hip),
// compare_pairs_groups_kernel (kernels_compare_pairs_groups.hip) and the isoform-group kernels (kernels_groups.hip) share:
// the sort of a column of order_keys in LDS, the count of the differences at or below three thresholds and, once both
// columns stand sorted, the statistics themselves.  One text, so that a group of one sample against a group of one, and a
// group of one isoform, give the pairwise pass's bits.  Workgroups of 256 threads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compare_pairs.hpp"
#include "order_key.hpp"

namespace miso {

// ascending, exact; B[0..N) published by a barrier, any N >= 1
__device__ __forceinline__ void pairs_sort(uint64_t *B, int N) {
  int P = 2;
  while (P < N) P <<= 1;
  for (int k = 2; k <= P; k <<= 1) {
    const int hk = k >> 1;
    for (int idx = threadIdx.x; idx < (P >> 1); idx += 256) {
      const int r = idx & (hk - 1), base = (idx - r) << 1;   // the block of k keys, r its pair: (base + r, base + k - 1 - r)
      const int i = base + r, l = base + k - 1 - r;
      if (l < N) {
        const uint64_t a = B[i], b = B[l];
        if (a > b) { B[i] = b; B[l] = a; }
      }
    }
    __syncthreads();
    for (int j = hk >> 1; j > 0; j >>= 1) {
      for (int idx = threadIdx.x; idx < (P >> 1); idx += 256) {
        const int i = 2 * idx - (idx & (j - 1)), l = i + j;   // the pair (i, i + j), bit j of i clear
        if (l < N) {
          const uint64_t a = B[i], b = B[l];
          if (a > b) { B[i] = b; B[l] = a; }
        }
      }
      __syncthreads();
    }
  }
}

// d <= t, or d < t
__device__ __forceinline__ bool pairs_below(double d, double t, bool strict) { return strict ? (d < t) : (d <= t); }

// draws of a that a thread searches for at once: with the three thresholds twelve independent chains of LDS reads, which is
// what hides their latency at the two wavefronts per SIMD the LDS leaves (the measurements)
constexpr int PAIRS_E = 4;

// cnt[q] = #{(i, j): fl(A[i] - B[j]) <= th[q]} (strict[q]: < th[q]) for three thresholds at once, the same numbers in every
// thread.  A, B ascending doubles; B in LDS, A in LDS or in global memory (written by this workgroup before a barrier).
// Thread t takes a[t], a[t + 256], ...: for each the start p of its suffix of b by a
// binary search that applies the predicate to the difference itself (a wavefront's 64 draws are neighbours in a, so their
// searches read the same few words of b).  part: four partial sums per query, which the caller alternates between two
// buffers from call to call (one barrier per call: a buffer is written again two calls later, behind the barrier of the call
// in between).
__device__ __forceinline__ void pairs_count(const double *A, int S1, const double *B, int S2, const double (&th)[3],
                                            const bool (&strict)[3], uint32_t (&cnt)[3], uint32_t (*part)[3]) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  cnt[0] = cnt[1] = cnt[2] = 0;
  for (int i = t; i < S1; i += 256 * PAIRS_E) {
    double a[PAIRS_E];
    int p[PAIRS_E][3];
#pragma unroll
    for (int e = 0; e < PAIRS_E; e++) {
      a[e] = A[min(i + 256 * e, S1 - 1)];               // (past the end: searched like the last draw, not counted)
      p[e][0] = p[e][1] = p[e][2] = 0;
    }
    int len = S2;
    while (len > 1) {                                 // the starts lie in [p, p + len]
      const int half = len >> 1;
#pragma unroll
      for (int e = 0; e < PAIRS_E; e++)
#pragma unroll
        for (int q = 0; q < 3; q++)
          if (!pairs_below(a[e] - B[p[e][q] + half - 1], th[q], strict[q])) p[e][q] += half;
      len -= half;
    }
#pragma unroll
    for (int e = 0; e < PAIRS_E; e++)
#pragma unroll
      for (int q = 0; q < 3; q++) {
        if (!pairs_below(a[e] - B[p[e][q]], th[q], strict[q])) p[e][q]++;
        if (i + 256 * e < S1) cnt[q] += static_cast<uint32_t>(S2 - p[e][q]);
      }
  }
#pragma unroll
  for (int q = 0; q < 3; q++) {
    uint32_t v = cnt[q];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
    if (lane == 0) part[wave][q] = v;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 3; q++) cnt[q] = part[0][q] + part[1][q] + part[2][q] + part[3][q];
}

// What an all-pairs kernel's workgroup holds beside its columns
struct PairsScratch {
  uint32_t part[2][4][3];
  uint32_t cnt[2 + 2 * PAIRS_MAX_TAU];   // thread 0's: the threshold counts until it puts them together
};

// A column pair's statistics (compare_pairs.hpp: pairs_words(pa.n_tau) words at o) once A[0..S1) and B[0..S2) stand
// ascending and published, A in LDS or global memory, B in LDS: the three order statistics by bisections over the keys of
// [smallest difference, largest difference] that share their passes, then the threshold counts, three to a pass.  Every
// barrier in workgroup-uniform control flow (the bisections' bounds are the same numbers in every thread).
__device__ __forceinline__ void pairs_statistics(const double *A, int S1, const double *B, int S2, const PairsArgs &pa, uint64_t *o,
                                                 PairsScratch &sc) {
  const int t = threadIdx.x;
  const uint32_t M = static_cast<uint32_t>(S1) * static_cast<uint32_t>(S2);   // <= 2^28
  int buf = 0;

  uint64_t lo_k[3], hi_k[3];
  {
    const uint64_t kmin = order_key(A[0] - B[S2 - 1]), kmax = order_key(A[S1 - 1] - B[0]);
#pragma unroll
    for (int q = 0; q < 3; q++) { lo_k[q] = kmin; hi_k[q] = kmax; }
  }
  const bool not_strict[3] = {false, false, false};
  while (lo_k[0] < hi_k[0] || lo_k[1] < hi_k[1] || lo_k[2] < hi_k[2]) {
    uint64_t mid[3];
    double th[3];
    uint32_t cnt[3];
#pragma unroll
    for (int q = 0; q < 3; q++) { mid[q] = lo_k[q] + ((hi_k[q] - lo_k[q]) >> 1); th[q] = key_value(mid[q]); }
    pairs_count(A, S1, B, S2, th, not_strict, cnt, sc.part[buf]);
    buf ^= 1;
#pragma unroll
    for (int q = 0; q < 3; q++)
      if (lo_k[q] < hi_k[q]) {
        if (cnt[q] >= pa.rank[q] + 1u) hi_k[q] = mid[q]; else lo_k[q] = mid[q] + 1;
      }
  }

  // the counts: query 0 is #{d <= 0}, 1 #{d < 0}, 2 + 2 j #{d < tau_j}, 3 + 2 j #{d <= -tau_j}; three to a pass
  const int n_query = 2 + 2 * pa.n_tau;
  for (int q0 = 0; q0 < n_query; q0 += 3) {
    double th[3];
    bool strict[3];
    uint32_t cnt[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const int qi = q0 + q;
      th[q] = 0.0; strict[q] = false;
      if (qi == 1) strict[q] = true;
      else if (qi >= 2 && qi < n_query) {
        const double tau = pa.tau[(qi - 2) >> 1];
        if (qi & 1) th[q] = -tau; else { th[q] = tau; strict[q] = true; }
      }
    }
    pairs_count(A, S1, B, S2, th, strict, cnt, sc.part[buf]);
    buf ^= 1;
    if (t == 0) {
#pragma unroll
      for (int q = 0; q < 3; q++)
        if (q0 + q < n_query) sc.cnt[q0 + q] = cnt[q];
    }
  }
  if (t == 0) {
    // (+ 0.0: the smallest key whose count suffices is -0.0's when the order statistic is zero)
#pragma unroll
    for (int q = 0; q < 3; q++) o[q] = static_cast<uint64_t>(__double_as_longlong(key_value(lo_k[q]) + 0.0));
    o[3] = M - sc.cnt[0];
    o[4] = sc.cnt[1];
    o[5] = 1;
    for (int j = 0; j < pa.n_tau; j++) o[PAIRS_FIXED_WORDS + j] = static_cast<uint64_t>(M - sc.cnt[2 + 2 * j]) + sc.cnt[3 + 2 * j];
  }
}

// ... and of a pair that is not finite, or whose event was never decoded: three NaN, no counts, finite = 0
__device__ __forceinline__ void pairs_not_finite(uint64_t *o, int n_tau) {
  const uint64_t nan = 0x7FF8000000000000ull;
  o[0] = nan; o[1] = nan; o[2] = nan;
  for (int w = 3; w < PAIRS_FIXED_WORDS + n_tau; w++) o[w] = 0;
}

}  // namespace miso
