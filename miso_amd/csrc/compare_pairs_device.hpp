// compare_pairs_device.hpp -- the device routines compare_pairs_kernel (kernels_compare_pairs.hip) and
// compare_pairs_groups_kernel (kernels_compare_pairs_groups.hip) share: the sort of a column of order_keys in LDS and the
// count of the differences at or below three thresholds.  One text, so that a group of one sample against a group of one
// gives the pairwise pass's bits.  Workgroups of 256 threads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

}  // namespace miso
