// kernels_diagnose_rank.hip -- rank-normalised chain diagnostics on the device: per (event, isoform) column
// of the resident samples the bulk and the folded split R-hat, the bulk effective sample size, and the effective sample
// size of the indicators of the two credible-interval bounds (Vehtari, Gelman, Simpson, Carpenter & Buerkner 2021, with
// the tails at the interval's own order statistics).  No reference counterpart.
//
// The sequences (C, n, h, M = 2 C, N = M h, e = j h + i) and the moments-and-Geyer stage are diagnose_column.hpp's.  With
// srt[0..N) the used draws in ascending order, lo and hi the interval's order statistics over N (the host's):
//
//   rank normalisation of values v[0..N):  less = #{v < v_e}, equal = #{v == v_e} (as doubles compare: -0.0 == +0.0),
//       r2 = 2 less + equal + 1 (twice the average rank, an integer),  p = (0.5 r2 - 0.375) / (N + 0.25),
//       z_e = miso_det_qnorm(p)
//   bulk       z of the used draws
//   folded     med = 0.5 srt[N/2 - 1] + 0.5 srt[N/2];  z of |x_e - med|
//   low tail   x_e <= srt[lo] ? 1.0 : 0.0
//   high tail  x_e >= srt[hi] ? 1.0 : 0.0
//
// each column then through diag_moments.  Out, six doubles: rhat of bulk, rhat of folded, ess of bulk, ess of low tail,
// ess of high tail, the number of distinct used draws.  A NaN or an infinity among the used draws: five NaN and 0.
//
// One 256-thread workgroup per column; dynamic LDS, in 8-byte words:  A[N] the used draws at e, as loaded from HBM once;
// B[P] (P the power of two >= N) the sort's keys, then the transformed column in its first N words;  then the larger of
// diag_moments' 3 M doubles and N 16-bit words R, which hold r2 between the searches and the normal scores: the
// searches read all of B, the scores overwrite it, and r2 <= 2 N = 16384 fits.  At most (8192 + 8192 + 3 * 1024) * 8 bytes =
// 152 KB.  Pass 0 sorts the draws (bitonic network over P keys, padded with the largest key, which no finite value has;
// P / 2 compare-exchanges per stage, a barrier after each), takes srt[lo], srt[hi], med and the distinct count from the
// sorted keys and ranks every draw by a lower-bound and an upper-bound binary search; pass 1 the same on |x - med|; passes
// 2 and 3 write the indicators from A.  Every barrier sits in workgroup-uniform control flow.
#include <hip/hip_runtime.h>

#include "device.hpp"
#include "diagnose_column.hpp"
#include "miso_detmath.h"
#include "order_key.hpp"

namespace miso {

// ascending, exact; B[P] published by a barrier, P a power of two >= 2
__device__ __forceinline__ void rank_sort(uint64_t *B, int P) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int idx = threadIdx.x; idx < (P >> 1); idx += 256) {
        const int i = 2 * idx - (idx & (j - 1)), l = i + j;   // the pair (i, i + j), bit j of i clear
        const uint64_t a = B[i], b = B[l];
        const bool up = (i & k) == 0;
        if ((a > b) == up) { B[i] = b; B[l] = a; }
      }
      __syncthreads();
    }
  }
}

// r2 = 2 less + equal + 1 of key among the sorted keys B[0..N)
__device__ __forceinline__ int rank_r2(const uint64_t *B, int N, uint64_t key) {
  int lb = 0, end = N;
  while (lb < end) {
    const int mid = (lb + end) >> 1;
    if (B[mid] < key) lb = mid + 1; else end = mid;
  }
  int ub = lb;
  end = N;
  while (ub < end) {
    const int mid = (ub + end) >> 1;
    if (B[mid] <= key) ub = mid + 1; else end = mid;
  }
  return lb + ub + 1;
}

// Grid (events, kmax), one workgroup per column; out: six doubles per (event, isoform) at rank_off[ev] + 6 k.  The host
// refuses N > 8192 and C > 512 and sizes the dynamic LDS: (N + P + max(3 M, (N + 3) / 4)) * 8 bytes.
__global__ __launch_bounds__(256) void diagnose_rank_kernel(const DevEvent *events, const unsigned char *out_pool,
                                                            int n_events, int C, int n, int h, int P, int lo, int hi,
                                                            double log10N, const uint64_t *rank_off, double *out) {
  extern __shared__ double rank_lds[];
  __shared__ double s_o[4];
  __shared__ int s_cnt[4];
  const int ev = blockIdx.x, kk = blockIdx.y;
  if (ev >= n_events) return;
  const DevEvent E = events[ev];
  if (kk >= E.K) return;
  const double *x = reinterpret_cast<const double *>(out_pool + E.off_samples) + kk;
  double *o = out + rank_off[ev] + 6 * kk;
  const DiagShape sh{C, n, h, E.K};
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int M = 2 * C, N = M * h;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);

  double *A = rank_lds;
  double *Z = A + N;
  uint64_t *B = reinterpret_cast<uint64_t *>(Z);
  double *m = Z + P;
  unsigned short *R = reinterpret_cast<unsigned short *>(m);

  const bool finite = diag_load(x, sh, A);
  if (__syncthreads_or(finite ? 0 : 1)) {             // workgroup-uniform
    if (t == 0) { o[0] = nan; o[1] = nan; o[2] = nan; o[3] = nan; o[4] = nan; o[5] = 0.0; }
    return;
  }

  double thr_lo = 0.0, thr_hi = 0.0, med = 0.0;
  for (int pass = 0; pass < 4; pass++) {
    if (pass < 2) {
      // (x + 0.0: -0.0 becomes +0.0, so equal doubles have equal keys)
      for (int e = t; e < P; e += 256)
        B[e] = (e < N) ? order_key(pass ? fabs(A[e] - med) : A[e] + 0.0) : ~0ull;
      __syncthreads();
      rank_sort(B, P);
      if (pass == 0) {
        thr_lo = key_value(B[lo]);
        thr_hi = key_value(B[hi]);
        med = 0.5 * key_value(B[N / 2 - 1]) + 0.5 * key_value(B[N / 2]);
        int c = 0;
        for (int e = t; e < N; e += 256) c += (e == 0 || B[e] != B[e - 1]) ? 1 : 0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) c += __shfl_down(c, off);
        if (lane == 0) s_cnt[wave] = c;               // read by thread 0 behind the barriers below
      }
      for (int e = t; e < N; e += 256)
        R[e] = static_cast<unsigned short>(rank_r2(B, N, order_key(pass ? fabs(A[e] - med) : A[e] + 0.0)));
      __syncthreads();                                // the searches are done with B: the scores go over it
      for (int e = t; e < N; e += 256) {
        const double p = (0.5 * static_cast<double>(R[e]) - 0.375) / (static_cast<double>(N) + 0.25);
        Z[e] = miso_det_qnorm(p);
      }
    } else {
      for (int e = t; e < N; e += 256) Z[e] = ((pass == 2) ? (A[e] <= thr_lo) : (A[e] >= thr_hi)) ? 1.0 : 0.0;
    }
    __syncthreads();                                  // Z is whole; R is read: m may take its place
    diag_moments<true>(nullptr, sh, log10N, s_o, Z, m);
    if (t == 0) {
      if (pass == 0) { o[0] = s_o[0]; o[2] = s_o[1]; o[5] = static_cast<double>(s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]); }
      else if (pass == 1) o[1] = s_o[0];
      else o[pass + 1] = s_o[1];
    }
    __syncthreads();                                  // Z, m and s_o are free for the next pass
  }
}

}  // namespace miso
