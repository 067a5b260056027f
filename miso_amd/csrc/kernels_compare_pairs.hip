// kernels_compare_pairs.hip -- the posterior of delta psi = psi_1 - psi_2 over ALL pairs of two samples' draws:
// per (event, isoform) column pair a[0..S1) of sample 1 and b[0..S2) of sample 2, with D the multiset of the M = S1 S2 IEEE
// doubles fl(a_i - b_j): three order statistics of D (lower median, the two bounds of a credible interval; the ranks are
// the host's) and the exact counts #{d > 0}, #{d < 0} and, per threshold tau, #{d >= tau} + #{d <= -tau}.  No reference
// counterpart (the reference pairs the draws by row index, hypothesis_test.py:89-179).
//
// D is never formed.  fl(a - b) is monotone in a and in -b, so with both columns ascending the pairs with fl(a_i - b_j) <= t
// are, for every i, a suffix j >= p_i of b, and p_i does not fall as i grows: #{d <= t} is the sum of S2 - p_i.  The order
// statistic of rank r is the value of the smallest order_key k with #{d <= key_value(k)} >= r + 1: a bisection over 64-bit
// keys between the keys of the smallest and the largest difference, at most 64 counts.  The three bisections share their
// passes over the columns.
//
// One 256-thread workgroup per column pair; dynamic LDS: the S1 + S2 draws, 8 bytes each -- as order_keys while they are
// sorted, as doubles after.  The sort is the bitonic network in its all-ascending form (the first stage of every merge pairs
// i with its mirror image in the block): a key past the end of the column would be the largest and stay where it is, so the
// pairs that reach past the end are skipped and no padding to a power of two is stored -- two 5 000-draw columns take 80 KB,
// two workgroups per CU, where kernels_diagnose_rank.hip's padded rank_sort would take 128 KB and leave one.
// A count: every thread takes every 256th a_i and finds p_i by a binary search over b, four of them at a time (measured
// against a chunk of consecutive a_i per thread with one search and a walk, which is seven times slower: DESIGN.md 19).
// Plain C++, f64 subtraction and comparison only; every barrier in workgroup-uniform control flow
// (the bisections' bounds are the same numbers in every thread).
#include <hip/hip_runtime.h>

#include "compare_pairs.hpp"
#include "compare_pairs_device.hpp"
#include "device.hpp"
#include "order_key.hpp"
#include "text_digits.hpp"

namespace miso {

// Grid (events, kmax), one workgroup per column pair; out: pairs_words(n_tau) 64-bit words per (event, isoform) at
// (col_off[ev] + k) * pairs_words(n_tau) (compare_pairs.hpp; col_off[ev] with PAIRS_SKIP_EVENT set: not finite, nothing read).  The host refuses S1, S2 outside [1, 8192] and sizes the
// dynamic LDS: (S1 + S2) * 8 bytes.
__global__ __launch_bounds__(256) void compare_pairs_kernel(const DevEvent *events1, const unsigned char *pool1, int S1,
                                                            const DevEvent *events2, const unsigned char *pool2, int S2,
                                                            int n_events, PairsArgs pa, int as_text, const uint64_t *col_off,
                                                            uint64_t *out) {
  extern __shared__ uint64_t pairs_lds[];
  __shared__ PairsScratch sc;
  const int ev = blockIdx.x, kk = blockIdx.y;
  if (ev >= n_events) return;
  const DevEvent E1 = events1[ev], E2 = events2[ev];
  if (kk >= E1.K) return;
  const double *x1 = reinterpret_cast<const double *>(pool1 + E1.off_samples) + kk;
  const double *x2 = reinterpret_cast<const double *>(pool2 + E2.off_samples) + kk;
  const int W = PAIRS_FIXED_WORDS + pa.n_tau;
  const uint64_t first_col = col_off[ev];
  uint64_t *o = out + ((first_col & ~PAIRS_SKIP_EVENT) + kk) * W;
  const int t = threadIdx.x;
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  const bool skip = (first_col & PAIRS_SKIP_EVENT) != 0;   // (the event's samples were never decoded: nothing of it is read)

  uint64_t *KA = pairs_lds, *KB = KA + S1;
  // as_text: a draw as its `.miso` file prints it and a reader parses it back (text_digits.hpp), so that a run's table is
  // the table of the files it wrote.  (x + 0.0: -0.0 becomes +0.0; the differences compare the same)
  int bad = skip ? 1 : 0;
  for (int e = t; e < (skip ? 0 : S1); e += 256) {
    double v = x1[static_cast<size_t>(e) * E1.K];
    if (as_text && text_rounds(v)) v = static_cast<double>(text_digits(v)) / 10000.0;
    bad |= !(fabs(v) < inf);
    KA[e] = order_key(v + 0.0);
  }
  for (int e = t; e < (skip ? 0 : S2); e += 256) {
    double v = x2[static_cast<size_t>(e) * E2.K];
    if (as_text && text_rounds(v)) v = static_cast<double>(text_digits(v)) / 10000.0;
    bad |= !(fabs(v) < inf);
    KB[e] = order_key(v + 0.0);
  }
  if (__syncthreads_or(bad)) {                        // workgroup-uniform (a skipped event: bad in every thread, below)
    if (t == 0) pairs_not_finite(o, pa.n_tau);
    return;
  }
  pairs_sort(KA, S1);
  pairs_sort(KB, S2);
  double *A = reinterpret_cast<double *>(KA), *B = reinterpret_cast<double *>(KB);
  for (int e = t; e < S1; e += 256) A[e] = key_value(KA[e]);
  for (int e = t; e < S2; e += 256) B[e] = key_value(KB[e]);
  __syncthreads();

  pairs_statistics(A, S1, B, S2, pa, o, sc);
}

}  // namespace miso
