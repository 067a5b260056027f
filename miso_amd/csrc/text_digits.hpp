// text_digits.hpp -- a sample as its `.miso` file prints it: the digits of "%.4f" (kernels_summary.hip summarize_column<.., TEXT>;
// kernels_selftest.hip runs the routine on its own, miso_selftest_text_digits).
#pragma once

#include <hip/hip_runtime.h>

namespace miso {

// TEXT: summarise what summarize_miso READS, not what the sampler computed: the reference's summaries come from the
// `.miso` file (samples_utils.py:130-262 -> credible_intervals.py), where every sample is the text "%.4f" of psi.
// k = psi x 10^4 rounded to the nearest integer, ties to even, decided on the EXACT product (fma gives the rounding
// error of the multiplication), which is what a correctly rounded "%.4f" prints; the value read back is the double
// nearest to k / 10^4 = the correctly rounded quotient.  The mean is then the exact integer sum of the k over
// S x 10^4 (correctly rounded; numpy's pairwise float sum of the same values agrees to the last bit or two).
//
// v x 10^4 = p + e exactly, r = rint(p), a = p - r (exact, |a| <= 1/2).  p, r and 1/2 lie on the grid of ulp(p) and
// |e| <= ulp(p) / 2, so |a| < 1/2 leaves |a + e| < 1/2 and r stands.  Only |a| = 1/2 needs e, and there its SIGN
// decides: rint went to the even neighbour, the exact product lies beyond the half when e points away from r, and is
// a true tie (r even: stays) when e = 0.  The SUM a + e must not be formed: it is not exact -- for |e| below half an
// ulp of 1/2 it rounds back to +-1/2 and reads as a tie (the nearest doubles to 5e-05, 0.00025, 0.00035, 0.00095 and
// 0.00645 came out one digit off that way; tests/test_gpu_text_digits.py).
// Exact for |v| < 2^38 (p below 2^52, where it still has a fraction to round).
__device__ __forceinline__ long long text_digits(double v) {
  const double p = v * 10000.0;
  const double e = __builtin_fma(v, 10000.0, -p);        // v x 10^4 = p + e exactly
  double r = __builtin_rint(p);                          // nearest, ties to even
  const double a = p - r;
  if (a == 0.5 && e > 0.0) r = r + 1.0;
  else if (a == -0.5 && e < 0.0) r = r - 1.0;
  return static_cast<long long>(r);
}

// The values text_digits rounds.  The rest is read back as it is: nan and +-inf print as themselves, and from 2^52 on a
// double is an integer, which "%.4f" prints digit for digit.  In between (2^38 <= |v| < 2^52, nothing a posterior sample
// can be) "%.4f" does round and this does not: DESIGN.md section 8.
__device__ __forceinline__ bool text_rounds(double v) { return __builtin_fabs(v) < 274877906944.0; }   // 2^38; false for NaN

}  // namespace miso
