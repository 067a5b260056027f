// order_key.hpp -- doubles as order-preserving 64-bit keys: the radix select of kernels_summary.hip and the sort of
// kernels_diagnose_rank.hip compare these as unsigned integers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace miso {

// (every NaN gets the largest key, whatever its sign bit: numpy's sort -- the reference's, credible_intervals.py:53 --
// puts NaN behind +inf; the bit pattern alone would put a sign-bit NaN in front of -inf)
__device__ __forceinline__ uint64_t order_key(double x) {
  const uint64_t u = __double_as_longlong(x);
  if (x != x) return ~0ull;
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  return __longlong_as_double(u);
}

}  // namespace miso
