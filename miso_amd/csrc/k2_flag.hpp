// k2_flag.hpp -- the bookkeeping of the single-end two-isoform read loop (kernels_k2.inl gibbs()) that is not per-read
// arithmetic, as plain functions for device and host alike: which trips held a read ON the threshold.  No compare, no
// select, no lane mask: it runs on the loop's always-taken path.
// (kernels_selftest.hip runs them one element per thread, tools/k2_flag_host.cpp on the host.)
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define K2_FLAG_FN __host__ __device__ __forceinline__
#else
#define K2_FLAG_FN inline
#endif

namespace miso {

// A trip's running minimum m of x ^ th over its words, both 16-bit halves: a half of m is zero iff a read of the trip sits
// on the threshold.  z = (m - 0x00010001) & ~m & 0x80008000 is non-zero iff a half of m is zero (exact as a whole; bit 31
// is also set by the borrow of a zero LOW half into a high half equal to 1).  `n` counts z's bits over the lane's trips,
// `s` sums their stride positions, each as often as its trip has bits.
//   n == 0: no trip of the lane is flagged.   n == 1: exactly one is, with one bit, and s IS its position.
//   n >= 2: several trips -- or one trip with two bits: both halves on the threshold, or a low half on it under a high half
//           of 1 (about 3e-8 per trip together): the caller rescans all of the lane's blocks, which is always correct.
// Bounds: a trip adds at most 2 to n and a lane makes at most n_draw / 8 + 1 < 2^28 trips and single steps per Gibbs step, so
// n stays below 2^29 and never wraps to "none".  s may wrap: it is read only when n == 1, when it is a single term.  The
// position goes through a 24-bit multiply: exact for k < 2^24.  The largest the kernels produce is k < npos <= n_draw / 8 + 1
// (one lane walking a whole chain; a chain of 10^5 reads: 12 500; the loop's chunk: 16 000); a lane with more than 2^24
// positions -- over 1.3e8 reads -- does not trust s and rescans (gibbs(): `npos <= K2_FLAG_MAX_POS`).
constexpr int K2_FLAG_MAX_POS = 1 << 24;
struct K2Flag { uint32_t n = 0, s = 0; };

K2_FLAG_FN uint32_t k2_mul24(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul24(a, b);
#else
  return (a & 0xFFFFFFu) * (b & 0xFFFFFFu);
#endif
}

// note the trip or single step that began at stride position k (k < 2^24) and whose flag word is z: at most two bits, non-zero
// iff a read of the trip sits on the threshold (the read loop's z: k2_count.hpp k2_count_flag)
K2_FLAG_FN void k2_flag_note_z(K2Flag &f, uint32_t z, uint32_t k) {
  const uint32_t c = static_cast<uint32_t>(__builtin_popcount(z));
  f.n += c;
  f.s += k2_mul24(c, k);
}

// the same from a running minimum m of x ^ th
K2_FLAG_FN void k2_flag_note(K2Flag &f, uint32_t m, uint32_t k) {
  k2_flag_note_z(f, (m - 0x00010001u) & ~m & 0x80008000u, k);
}

enum { K2_FLAG_NONE = 0, K2_FLAG_ONE = 1, K2_FLAG_MANY = 2 };

// behind the loop: none / exactly one flagged trip, at position `pos` / more than one (rescan)
K2_FLAG_FN int k2_flag_read(const K2Flag &f, uint32_t &pos) {
  pos = f.s;
  return f.n == 0 ? K2_FLAG_NONE : (f.n == 1 ? K2_FLAG_ONE : K2_FLAG_MANY);
}

// the halves of word w of a partial block of rem reads that are NOT reads (rem = 0: no partial block, all of them)
K2_FLAG_FN uint32_t k2_part_inv(int rem, int w) {
  return (2 * w < rem ? 0u : 0xFFFFu) | (2 * w + 1 < rem ? 0u : 0xFFFF0000u);
}

}  // namespace miso
