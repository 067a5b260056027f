// compare_pairs.hpp -- what compare_pairs_kernel (kernels_compare_pairs.hip) and its host driver (runtime.hip
// miso_batch::compare_pairs) agree on: the limits, the call's arguments and the layout of a column's results.
#pragma once
#include <stdint.h>

namespace miso {

// draws per column at most: both sorted columns stay in LDS, 2 * 8192 * 8 bytes = 128 KB of a workgroup's 160 KB
constexpr int PAIRS_MAX_DRAWS = 8192;
constexpr int PAIRS_MAX_TAU = 4;
// pooled draws per column and group at most in compare_pairs_groups_kernel (kernels_compare_pairs_groups.hip): one sorted
// group stays in LDS, 16384 * 8 bytes = 128 KB, the other in global memory; M <= 2^28, ranks and counts fit 32 bits
constexpr int PAIRS_GROUP_MAX_DRAWS = 16384;

// the three order statistics' ranks over the S1 * S2 differences (median, ci_low, ci_high) and the thresholds
struct PairsArgs {
  uint32_t rank[3];
  int32_t n_tau;
  double tau[PAIRS_MAX_TAU];
};

// the top bit of an event's column offset as the kernel gets it: the event's columns are not read and come back not finite
constexpr uint64_t PAIRS_SKIP_EVENT = 0x8000000000000000ull;

// A column's results, in 64-bit words: the bits of median, ci_low, ci_high; n_gt0, n_lt0; finite; then n_abs_ge per threshold
constexpr int PAIRS_FIXED_WORDS = 6;
inline int pairs_words(int n_tau) { return PAIRS_FIXED_WORDS + n_tau; }

}  // namespace miso
