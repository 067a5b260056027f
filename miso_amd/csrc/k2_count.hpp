// k2_count.hpp -- the per-word arithmetic of the single-end two-isoform read loop (kernels_k2.inl gibbs()) and the
// expression that finishes a lane's count, as plain functions for device and host alike; the assembly statements the loop
// issues are the device's fast form of the same functions (kernels_selftest.hip runs the statements one element per thread,
// tools/k2_count_host.cpp the plain functions on the host; the tests compare the two).
//
// A read picks isoform 0 iff its uniform u = x 2^16 + lo is below t = th 2^16 + tl: x < th, or x == th and lo < tl.  The loop
// looks at the high halves x only, two per generator word, and classifies each THREE ways with one saturating subtract:
//   P = th + 1 in both halves;   d = sat(P - x):  0 iff x > th,  1 iff x == th,  >= 2 iff x < th;   c = min(d, 2)
//   acc += c  (per half: 2 * below + on: a plain 32-bit add, the halves never carry into each other -- K2_COUNT_MAX_BLOCKS)
//   o   |= c  (bit 0 of a half of o: some c of that half was 1 -- a read ON the threshold: the trip's flag, k2_flag.hpp)
// Behind the loop a lane holds A = sum of c over its reads = 2 below + E, E its reads on the threshold; the settle path (only
// lanes with a flagged trip) counts E and `more`, those of the E whose low half is below tl:  d0 = (A - E) / 2 + more.
//   th = 0:      P = 1: nothing is below, a half of 0 is on the threshold.  Exact as written.
//   th = 0xFFFF: P = 0x10000 does not fit a half.  The loop runs with P = 0xFFFF: c = 0 is a half of 0xFFFF (ON the threshold,
//                NOT flagged), c = 1 a half of 0xFFFE (below, flagged), c = 2 anything else (below).  A lane that is not
//                flagged and has A == 2 N (N its reads) holds neither: all N are below (k2_count_top_clean); any other lane
//                counts its reads directly behind the loop.
//   th = 65536  (t = 2^32): every read picks isoform 0: closed form, the loop's sums are not looked at.
#pragma once
#include <cstdint>

#include "k2_flag.hpp"

namespace miso {

constexpr uint32_t K2_COUNT_TWO = 0x00020002u;    // the cap of c, both halves
constexpr uint32_t K2_COUNT_ON = 0x00010001u;     // bit 0 of both halves: "on the threshold"
// A half's counter takes at most 8 per block (four words of at most 2): 8191 blocks are 65 528 < 2^16.  The loop empties
// the counters at least that often.
constexpr int K2_COUNT_MAX_BLOCKS = 8191;
constexpr uint32_t K2_COUNT_TOP = 0xFFFFu;        // the high-half threshold whose P = th + 1 does not fit a half

// the loop's subtrahend for high-half threshold th (th <= 65536), replicated into both halves
K2_FLAG_FN uint32_t k2_count_p(uint32_t th) {
  const uint32_t p = th >= K2_COUNT_TOP ? K2_COUNT_TOP : th + 1u;
  return p | (p << 16);
}

// one half: min(sat(p - x), 2)
K2_FLAG_FN uint32_t k2_count_half(uint32_t p, uint32_t x) {
  const uint32_t d = p > x ? p - x : 0u;
  return d < 2u ? d : 2u;
}

// both halves of generator word u (v_pk_sub_u16 P, u clamp; v_pk_min_u16 .., TWO)
K2_FLAG_FN uint32_t k2_count_word(uint32_t P, uint32_t u) {
  return k2_count_half(P & 0xFFFFu, u & 0xFFFFu) | (k2_count_half(P >> 16, u >> 16) << 16);
}

// a word of the loop: inv = the halves that are NOT reads of the chain (0xFFFF each; steady trips: 0).  They count nothing
// and flag nothing.
K2_FLAG_FN void k2_count_step(uint32_t &acc, uint32_t &o, uint32_t P, uint32_t u, uint32_t inv) {
  const uint32_t c = k2_count_word(P, u) & ~inv;
  acc += c;   // v_add_u32
  o |= c;     // v_or_b32
}

// a trip's flag word from its o: at most two bits (k2_flag_note_z)
K2_FLAG_FN uint32_t k2_count_flag(uint32_t o) { return o & K2_COUNT_ON; }

// the two counters of acc together: a lane's A since they were last emptied
K2_FLAG_FN int k2_count_sum(uint32_t acc) { return static_cast<int>(acc & 0xFFFFu) + static_cast<int>(acc >> 16); }

// the lane's reads on isoform 0 from A = 2 below + E, its E reads on the threshold and the `more` of them with lo < tl
// (A - E is even; a lane without a flagged trip has E = more = 0: one shift)
K2_FLAG_FN int k2_count_finish(int A, int E, int more) { return ((A - E) >> 1) + more; }

// th = 0xFFFF: true iff none of the lane's N reads has a high half of 0xFFFE (it would have flagged a trip: n_flagged != 0)
// or 0xFFFF (c = 0: A < 2 N) -- then all N are below the threshold
K2_FLAG_FN bool k2_count_top_clean(int A, uint32_t n_flagged, int N) { return n_flagged == 0u && A == 2 * N; }

#if defined(__HIPCC__)
// The device's fast form.  Two words per statement: THREE operations per word -- sub, min, and half of a three-input add and
// a three-input or that take both words' c at once (v_add3_u32: acc + c_a + c_b, the same 32-bit sum as two adds, the halves
// carry no more than before; v_or3_b32: o | c_a | c_b).  The two subtracts and the two minima are interleaved so that no
// packed operation reads the result of the one before it; the three-input add reads both minima and so follows one directly:
// a dependent pair of these issues like an independent one (profiles/issue_costs_k2.txt).  Inside a statement the hardware's
// interlocks apply; behind a statement of its own the compiler pads with s_nop.
// FIRST: the trip's first pair starts o as c_a | c_b.
// STEADY trips: classification and sums in one statement.
template <bool FIRST>
__device__ __forceinline__ void k2_count_pair(uint32_t &acc, uint32_t &o, uint32_t P, uint32_t two, uint32_t ua, uint32_t ub) {
  uint32_t ca, cb;
  if (FIRST)
    asm("v_pk_sub_u16 %0, %4, %5 clamp\n\tv_pk_sub_u16 %1, %4, %6 clamp\n\t"
        "v_pk_min_u16 %0, %0, %7\n\tv_pk_min_u16 %1, %1, %7\n\t"
        "v_add3_u32 %2, %2, %0, %1\n\tv_or_b32 %3, %0, %1"
        : "=&v"(ca), "=&v"(cb), "+v"(acc), "=&v"(o) : "v"(P), "v"(ua), "v"(ub), "v"(two));
  else
    asm("v_pk_sub_u16 %0, %4, %5 clamp\n\tv_pk_sub_u16 %1, %4, %6 clamp\n\t"
        "v_pk_min_u16 %0, %0, %7\n\tv_pk_min_u16 %1, %1, %7\n\t"
        "v_add3_u32 %2, %2, %0, %1\n\tv_or3_b32 %3, %3, %0, %1"
        : "=&v"(ca), "=&v"(cb), "+v"(acc), "+v"(o) : "v"(P), "v"(ua), "v"(ub), "v"(two));
}
// MASKED trips and single steps: the masks go between the classification and the sums -- two statements, one `and` per word.
template <bool FIRST>
__device__ __forceinline__ void k2_count_pair_masked(uint32_t &acc, uint32_t &o, uint32_t P, uint32_t two, uint32_t ua, uint32_t ub,
                                                     uint32_t inva, uint32_t invb) {
  uint32_t ca, cb;
  asm("v_pk_sub_u16 %0, %2, %3 clamp\n\tv_pk_sub_u16 %1, %2, %4 clamp\n\t"
      "v_pk_min_u16 %0, %0, %5\n\tv_pk_min_u16 %1, %1, %5"
      : "=&v"(ca), "=&v"(cb) : "v"(P), "v"(ua), "v"(ub), "v"(two));
  ca &= ~inva;
  cb &= ~invb;
  if (FIRST)
    asm("v_add3_u32 %0, %0, %2, %3\n\tv_or_b32 %1, %2, %3"
        : "+v"(acc), "=&v"(o) : "v"(ca), "v"(cb));
  else
    asm("v_add3_u32 %0, %0, %2, %3\n\tv_or3_b32 %1, %1, %2, %3"
        : "+v"(acc), "+v"(o) : "v"(ca), "v"(cb));
}
#endif

}  // namespace miso
