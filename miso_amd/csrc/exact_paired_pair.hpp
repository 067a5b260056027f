// exact_paired_pair.hpp -- what the two kernels over PAIRS of paired-end exact-mode posteriors share beside the tables
// (kernels_exact_paired_compare.hip; kernels_exact_paired_delta.hip): the move of wavefront-uniform
// values to scalar registers, the loader of one sample's side of a pair, and the layout of the global rows that keep A's f.
// Included after batch.hpp (ExactPairedCmpSide).  -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "batch.hpp"

#include "exact_paired.hpp"
#include "hip_host.hpp"

namespace miso {

constexpr int EXPC_ROW = EXACT_G + 64;      // doubles of a workgroup's row of A's f: 64 j + l, the grid's last point at 2048; 512-byte rows
constexpr int EXPC_LAUNCH = 8192;           // pairs per launch: bounds the rows' buffer (138 MB)

// A value every lane holds alike, moved to scalar registers (the same bits).  The statistics, windows and table scalars of
// three densities live across five sweeps over the pairs; as vector registers they would not fit beside a sweep's points.
__device__ __forceinline__ double exact_uni(double v) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ ExactStats exact_uni(const ExactStats &s) {
  return ExactStats{exact_uni(s.am1), exact_uni(s.bm1), exact_uni(s.a), exact_uni(s.b), exact_uni(s.c), exact_uni(s.n), exact_uni(s.e0), exact_uni(s.e1)};
}
__device__ __forceinline__ ExactTable exact_uni(const ExactTable &T) {
  return ExactTable{exact_uni(T.tm), exact_uni(T.gmax), exact_uni(T.tL), exact_uni(T.tR), exact_uni(T.h), exact_uni(T.Z), exact_uni(T.mean0),
                    exact_uni(T.mean1), exact_uni(T.sf), T.F, T.f};
}

struct ExactUni {
  template <class T> __device__ __forceinline__ T operator()(const T &v) const { return exact_uni(v); }
};

// pair i of one sample: its statistics and c8, in scalar registers, and its drawing pairs
__device__ __forceinline__ void exact_paired_cmp_side(const ExactPairedCmpSide &sd, const int32_t *list, int i, ExactStats &st, double &c8,
                                                      ExactPairs &pr) {
  exact_paired_element(sd.stats6, sd.mm, sd.offs, sd.in_pool, sd.events, list, sd.frag_prob, sd.il, i, st, c8, pr, ExactUni());
}

// Host: one sample's side of the n pairs as the kernels take it -- the statistics uploaded on the call's stream, and EITHER the
// caller-given probabilities (n_pairs of them: exact_paired_check's count) OR the batch's device pointers as they are
inline ExactPairedCmpSide exact_paired_cmp_upload(HipCall &call, const ExactPairedCmpInput &I, int n, int64_t n_pairs) {
  ExactPairedCmpSide sd{};
  sd.stats6 = call.upload(I.stats6, static_cast<size_t>(n) * 6 * 8);
  if (I.m) {
    sd.mm = call.upload(I.m, static_cast<size_t>(n_pairs) * 2 * 8);
    sd.offs = call.upload(I.offs, static_cast<size_t>(n + 1) * 8);
  } else {
    sd.events = I.events; sd.in_pool = I.in_pool; sd.frag_prob = I.frag_prob; sd.il = I.il;
  }
  return sd;
}

}  // namespace miso
