// exact_delta_groups.hpp -- what the two units that pool the exact quantiles of delta psi over GROUPS of replicates share
// (kernels_exact_delta_groups.hip, single-end; kernels_exact_paired_delta_groups.hip, paired-end, DESIGN.md
// 20b): the limits, the layout of a replicate's row of the global workspace with its stores and loads, and the launch of
// exact_groups_update, which lives in the single-end unit and only reads rows and the pairs' H.  -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "exact_delta.hpp"

namespace miso {

constexpr int EXACT_GROUP_MAX = 8;                                  // replicates a group
// a replicate's row of the workspace, in doubles: F, f, then {tm, gmax, tL, tR, h, Z, mean0, mean1, sf}, the window's width in
// psi, {am1, bm1, a, b, c, n, e0, e1}
constexpr int EXACT_GROUPS_SCALARS = 18;
constexpr int EXACT_GROUPS_ROW = 2 * EXACT_PAD + EXACT_GROUPS_SCALARS;
// the sweeps of the first launch: slot 0 H(0.0), slot 1 round 1, slot 2 the caller's points; later slot k = probability k
constexpr int EXACT_GROUPS_FIRST_SLOTS = 3;
// what one launch range holds on the device at most (workspace, the pairs' H and the brackets)
constexpr size_t EXACT_GROUPS_WORK_BYTES = size_t{256} << 20;

__device__ __forceinline__ void exact_groups_store_scalars(double *s, const ExactTable &T, double w, const ExactStats &st) {
  s[0] = T.tm; s[1] = T.gmax; s[2] = T.tL; s[3] = T.tR; s[4] = T.h; s[5] = T.Z; s[6] = T.mean0; s[7] = T.mean1; s[8] = T.sf;
  s[9] = w;
  s[10] = st.am1; s[11] = st.bm1; s[12] = st.a; s[13] = st.b; s[14] = st.c; s[15] = st.n; s[16] = st.e0; s[17] = st.e1;
}
__device__ __forceinline__ ExactTable exact_groups_load_table(const double *s, const double *F, const double *f) {
  ExactTable T;
  T.tm = s[0]; T.gmax = s[1]; T.tL = s[2]; T.tR = s[3]; T.h = s[4]; T.Z = s[5]; T.mean0 = s[6]; T.mean1 = s[7]; T.sf = s[8];
  T.F = F; T.f = f;
  return T;
}
__device__ __forceinline__ ExactStats exact_groups_load_stats(const double *s) {
  ExactStats st;
  st.am1 = s[10]; st.bm1 = s[11]; st.a = s[12]; st.b = s[13]; st.c = s[14]; st.n = s[15]; st.e0 = s[16]; st.e1 = s[17];
  return st;
}

// kernels_exact_delta_groups.hip: exact_groups_update on `st` for the ne events of a range, (ne n_p + 63) / 64 workgroups
void exact_groups_update_launch(hipStream_t st, const double *ws, const double *Hp, const double *prob, int n_p, int n_z, int n1, int n2,
                                int ne, int n_slots, int round, ExactBracket *br, double *out);

}  // namespace miso
