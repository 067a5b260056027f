// kernels_exact_paired.hip -- the exact-posterior mode of paired-end two-isoform events (miso_batch_set_exact_paired,
// DESIGN.md 17).
//
// The reference's paired chain (miso_paired.c: Gibbs step 24-86, psi step 88-174, whose read term does not depend on psi)
// has, summed over the pairs' assignments and with x = psi_0, y = 1 - x, the law
//     log p(x) = (n10 + h0 - 1) log x + (n01 + h1 - 1) log y + sum_i log(x m0_i + y m1_i) - n log(x A0 + y A1) + const,
// n10 / n01 the pairs compatible with isoform 0 / 1 only (the packer's base_count), the sum over the drawing pairs (both
// isoforms; m their fragment-length probabilities), n all of them, A_k = exp(assscores_k).  No chain is run: ONE WAVEFRONT
// per event tabulates the density and draws the event's rows from the table, as kernels_exact.hip does for single-end
// events -- but this density is a product over the event's pairs: the hot loop is pairs x grid points.
//
// LOGIT SPACE, as there: t = logit x, g(t) = log p + log x + log y.  The pair-free part is exact_point() with e = A; to it
// comes P(t) = sum_i log(x m0_i + y m1_i).  g may have SEVERAL maxima (g' is a sum of differently shifted sigmoids), so
// nothing here looks for "the" mode.  What is known: g'' >= -(n + h0 + h1) / 4, and for h >= 1 the tails fall at least
// like e^-|t|.
//
// THE SCHEME (every operation in a fixed order, exp / log from miso_detmath.h, no contraction; tests/_exact_paired_ref.py
// restates it operation by operation, the two agree bit for bit, tests/test_gpu_exact_paired.py):
//   P.  The pair sum at a point: the factors x m0 + y m1 of EXP_BLOCK = 16 consecutive pairs are multiplied in pair order,
//       one log per block, the logs added in block order.  Sixteen, because a factor is at least the smallest
//       fragment-length probability, >= 2^-63 by the eligibility rule: sixteen multiply to >= 2^-1008, a normal number;
//       sixty-four need not (4e-6 at +-4 sd already gives 1e-346).  The pairs come 64 at a time through LDS -- lane i
//       fetches record base + i and its two probabilities -- and every lane reads them back at one address (a broadcast)
//       for the points it keeps in registers.  Exactly n_draw records are read: the layouts' padding never enters.
//   1.  EXP_PASSES = 2 window passes.  A pass lays 512 points, 8 per lane, on [lo, hi] (first [-64, 64]), d apart, takes the
//       largest g among them (gref) and keeps the span from one point before the first to one point behind the last with
//       g >= gref - (40 + slack), slack = (n + h0 + h1) / 32 d^2: by the bound on g'' no point between two grid points
//       exceeds the larger of them by more than slack, so the span holds every point with g >= max g - 40, however many
//       maxima there are, and gref is within slack of max g.
//   2.  The table: G = 2048 cells on the last span, f = exp(g - gref) at the 2049 points and one point beyond each end, lane l
//       the points [32 l, 32 l + 32) in four sweeps of 8 over the pairs, the three points left over in a fifth.  A cell's mass is the
//       derivative-free fourth-order rule h/24 (-f[-1] + 13 f[0] + 13 f[1] - f[2]); CDF table, prefix sums and the
//       trapezoid means as kernels_exact.hip's step 3.
//   3.  Inversion: exact_invert (binary search + cubic Hermite on F with slopes h f), unchanged.
//
// Sample s inverts u F[G] at the uniform of (seed, event id, sample s, MISO_SITE_EXACT); logLik[s] is log p at the sample
// with the Dirichlet normaliser (P evaluated at the sample: the pairs are walked once per 512 rows); the assignment is one
// reassignment of the pairs from the last row's psi by the paired pick rule, on the words of the paired sampler's initial
// reassignment of chain 0.
//
// WHERE THE PIECES LIVE.  Steps P, 1, 2, the workgroup's LDS layout, c8 and the loader of a caller-given element:
// exact_paired.hpp (kernels_exact_paired_compare.hip tabulates with them too).  Step 3, the sample's uniform and the chain
// records of a mode without a chain: exact_posterior.hpp, shared with the single-end mode.  The host driver's stream, buffers
// and HIP_OK: hip_host.hpp.  Here: the two kernels, the driver of the posterior stage and the check of caller-given elements
// (exact_paired_check, which the comparison's driver calls as well).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "batch.hpp"
#include "device.hpp"
#include "miso_amd.h"
#include "miso_detmath.h"
#include "miso_philox.h"

#include "exact_paired.hpp"
#include "hip_host.hpp"

namespace miso {

__device__ __forceinline__ ExactTable exact_paired_tabulate(const ExactStats &st, double c8, const ExactPairs &pr, ExactPairedLds &L, int lane) {
  const ExactTable W = exact_paired_window(st, c8, pr, L.mbuf, L.red, L.redi, lane);
  return exact_paired_table(st, W, pr, L.mbuf, L.F, L.f, L.fext, L.red, lane);
}

// the event of slot `slot` of the launch's list: its statistics from the batch's pool (integer counts, the packed hyper - 1)
// and its pairs
__device__ __forceinline__ void exact_paired_event(const KernelArgs &a, const double *A2, int slot, const DevEvent &E, ExactStats &st,
                                                   double &c8, ExactPairs &pr) {
  const double *consts = reinterpret_cast<const double *>(a.in_pool + E.off_consts);
  const int32_t *base = reinterpret_cast<const int32_t *>(a.in_pool + E.off_base);
  const int n10 = base[0], n01 = base[1];
  const double n = static_cast<double>(n10 + n01 + E.n_draw);
  st = exact_stats(static_cast<double>(n10), static_cast<double>(n01), n, A2[2 * slot], A2[2 * slot + 1], consts[4], consts[5]);
  c8 = exact_paired_c8(n, consts[4], consts[5]);
  pr = exact_pairs_resident(a.in_pool, E, a.frag_prob, a.il);
}

// One workgroup = one wavefront = one event of the launch's list.  A2: A0, A1 per event of the list.
__global__ __launch_bounds__(64) void exact_paired_sample(const KernelArgs a, const double *A2, int S) {
  __shared__ ExactPairedLds L;
  const int lane = threadIdx.x;
  const int slot = blockIdx.x;
  if (slot >= a.n_slots) return;   // (uniform: the whole workgroup)
  const int ev = a.slot_event[slot];
  const DevEvent E = a.events[ev];
  const uint32_t event_id = E.has_id ? E.explicit_id : a.first_event_id + static_cast<uint32_t>(ev);
  const double *consts = reinterpret_cast<const double *>(a.in_pool + E.off_consts);
  ExactStats st; double c8; ExactPairs pr;
  exact_paired_event(a, A2, slot, E, st, c8, pr);
  const double lg_sum = consts[6], lg_each = consts[7];
  const ExactTable T = exact_paired_tabulate(st, c8, pr, L, lane);
  double *samples = reinterpret_cast<double *>(a.out_pool + E.off_samples);
  double *loglik = reinterpret_cast<double *>(a.out_pool + E.off_loglik);
  const uint32_t k0 = static_cast<uint32_t>(a.seed), k1 = static_cast<uint32_t>(a.seed >> 32);
  auto sample = [&](int s) { return exact_at(st, exact_invert(T, exact_uniform(s, event_id, k0, k1) * T.Z)); };
  // rows [s0, s0 + 512) per sweep over the pairs: lane l the rows s0 + l + 64 j
  for (int s0 = 0; s0 < S; s0 += 64 * EXP_ROW_PTS) {
    double x[EXP_ROW_PTS], y[EXP_ROW_PTS], base_ll[EXP_ROW_PTS], nld[EXP_ROW_PTS], P[EXP_ROW_PTS];
#pragma unroll
    for (int j = 0; j < EXP_ROW_PTS; j++) {
      const int s = s0 + lane + 64 * j;
      const ExactAt r = sample(s < S ? s : S - 1);   // (rows beyond the last: the last again, not stored)
      x[j] = r.x; y[j] = r.y;
      base_ll[j] = st.am1 * r.lx + st.bm1 * r.ly;
      nld[j] = st.n * r.ldx;
    }
    exact_pair_logsum<EXP_ROW_PTS>(pr, L.mbuf, lane, x, y, P);
#pragma unroll
    for (int j = 0; j < EXP_ROW_PTS; j++) {
      const int s = s0 + lane + 64 * j;
      if (s < S) {
        reinterpret_cast<double2 *>(samples)[s] = make_double2(x[j], y[j]);
        loglik[s] = ((((base_ll[j] + P[j]) - nld[j]) + lg_sum) - lg_each);
      }
    }
  }
  if (S > 0 && E.n_draw > 0) {   // the one reassignment, from the last row's psi (every lane makes that row again)
    const ExactAt r = sample(S - 1);
    uint8_t *drawass = a.out_pool + E.off_drawass;
    const int top = a.il - 1;
    for (int rd = lane; rd < E.n_draw; rd += 64) {
      const miso_u32x4 u = miso_philox4x32(static_cast<uint32_t>(rd >> 2), MISO_ITER_INIT, MISO_SITE_GIBBS, event_id, k0, k1);
      const uint32_t word = (rd & 3) == 0 ? u.v[0] : ((rd & 3) == 1 ? u.v[1] : ((rd & 3) == 2 ? u.v[2] : u.v[3]));
      const uint32_t ff = pr.rec[rd];
      const int f0 = static_cast<int>(ff & 0xFFFFu), f1 = static_cast<int>(ff >> 16);
      const double c0 = 0.0 + r.x * a.frag_prob[f0 < top ? f0 : top];   // (miso_paired.c:11-22, 64-68, as kernels_k2.inl pe_pick)
      const double Tt = c0 + r.y * a.frag_prob[f1 < top ? f1 : top];
      drawass[rd] = miso_u01(word) * Tt < c0 ? 0 : 1;
    }
  }
  exact_chain_stats(reinterpret_cast<ChainStats *>(a.out_pool + E.off_stats), a.C, S, lane);
}

// The posterior stage alone.  mm == null: element i is event i of the launch's list (the summaries of
// miso_batch_get_exact_summary); otherwise caller-given statistics and pairs (miso_selftest_exact_paired).
__global__ __launch_bounds__(64) void exact_paired_probe(const KernelArgs a, const double *A2, const double *stats6, const double *mm,
                                                         const int64_t *offs, int n, const double *prob, int n_prob, double *out8,
                                                         double *icdf) {
  __shared__ ExactPairedLds L;
  const int lane = threadIdx.x;
  const int i = blockIdx.x;
  if (i >= n) return;
  ExactStats st; double c8; ExactPairs pr;
  if (mm) exact_paired_element(stats6, mm, offs, nullptr, nullptr, nullptr, nullptr, 0, i, st, c8, pr);
  else exact_paired_event(a, A2, i, a.events[a.slot_event[i]], st, c8, pr);
  const ExactTable T = exact_paired_tabulate(st, c8, pr, L, lane);
  if (lane == 0) {
    double *o = out8 + 8 * static_cast<size_t>(i);
    o[0] = T.mean0; o[1] = T.mean1; o[2] = T.tL; o[3] = T.tR; o[4] = T.Z; o[5] = T.gmax; o[6] = T.h;
    o[7] = miso_det_log(T.Z) + T.gmax;
  }
  for (int j = lane; j < n_prob; j += 64) {
    const ExactAt r = exact_at(st, exact_invert(T, prob[j] * T.Z));
    icdf[(static_cast<size_t>(i) * n_prob + j) * 2] = r.x;
    icdf[(static_cast<size_t>(i) * n_prob + j) * 2 + 1] = r.y;
  }
}

// n elements as a paired driver takes them from its caller: every row of stats6 eligible; with caller-given pairs (offs !=
// null: m, offs as miso_selftest_exact_paired's) offsets that start at 0 and ascend, probabilities in [2^-63, 1].  Returns the
// number of caller-given pairs.
int64_t exact_paired_check(const double *stats6, const double *m, const int64_t *offs, int n) {
  for (int i = 0; i < n; i++) {
    const double *q = stats6 + 6 * static_cast<size_t>(i);
    if (!(q[0] >= 0 && q[1] >= 0) || !exact_paired_eligible(2, q + 2, q + 4, false))
      MISO_FAIL(MISO_EINVAL, "An element is not eligible for the paired exact mode");
  }
  if (!offs || n <= 0) return 0;
  if (offs[0] != 0) MISO_FAIL(MISO_EINVAL, "The pair offsets must start at 0");
  for (int i = 0; i < n; i++)
    if (offs[i + 1] < offs[i] || offs[i + 1] - offs[i] > INT32_MAX) MISO_FAIL(MISO_EINVAL, "The pair offsets must ascend");
  for (int64_t r = 0; r < 2 * offs[n]; r++)
    if (!(m[r] >= EXACT_PAIRED_MIN_PROB && m[r] <= 1.0)) MISO_FAIL(MISO_EINVAL, "A pair probability outside [2^-63, 1]");
  return offs[n];
}

const void *exact_paired_sample_fn() { return reinterpret_cast<const void *>(&exact_paired_sample); }

// ka != null: the events of ka's list (A2 on the device, stats6 / m / offs unused); otherwise caller-given elements
void exact_paired_probe_run(const KernelArgs *ka, const double *A2, const double *stats6, const double *m, const int64_t *offs,
                            int n, const double *prob, int n_prob, double *out8, double *icdf, hipStream_t st) {
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device");
  if (n < 0 || n_prob < 0) MISO_FAIL(MISO_EINVAL, "Negative element or probability count");
  exact_check_prob(prob, n_prob);
  const int64_t n_pairs = ka ? 0 : exact_paired_check(stats6, m, offs, n);
  if (n == 0) return;
  HipCall call(st);
  const size_t ob = static_cast<size_t>(n) * 8 * 8, qb = static_cast<size_t>(n) * n_prob * 2 * 8;
  const double *d_p = call.upload(prob, static_cast<size_t>(n_prob) * 8);
  double *d_o = call.alloc(ob), *d_q = call.alloc(qb);
  const double *d_st = nullptr, *d_m = nullptr;
  const int64_t *d_off = nullptr;
  if (!ka) {
    d_st = call.upload(stats6, static_cast<size_t>(n) * 6 * 8);
    d_m = call.upload(m, static_cast<size_t>(n_pairs) * 2 * 8);   // (no pair at all: still a buffer, the kernel tells the routes by it)
    d_off = call.upload(offs, static_cast<size_t>(n + 1) * 8);
  }
  KernelArgs none{};
  hipLaunchKernelGGL(exact_paired_probe, dim3(n), dim3(64), 0, call.st, ka ? *ka : none, A2, d_st, d_m, d_off, n, d_p, n_prob, d_o, d_q);
  HIP_OK(hipGetLastError());
  if (out8) HIP_OK(hipMemcpyAsync(out8, d_o, ob, hipMemcpyDeviceToHost, call.st));
  if (icdf && n_prob) HIP_OK(hipMemcpyAsync(icdf, d_q, qb, hipMemcpyDeviceToHost, call.st));
  HIP_OK(hipStreamSynchronize(call.st));
}

}  // namespace miso
