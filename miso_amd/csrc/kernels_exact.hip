// kernels_exact.hip -- the exact-posterior mode of single-end two-isoform events (miso_batch_set_exact).
//
// With x = psi_0 the reference's joint score (miso.c:124-182, 243-307) summed over the assignments of the reads is a
// density of one variable,
//     log p(x) = (n10 + h0 - 1) log x + (n01 + h1 - 1) log(1 - x) - n log(x e0 + (1 - x) e1) + const,
// n10 / n01 the reads compatible with isoform 0 / 1 only, n all reads with a compatible isoform, e the effective lengths,
// h the Dirichlet hyperparameters.  No chain is run: ONE WAVEFRONT per event tabulates the density once and draws the
// event's samples from the table, each an independent draw.
//
// LOGIT SPACE.  t = logit x, density g(t) = log p(x(t)) + log x + log(1 - x) = a t - c log(1 + e^t) - n log(e0 e^t + e1),
// a = n10 + h0, b = n01 + h1, c = a + b - n.  For h >= 1 it has one mode and tails that fall at least like e^(a t) and
// e^(-b t), also when the mass sits at psi ~ 1e-5.  Everything comes from E = exp(-|t|) <= 1: x and 1 - x are 1 / (1 + E)
// and E / (1 + E) (the small one keeps its relative precision), log x and log(1 - x) are -L and -|t| - L with
// L = log(1 + E), and the denominator is (e0 + E e1) / (1 + E) or (E e0 + e1) / (1 + E).
//
// THE SCHEME (every operation in a fixed order; exp / log from miso_detmath.h, no contraction: tests/_exact_ref.py restates
// it operation by operation and the two agree bit for bit, tests/test_gpu_exact.py):
//   1. the mode: g' = a - c x - n q (q = x e0 / (x e0 + (1 - x) e1)) changes sign once.  EXACT_MODE_ROUNDS times the 64
//      lanes evaluate g' at 64 points inside the interval, from [-64, 64], and the first lane with g' <= 0 closes the next
//      interval (1/65 of the last); the mode is the last interval's middle, gmax = g there;
//   2. the window [tL, tR] on which g >= gmax - EXACT_DROP, each end by EXACT_EDGE_ROUNDS such rounds within 128 of the mode;
//   3. G = 2048 cells of width h on it: f = exp(g - gmax) and f' = f g' at the 2049 points, lane l the cells [32 l, 32 l + 32).
//      A cell's mass is the trapezoid with its end-point correction, h/2 (f0 + f1) + h^2/12 (f0' - f1'); the CDF table F is
//      their running sum: sequential within a lane's 32 cells, then the lanes' totals added in lane order 0, 1, 2 ...;
//      the mean of x and of 1 - x are plain trapezoid sums over all points (spectrally accurate on such a bump), a lane's
//      own points in order, then the lanes in order;
//   4. a value T of the CDF is inverted by a binary search for its cell (11 steps) and, inside the cell, the cubic Hermite
//      interpolant of F (values F0, F1, slopes h f0, h f1) solved for T by EXACT_NEWTON Newton steps from the linear guess.
// Measured against mpmath at 40 digits (tests/test_exact_ref.py): posterior mean within 3e-15, quantiles within 6e-9 in psi.
//
// Sample s inverts u F[G], u = (word + 0.5) 2^-32, word = word 0 of Philox(key = seed, ctr = (s, 0, MISO_SITE_EXACT,
// event id)); its row holds x and 1 - x, logLik[s] the MARGINAL score at the sample -- log p above with the Dirichlet
// normaliser lgamma(h0 + h1) - lgamma(h0) - lgamma(h1), not a joint score with an assignment.  The returned assignment is
// one per-read reassignment from the LAST sample's psi, drawn as algorithm = MARGINAL draws its one (kernels_marginal.hip:
// Gibbs words of chain 0, MISO_ITER_INIT).
//
// WHERE THE PIECES LIVE.  The device functions of steps 1 - 4, the sample's uniform and the chain records of a mode without
// a chain: exact_posterior.hpp (the paired-end mode, kernels_exact_paired.hip, uses them too).  The host driver's stream,
// buffers and HIP_OK: hip_host.hpp.  Here: the two kernels, the driver of the posterior stage and the check of its
// probabilities (exact_check_prob, which the paired driver calls as well).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "batch.hpp"
#include "device.hpp"
#include "miso_amd.h"
#include "miso_detmath.h"
#include "miso_philox.h"

#include "exact_posterior.hpp"
#include "hip_host.hpp"

namespace miso {

// One workgroup = one wavefront = one event of the launch's list.  eff: e0, e1 per event of the list.
__global__ __launch_bounds__(64) void exact_sample(const KernelArgs a, const double *eff, int S) {
  __shared__ double F[EXACT_PAD], f[EXACT_PAD], red[256];
  const int lane = threadIdx.x;
  const int slot = blockIdx.x;
  if (slot >= a.n_slots) return;   // (uniform: the whole workgroup)
  const int ev = a.slot_event[slot];
  const DevEvent E = a.events[ev];
  const uint32_t event_id = E.has_id ? E.explicit_id : a.first_event_id + static_cast<uint32_t>(ev);
  const double *consts = reinterpret_cast<const double *>(a.in_pool + E.off_consts);
  const int32_t *base = reinterpret_cast<const int32_t *>(a.in_pool + E.off_base);
  const int n10 = base[0], n01 = base[1];
  const ExactStats st = exact_stats(static_cast<double>(n10), static_cast<double>(n01), static_cast<double>(n10 + n01 + E.n_draw),
                                    eff[2 * slot], eff[2 * slot + 1], consts[4], consts[5]);   // (hyper - 1 at [2K, 3K), K = 2)
  const double lg_sum = consts[6], lg_each = consts[7];
  const ExactTable T = exact_tabulate(st, F, f, red, lane);
  double *samples = reinterpret_cast<double *>(a.out_pool + E.off_samples);
  double *loglik = reinterpret_cast<double *>(a.out_pool + E.off_loglik);
  const uint32_t k0 = static_cast<uint32_t>(a.seed), k1 = static_cast<uint32_t>(a.seed >> 32);
  auto sample = [&](int s) { return exact_at(st, exact_invert(T, exact_uniform(s, event_id, k0, k1) * T.Z)); };
  for (int s = lane; s < S; s += 64) {   // consecutive lanes, consecutive rows of the K x S column-major sample matrix
    const ExactAt r = sample(s);
    reinterpret_cast<double2 *>(samples)[s] = make_double2(r.x, r.y);   // one 16-byte store per row (the pool's offsets are multiples of 16)
    loglik[s] = (((st.am1 * r.lx + st.bm1 * r.ly) - st.n * r.ldx) + lg_sum) - lg_each;
  }
  if (S > 0 && E.n_draw > 0) {   // the one reassignment, from the last sample's psi (every lane makes that sample again)
    const ExactAt r = sample(S - 1);
    const double total = (0.0 + r.x) + r.y;
    uint8_t *drawass = a.out_pool + E.off_drawass;
    for (int rd = lane; rd < E.n_draw; rd += 64) {
      const uint32_t word = miso_split_word(a.seed, event_id, 0u, MISO_ITER_INIT, static_cast<uint32_t>(rd));
      const double rnd = miso_u01(word) * total;
      drawass[rd] = rnd < r.x ? 0 : 1;
    }
  }
  exact_chain_stats(reinterpret_cast<ChainStats *>(a.out_pool + E.off_stats), a.C, S, lane);
}

// the posterior stage alone (miso_selftest_exact; the summaries of miso_batch_get_exact_summary)
__global__ __launch_bounds__(64) void exact_probe(const double *stats7, int n, const double *prob, int n_prob, double *out8,
                                                  double *icdf) {
  __shared__ double F[EXACT_PAD], f[EXACT_PAD], red[256];
  const int lane = threadIdx.x;
  const int i = blockIdx.x;
  if (i >= n) return;
  const double *q = stats7 + 7 * static_cast<size_t>(i);
  const ExactStats st = exact_stats(q[0], q[1], q[2], q[3], q[4], q[5] - 1.0, q[6] - 1.0);
  const ExactTable T = exact_tabulate(st, F, f, red, lane);
  if (lane == 0) {
    double *o = out8 + 8 * static_cast<size_t>(i);
    o[0] = T.mean0; o[1] = T.mean1; o[2] = T.tL; o[3] = T.tR; o[4] = T.Z; o[5] = T.tm; o[6] = T.h; o[7] = T.gmax;
  }
  for (int j = lane; j < n_prob; j += 64) {
    const ExactAt r = exact_at(st, exact_invert(T, prob[j] * T.Z));
    icdf[(static_cast<size_t>(i) * n_prob + j) * 2] = r.x;
    icdf[(static_cast<size_t>(i) * n_prob + j) * 2 + 1] = r.y;
  }
}

// the probabilities at which a posterior stage inverts its CDF
void exact_check_prob(const double *prob, int n_prob) {
  for (int j = 0; j < n_prob; j++) if (!(prob[j] > 0.0 && prob[j] < 1.0)) MISO_FAIL(MISO_EINVAL, "A probability must lie inside (0, 1)");
}

// (st: the stream to work on -- a batch's own; null: one of this call's, so that no other stream of the process waits)
void exact_probe_run(const double *stats7, int n, const double *prob, int n_prob, double *out8, double *icdf, hipStream_t st) {
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device");
  if (n < 0 || n_prob < 0) MISO_FAIL(MISO_EINVAL, "Negative element or probability count");
  exact_check_prob(prob, n_prob);
  if (n == 0) return;
  HipCall call(st);
  const size_t sb = static_cast<size_t>(n) * 7 * 8, ob = static_cast<size_t>(n) * 8 * 8, qb = static_cast<size_t>(n) * n_prob * 2 * 8;
  const double *d_st = call.upload(stats7, sb), *d_p = call.upload(prob, static_cast<size_t>(n_prob) * 8);
  double *d_o = call.alloc(ob), *d_q = call.alloc(qb);
  hipLaunchKernelGGL(exact_probe, dim3(n), dim3(64), 0, call.st, d_st, n, d_p, n_prob, d_o, d_q);
  HIP_OK(hipGetLastError());
  if (out8) HIP_OK(hipMemcpyAsync(out8, d_o, ob, hipMemcpyDeviceToHost, call.st));
  if (icdf && n_prob) HIP_OK(hipMemcpyAsync(icdf, d_q, qb, hipMemcpyDeviceToHost, call.st));
  HIP_OK(hipStreamSynchronize(call.st));
}

}  // namespace miso
