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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "batch.hpp"
#include "device.hpp"
#include "miso_amd.h"
#include "miso_detmath.h"
#include "miso_philox.h"

namespace miso {

constexpr int EXACT_G = 2048;            // cells
constexpr int EXACT_CELLS = EXACT_G / 64;
constexpr double EXACT_DROP = 40.0;
constexpr double EXACT_T_MODE = 64.0, EXACT_T_SPAN = 128.0;
constexpr int EXACT_MODE_ROUNDS = 4, EXACT_EDGE_ROUNDS = 3, EXACT_NEWTON = 4;
// tables in LDS: point i at i + i / 32, so that the lanes' chunks (32 points apart) start on different banks
constexpr int EXACT_PAD = EXACT_G + 1 + EXACT_G / 32;
__device__ __forceinline__ int exact_idx(int i) { return i + (i >> 5); }

struct ExactStats { double am1, bm1, a, b, c, n, e0, e1; };
struct ExactPoint { double g, gp, x, y, L, ld, at; };
struct ExactTable {
  double tm, gmax, tL, tR, h, Z, mean0, mean1;
  const double *F, *f;
};

__device__ __forceinline__ ExactStats exact_stats(double n10, double n01, double n, double e0, double e1, double hm0, double hm1) {
  ExactStats s;
  s.am1 = n10 + hm0; s.bm1 = n01 + hm1;
  s.a = s.am1 + 1.0; s.b = s.bm1 + 1.0;
  s.c = (s.a + s.b) - n;
  s.n = n; s.e0 = e0; s.e1 = e1;
  return s;
}

__device__ __forceinline__ ExactPoint exact_point(const ExactStats &s, double t) {
  ExactPoint p;
  p.at = __builtin_fabs(t);
  const double E = miso_det_exp(-p.at);
  const double s1 = 1.0 + E;
  p.L = miso_det_log(s1);
  const bool pos = t >= 0.0;
  const double r = 1.0 / s1, Er = E / s1;
  p.x = pos ? r : Er;
  p.y = pos ? Er : r;
  const double Ee0 = E * s.e0, Ee1 = E * s.e1;
  const double den = pos ? s.e0 + Ee1 : Ee0 + s.e1;
  p.ld = miso_det_log(den);
  const double lin = (pos ? s.b : s.a) * p.at;
  p.g = ((0.0 - lin) - s.c * p.L) - s.n * p.ld;
  const double q = (pos ? s.e0 : Ee0) / den;
  p.gp = s.a - (s.c * p.x + s.n * q);
  return p;
}

// `rounds` times: the 64 lanes' points inside [lo, hi]; the first at which pred holds closes the new interval
template <class Pred>
__device__ __forceinline__ void exact_section(const ExactStats &s, double &lo, double &hi, int rounds, int lane, Pred pred) {
  for (int r = 0; r < rounds; r++) {
    const double w = (hi - lo) / 65.0;
    const ExactPoint p = exact_point(s, lo + w * static_cast<double>(lane + 1));
    const unsigned long long m = __ballot(pred(p) ? 1 : 0);
    const int idx = m ? __builtin_ctzll(m) : 64;
    const double nlo = idx == 0 ? lo : lo + w * static_cast<double>(idx);
    const double nhi = idx == 64 ? hi : lo + w * static_cast<double>(idx + 1);
    lo = nlo; hi = nhi;
  }
}

// steps 1 - 3 by the workgroup's one wavefront; F, f: EXACT_PAD doubles of LDS each, red: 4 x 64
__device__ __forceinline__ ExactTable exact_tabulate(const ExactStats &s, double *F, double *f, double *red, int lane) {
  ExactTable T;
  double lo = -EXACT_T_MODE, hi = EXACT_T_MODE;
  exact_section(s, lo, hi, EXACT_MODE_ROUNDS, lane, [](const ExactPoint &p) { return !(p.gp > 0.0); });
  T.tm = 0.5 * (lo + hi);
  T.gmax = exact_point(s, T.tm).g;
  const double thr = T.gmax - EXACT_DROP;
  lo = T.tm - EXACT_T_SPAN; hi = T.tm;
  exact_section(s, lo, hi, EXACT_EDGE_ROUNDS, lane, [thr](const ExactPoint &p) { return p.g >= thr; });
  T.tL = lo;
  lo = T.tm; hi = T.tm + EXACT_T_SPAN;
  exact_section(s, lo, hi, EXACT_EDGE_ROUNDS, lane, [thr](const ExactPoint &p) { return p.g < thr; });
  T.tR = hi;
  const double h = (T.tR - T.tL) / static_cast<double>(EXACT_G);
  const double hh = 0.5 * h, h12 = (h * h) / 12.0;
  T.h = h;
  const int i0 = EXACT_CELLS * lane;
  double ax = 0.0, ay = 0.0, af = 0.0, acc = 0.0, f_prev, d_prev;
  {
    const ExactPoint p = exact_point(s, T.tL + h * static_cast<double>(i0));
    f_prev = miso_det_exp(p.g - T.gmax);
    d_prev = f_prev * p.gp;
    f[exact_idx(i0)] = f_prev;
    const double wf = (i0 == 0 ? 0.5 : 1.0) * f_prev;
    ax = ax + p.x * wf; ay = ay + p.y * wf; af = af + wf;
  }
  for (int j = 1; j <= EXACT_CELLS; j++) {
    const int i = i0 + j;
    const ExactPoint p = exact_point(s, T.tL + h * static_cast<double>(i));
    const double fi = miso_det_exp(p.g - T.gmax), di = fi * p.gp;
    double cell = hh * (f_prev + fi) + h12 * (d_prev - di);
    cell = cell < 0.0 ? 0.0 : cell;
    acc = acc + cell;
    F[exact_idx(i)] = acc;
    if (j < EXACT_CELLS || lane == 63) {   // the next lane's first point; the last lane owns the grid's last point too
      f[exact_idx(i)] = fi;
      const double wf = (j < EXACT_CELLS ? 1.0 : 0.5) * fi;
      ax = ax + p.x * wf; ay = ay + p.y * wf; af = af + wf;
    }
    f_prev = fi; d_prev = di;
  }
  red[lane] = acc; red[64 + lane] = ax; red[128 + lane] = ay; red[192 + lane] = af;
  if (lane == 0) F[0] = 0.0;
  __syncthreads();
  double off = 0.0, sx = 0.0, sy = 0.0, sf = 0.0;
  for (int m = 0; m < 64; m++) {
    if (m < lane) off = off + red[m];
    sx = sx + red[64 + m]; sy = sy + red[128 + m]; sf = sf + red[192 + m];
  }
  for (int j = 1; j <= EXACT_CELLS; j++) F[exact_idx(i0 + j)] = off + F[exact_idx(i0 + j)];
  __syncthreads();
  T.Z = F[exact_idx(EXACT_G)];
  T.mean0 = sx / sf; T.mean1 = sy / sf;
  T.F = F; T.f = f;
  return T;
}

// step 4: the logit-space point at which the tabulated CDF takes the value `target`
__device__ __forceinline__ double exact_invert(const ExactTable &T, double target) {
  int lo = 0, hi = EXACT_G;
  for (int it = 0; it < 11; it++) {
    const int mid = (lo + hi) >> 1;
    const bool le = T.F[exact_idx(mid)] <= target;
    lo = le ? mid : lo;
    hi = le ? hi : mid;
  }
  const int j = lo;   // 0 .. G - 1
  const double F0 = T.F[exact_idx(j)], F1 = T.F[exact_idx(j + 1)];
  const double m0 = T.h * T.f[exact_idx(j)], m1 = T.h * T.f[exact_idx(j + 1)];
  const double dF = F1 - F0, R = target - F0;
  double s = dF > 0.0 ? R / dF : 0.5;
  s = s > 1.0 ? 1.0 : s;
  s = s < 0.0 ? 0.0 : s;
  const double c2 = (3.0 * dF - 2.0 * m0) - m1, c3 = (m0 + m1) - 2.0 * dF;
  for (int it = 0; it < EXACT_NEWTON; it++) {
    const double r = (m0 + s * (c2 + s * c3)) * s - R;
    const double dp = m0 + s * (2.0 * c2 + (3.0 * c3) * s);
    s = dp > 0.0 ? s - r / dp : s;
    s = s > 1.0 ? 1.0 : s;
    s = s < 0.0 ? 0.0 : s;
  }
  return T.tL + T.h * (static_cast<double>(j) + s);
}

// x, 1 - x and log x, log(1 - x), log(x e0 + (1 - x) e1) at a logit-space point
struct ExactAt { double x, y, lx, ly, ldx; };
__device__ __forceinline__ ExactAt exact_at(const ExactStats &s, double t) {
  const ExactPoint p = exact_point(s, t);
  const bool pos = t >= 0.0;
  const double nL = 0.0 - p.L, naL = (0.0 - p.at) - p.L;
  ExactAt r;
  r.x = p.x; r.y = p.y;
  r.lx = pos ? nL : naL;
  r.ly = pos ? naL : nL;
  r.ldx = p.ld - p.L;
  return r;
}

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
  auto sample = [&](int s) {
    const miso_u32x4 w = miso_philox4x32(static_cast<uint32_t>(s), 0u, MISO_SITE_EXACT, event_id, k0, k1);
    const double u = (static_cast<double>(w.v[0]) + 0.5) * (1.0 / 4294967296.0);
    return exact_at(st, exact_invert(T, u * T.Z));
  };
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
  // no chain ran: every sample counts as accepted, dealt over the chains' records so that they add up to S
  ChainStats *cs = reinterpret_cast<ChainStats *>(a.out_pool + E.off_stats);
  for (int c = lane; c < a.C; c += 64) {
    cs[c].counts_hash = 0;
    cs[c].accepted = (S + a.C - 1 - c) / a.C;
    cs[c].hw_id = __builtin_amdgcn_s_getreg((31 << 11) | 4);
  }
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

#define HIP_OK(call)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess)                                                                  \
      MISO_FAIL(MISO_ENODEVICE, std::string(#call) + ": " + hipGetErrorString(e_));        \
  } while (0)

// (st: the stream to work on -- a batch's own; null: one of this call's, so that no other stream of the process waits)
void exact_probe_run(const double *stats7, int n, const double *prob, int n_prob, double *out8, double *icdf, hipStream_t st) {
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device");
  if (n < 0 || n_prob < 0) MISO_FAIL(MISO_EINVAL, "Negative element or probability count");
  for (int j = 0; j < n_prob; j++) if (!(prob[j] > 0.0 && prob[j] < 1.0)) MISO_FAIL(MISO_EINVAL, "A probability must lie inside (0, 1)");
  if (n == 0) return;
  struct Held {   // freed on every way out, a failed call's included
    double *p[4] = {nullptr, nullptr, nullptr, nullptr};
    hipStream_t own = nullptr;
    ~Held() { for (double *q : p) if (q) (void) hipFree(q); if (own) (void) hipStreamDestroy(own); }
  } held;
  if (!st) { HIP_OK(hipStreamCreateWithFlags(&held.own, hipStreamNonBlocking)); st = held.own; }
  double *&d_st = held.p[0], *&d_p = held.p[1], *&d_o = held.p[2], *&d_q = held.p[3];
  const size_t nq = static_cast<size_t>(n) * std::max(n_prob, 1) * 2;
  HIP_OK(hipMalloc(reinterpret_cast<void **>(&d_st), static_cast<size_t>(n) * 7 * 8));
  HIP_OK(hipMalloc(reinterpret_cast<void **>(&d_p), std::max(n_prob, 1) * 8));
  HIP_OK(hipMalloc(reinterpret_cast<void **>(&d_o), static_cast<size_t>(n) * 8 * 8));
  HIP_OK(hipMalloc(reinterpret_cast<void **>(&d_q), nq * 8));
  HIP_OK(hipMemcpyAsync(d_st, stats7, static_cast<size_t>(n) * 7 * 8, hipMemcpyHostToDevice, st));
  if (n_prob) HIP_OK(hipMemcpyAsync(d_p, prob, static_cast<size_t>(n_prob) * 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(exact_probe, dim3(n), dim3(64), 0, st, d_st, n, d_p, n_prob, d_o, d_q);
  HIP_OK(hipGetLastError());
  if (out8) HIP_OK(hipMemcpyAsync(out8, d_o, static_cast<size_t>(n) * 8 * 8, hipMemcpyDeviceToHost, st));
  if (icdf && n_prob) HIP_OK(hipMemcpyAsync(icdf, d_q, static_cast<size_t>(n) * n_prob * 2 * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
}

}  // namespace miso
