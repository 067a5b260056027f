// exact_posterior.hpp -- the exact-posterior mode's device functions: the density of psi of a single-end
// two-isoform event in logit space, its mode and window, its table on 2049 points, the inverse of the tabulated CDF.
// Shared by kernels_exact.hip (the mode itself; the scheme is described there), kernels_exact_compare.hip (two such
// posteriors compared; exact_compare.hpp) and, through exact_paired.hpp, the paired-end mode, whose sampling
// kernel draws its uniforms and fills its chain records with the two functions at the end.  Units that include it are built
// with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "device.hpp"
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
  double tm, gmax, tL, tR, h, Z, mean0, mean1, sf;   // (sf: the trapezoid sum of f the means are divided by)
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

// steps 1 - 2 by the workgroup's one wavefront: the mode and the window (tm, gmax, tL, tR, h of the result)
__device__ __forceinline__ ExactTable exact_window(const ExactStats &s, int lane) {
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
  T.h = (T.tR - T.tL) / static_cast<double>(EXACT_G);
  T.Z = 0.0; T.mean0 = 0.0; T.mean1 = 0.0; T.sf = 0.0;
  T.F = nullptr; T.f = nullptr;
  return T;
}

// step 3 on a window: the table; F, f: EXACT_PAD doubles of LDS each, red: 4 x 64
__device__ __forceinline__ ExactTable exact_table(const ExactStats &s, ExactTable T, double *F, double *f, double *red, int lane) {
  const double h = T.h;
  const double hh = 0.5 * h, h12 = (h * h) / 12.0;
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
  T.mean0 = sx / sf; T.mean1 = sy / sf; T.sf = sf;
  T.F = F; T.f = f;
  return T;
}

// steps 1 - 3
__device__ __forceinline__ ExactTable exact_tabulate(const ExactStats &s, double *F, double *f, double *red, int lane) {
  return exact_table(s, exact_window(s, lane), F, f, red, lane);
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

// the uniform of sample s: (word + 0.5) 2^-32, word 0 of Philox(key = seed (k0, k1), ctr = (s, 0, MISO_SITE_EXACT, event id))
__device__ __forceinline__ double exact_uniform(int s, uint32_t event_id, uint32_t k0, uint32_t k1) {
  const miso_u32x4 w = miso_philox4x32(static_cast<uint32_t>(s), 0u, MISO_SITE_EXACT, event_id, k0, k1);
  return (static_cast<double>(w.v[0]) + 0.5) * (1.0 / 4294967296.0);
}

// no chain ran: every sample counts as accepted, dealt over the C chains' records so that they add up to S
__device__ __forceinline__ void exact_chain_stats(ChainStats *cs, int C, int S, int lane) {
  for (int c = lane; c < C; c += 64) {
    cs[c].counts_hash = 0;
    cs[c].accepted = (S + C - 1 - c) / C;
    cs[c].hw_id = __builtin_amdgcn_s_getreg((31 << 11) | 4);
  }
}

}  // namespace miso
