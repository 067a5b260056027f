// exact_paired.hpp -- the paired-end exact-posterior mode's device functions (the scheme is described in
// kernels_exact_paired.hip; kernels_exact_paired_compare.hip, DESIGN.md 18, tabulates the product of two such densities with
// them).  Built on exact_posterior.hpp, which it leaves as it is: ExactStats / exact_point with e = A give the pair-free part
// of the density, exact_invert the inverse of the table.  Also what both units need of an element: its drawing pairs, c8, the
// loader of a (stats6, pairs) element and the workgroup's LDS layout.  -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "exact_posterior.hpp"

namespace miso {

constexpr int EXP_BLOCK = 16;          // drawing pairs whose factors are multiplied before one log
constexpr int EXP_CHUNK = 64;          // drawing pairs staged in LDS at a time (one per lane)
constexpr int EXP_PASSES = 2;          // window passes
constexpr int EXP_PASS_PTS = 8;        // points per lane in a window pass: 512 in all
constexpr int EXP_TAB_PTS = 8;         // points per lane and sweep of the table: 4 sweeps for the lane's 32 points, then one point more
constexpr int EXP_ROW_PTS = 8;         // sample rows per lane and sweep

// The event's drawing pairs: its records in the plain layout (one u32 per pair, f0 | f1 << 16, indices into the batch's
// fragment-length probabilities fp[il]) -- or, the selftest, the probabilities themselves (mm[2 r], mm[2 r + 1]).
struct ExactPairs {
  const uint32_t *rec;
  const double *fp;
  int il;
  const double *mm;
  int n;
};

// the drawing pairs of a resident event: its plain records (u16 f0, f1 per pair) in the batch's input pool
__device__ __forceinline__ ExactPairs exact_pairs_resident(const unsigned char *in_pool, const DevEvent &E, const double *fp, int il) {
  return ExactPairs{reinterpret_cast<const uint32_t *>(in_pool + E.off_draw), fp, il, nullptr, E.n_draw};
}

// (n + h0 + h1) / 32 from hyper - 1 (exact_paired_window's c8)
__device__ __forceinline__ double exact_paired_c8(double n, double hm0, double hm1) {
  return (n + ((hm0 + 1.0) + (hm1 + 1.0))) * 0.03125;
}

// Element i as the probe and compare kernels take it: statistics and c8 from row i of stats6 = {n10, n01, A0, A1, h0, h1} and
// the number of its drawing pairs, which are EITHER caller-given probabilities (mm != null; offs[i], offs[i + 1] bound them) OR
// the records of the resident event list[i] of a batch (in_pool, events, fp, il).  (The sampling kernel and the summaries' probe
// take a resident event's statistics from the batch's pool instead: kernels_exact_paired.hip exact_paired_event.)
// uni: what the caller makes of the statistics and of c8 before it keeps them -- nothing (ExactAsIs), or the comparison's move to
// scalar registers (kernels_exact_paired_compare.hip exact_uni).  A parameter, applied to the expressions themselves: with the
// move made afterwards by a wrapper the comparison kernel came out laid out differently and 0.5 % slower on a thousand pairs.
struct ExactAsIs {
  template <class T> __device__ __forceinline__ T operator()(const T &v) const { return v; }
};
template <class Uni = ExactAsIs>
__device__ __forceinline__ void exact_paired_element(const double *stats6, const double *mm, const int64_t *offs, const unsigned char *in_pool,
                                                     const DevEvent *events, const int32_t *list, const double *fp, int il, int i,
                                                     ExactStats &st, double &c8, ExactPairs &pr, Uni uni = Uni()) {
  const double *q = stats6 + 6 * static_cast<size_t>(i);
  if (mm) {
    pr.rec = nullptr; pr.fp = nullptr; pr.il = 0;
    pr.mm = mm + 2 * static_cast<size_t>(offs[i]); pr.n = static_cast<int>(offs[i + 1] - offs[i]);
  } else {
    pr = exact_pairs_resident(in_pool, events[list[i]], fp, il);
  }
  const double nn = (q[0] + q[1]) + static_cast<double>(pr.n), hm0 = q[4] - 1.0, hm1 = q[5] - 1.0;
  st = uni(exact_stats(q[0], q[1], nn, q[2], q[3], hm0, hm1));
  c8 = uni(exact_paired_c8(nn, hm0, hm1));
}

// the workgroup's LDS: one F / f pair (37 KB), the reductions' and the staged pairs' buffers, f at the points -1 and G + 1
struct ExactPairedLds {
  double F[EXACT_PAD], f[EXACT_PAD], red[256], mbuf[2 * EXP_CHUNK], fext[2];
  int redi[128];
};

// pairs [base, base + cnt) of the event -> mbuf[2 i], mbuf[2 i + 1]; lane i brings pair base + i
__device__ __forceinline__ void exact_pairs_stage(const ExactPairs &p, int base, int cnt, double *mbuf, int lane) {
  __syncthreads();   // (the chunk before has been read by every lane)
  if (lane < cnt) {
    double m0, m1;
    if (p.mm) {
      m0 = p.mm[2 * static_cast<size_t>(base + lane)];
      m1 = p.mm[2 * static_cast<size_t>(base + lane) + 1];
    } else {
      const uint32_t r = p.rec[base + lane];
      const int top = p.il - 1;
      const int f0 = static_cast<int>(r & 0xFFFFu), f1 = static_cast<int>(r >> 16);
      m0 = p.fp[f0 < top ? f0 : top];   // (the packer admits indices below il only; a drawing pair has both)
      m1 = p.fp[f1 < top ? f1 : top];
    }
    mbuf[2 * lane] = m0; mbuf[2 * lane + 1] = m1;
  }
  __syncthreads();
}

// P[j] = sum over the event's drawing pairs of log(x[j] m0 + y[j] m1) at the lane's NP points: the factors of the pairs
// [16 b, 16 b + 16) multiplied in pair order from 1.0, one log per block, the logs added in block order from 0.0.
// Called by the whole wavefront (barriers inside); exactly p.n records are read.
template <int NP>
__device__ __forceinline__ void exact_pair_logsum(const ExactPairs &p, double *mbuf, int lane, const double (&x)[NP],
                                                  const double (&y)[NP], double (&P)[NP]) {
#pragma unroll
  for (int j = 0; j < NP; j++) P[j] = 0.0;
  for (int base = 0; base < p.n; base += EXP_CHUNK) {
    const int cnt = p.n - base < EXP_CHUNK ? p.n - base : EXP_CHUNK;
    exact_pairs_stage(p, base, cnt, mbuf, lane);
    for (int b0 = 0; b0 < cnt; b0 += EXP_BLOCK) {
      const int nb = cnt - b0 < EXP_BLOCK ? cnt - b0 : EXP_BLOCK;
      double pr[NP];
#pragma unroll
      for (int j = 0; j < NP; j++) pr[j] = 1.0;
      if (nb == EXP_BLOCK) {
#pragma unroll
        for (int i = 0; i < EXP_BLOCK; i++) {
          const double m0 = mbuf[2 * (b0 + i)], m1 = mbuf[2 * (b0 + i) + 1];   // (one address for all lanes: a broadcast)
#pragma unroll
          for (int j = 0; j < NP; j++) pr[j] = pr[j] * (x[j] * m0 + y[j] * m1);
        }
      } else {
        for (int i = 0; i < nb; i++) {
          const double m0 = mbuf[2 * (b0 + i)], m1 = mbuf[2 * (b0 + i) + 1];
#pragma unroll
          for (int j = 0; j < NP; j++) pr[j] = pr[j] * (x[j] * m0 + y[j] * m1);
        }
      }
#pragma unroll
      for (int j = 0; j < NP; j++) P[j] = P[j] + miso_det_log(pr[j]);
    }
  }
}

// A density has one segment -- one sample's statistics and pairs (s, p below; kernels_exact_paired.hip) -- or two: the
// product of two samples' densities of one event (kernels_exact_paired_compare.hip), whose second segment
// brings its own denominator term and its own pair sum:
//     g12 = ((((0 - lin) - c L) - n1 ld1) - n2 ld2) + (P1 + P2),   c = (a + b) - (n1 + n2),
// s then holding the pooled exponents and that c, with n and e0, e1 of sample 1.  Each sample's pairs go in their own
// blocks of sixteen, sample 1 first.  ExactOneSegment adds nothing, and the code is what it was without the parameter.
struct ExactOneSegment {
  __device__ __forceinline__ void point(double, const ExactPoint &, double &) const {}
  template <int NP>
  __device__ __forceinline__ void pairs(double *, int, const double (&)[NP], const double (&)[NP], double (&)[NP]) const {}
};
struct ExactSecondSegment {
  double n, e0, e1;   // sample 2's pair count and A0, A1
  ExactPairs p;       // ... and drawing pairs
  __device__ __forceinline__ void point(double t, const ExactPoint &pt, double &g) const {
    const double E = miso_det_exp(-pt.at);
    const double Ee0 = E * e0, Ee1 = E * e1;
    const double den = t >= 0.0 ? e0 + Ee1 : Ee0 + e1;
    g = g - n * miso_det_log(den);
  }
  template <int NP>
  __device__ __forceinline__ void pairs(double *mbuf, int lane, const double (&x)[NP], const double (&y)[NP], double (&P)[NP]) const {
    double P2[NP];
    exact_pair_logsum<NP>(p, mbuf, lane, x, y, P2);
#pragma unroll
    for (int j = 0; j < NP; j++) P[j] = P[j] + P2[j];
  }
};

// g, x, 1 - x at the lane's NP logit-space points
template <int NP, class Seg2 = ExactOneSegment>
__device__ __forceinline__ void exact_paired_eval(const ExactStats &s, const ExactPairs &p, double *mbuf, int lane,
                                                  const double (&t)[NP], double (&g)[NP], double (&x)[NP], double (&y)[NP],
                                                  const Seg2 &seg2 = Seg2()) {
#pragma unroll
  for (int j = 0; j < NP; j++) {
    const ExactPoint pt = exact_point(s, t[j]);
    x[j] = pt.x; y[j] = pt.y; g[j] = pt.g;
    seg2.point(t[j], pt, g[j]);
  }
  double P[NP];
  exact_pair_logsum<NP>(p, mbuf, lane, x, y, P);
  seg2.template pairs<NP>(mbuf, lane, x, y, P);
#pragma unroll
  for (int j = 0; j < NP; j++) g[j] = g[j] + P[j];
}

// Steps 1 - 2: the window [tL, tR] and gref (in T.gmax; T.tm is the window's middle, nothing is made of it).
// c8 = (n + h0 + h1) / 32: g'' >= -4 c8 everywhere, so between two grid points d apart g exceeds the larger of the two by
// at most c8 d^2.  red: 64 doubles, redi: 128 ints of LDS.
template <class Seg2 = ExactOneSegment>
__device__ __forceinline__ ExactTable exact_paired_window(const ExactStats &s, double c8, const ExactPairs &p, double *mbuf,
                                                          double *red, int *redi, int lane, const Seg2 &seg2 = Seg2()) {
  ExactTable T;
  double lo = -EXACT_T_MODE, hi = EXACT_T_MODE, gref = 0.0;
  constexpr int NPTS = 64 * EXP_PASS_PTS;
  for (int pass = 0; pass < EXP_PASSES; pass++) {
    const double d = (hi - lo) / static_cast<double>(NPTS - 1);
    double t[EXP_PASS_PTS], g[EXP_PASS_PTS], x[EXP_PASS_PTS], y[EXP_PASS_PTS];
#pragma unroll
    for (int j = 0; j < EXP_PASS_PTS; j++) t[j] = lo + d * static_cast<double>(EXP_PASS_PTS * lane + j);
    exact_paired_eval<EXP_PASS_PTS>(s, p, mbuf, lane, t, g, x, y, seg2);
    double m = g[0];
#pragma unroll
    for (int j = 1; j < EXP_PASS_PTS; j++) m = g[j] > m ? g[j] : m;
    __syncthreads();
    red[lane] = m;
    __syncthreads();
    double gm = red[0];
    for (int l = 1; l < 64; l++) { const double v = red[l]; gm = v > gm ? v : gm; }
    const double thr = gm - (EXACT_DROP + c8 * (d * d));
    int first = NPTS, last = -1;
#pragma unroll
    for (int j = 0; j < EXP_PASS_PTS; j++) {
      const int i = EXP_PASS_PTS * lane + j;
      if (g[j] >= thr) { first = i < first ? i : first; last = i > last ? i : last; }
    }
    redi[lane] = first; redi[64 + lane] = last;
    __syncthreads();
    for (int l = 0; l < 64; l++) {
      const int a = redi[l], b = redi[64 + l];
      first = a < first ? a : first; last = b > last ? b : last;
    }
    if (last >= first) {   // (always: the pass's largest point is kept)
      const double nlo = first <= 0 ? lo : lo + d * static_cast<double>(first - 1);
      const double nhi = last >= NPTS - 1 ? hi : lo + d * static_cast<double>(last + 1);
      lo = nlo; hi = nhi;
    }
    gref = gm;
  }
  T.tL = lo; T.tR = hi; T.gmax = gref; T.tm = 0.5 * (lo + hi);
  T.h = (T.tR - T.tL) / static_cast<double>(EXACT_G);
  T.Z = 0.0; T.mean0 = 0.0; T.mean1 = 0.0; T.sf = 0.0;
  T.F = nullptr; T.f = nullptr;
  return T;
}

// Step 3: the table on the window.  F, f: EXACT_PAD doubles of LDS each, red: 256, fext: 2 (f at the points -1 and G + 1).
template <class Seg2 = ExactOneSegment>
__device__ __forceinline__ ExactTable exact_paired_table(const ExactStats &s, ExactTable T, const ExactPairs &p, double *mbuf,
                                                         double *F, double *f, double *fext, double *red, int lane,
                                                         const Seg2 &seg2 = Seg2()) {
  const double h = T.h, h24 = h / 24.0;
  const int i0 = EXACT_CELLS * lane;
  double ax = 0.0, ay = 0.0, af = 0.0;
  // the lane's 32 points (its cells' left ends) in four sweeps of 8 over the pairs ...
  for (int sw = 0; sw < EXACT_CELLS / EXP_TAB_PTS; sw++) {
    double t[EXP_TAB_PTS], g[EXP_TAB_PTS], x[EXP_TAB_PTS], y[EXP_TAB_PTS];
#pragma unroll
    for (int j = 0; j < EXP_TAB_PTS; j++) t[j] = T.tL + h * static_cast<double>(i0 + EXP_TAB_PTS * sw + j);
    exact_paired_eval<EXP_TAB_PTS>(s, p, mbuf, lane, t, g, x, y, seg2);
#pragma unroll
    for (int j = 0; j < EXP_TAB_PTS; j++) {
      const int i = i0 + EXP_TAB_PTS * sw + j;
      const double fi = miso_det_exp(g[j] - T.gmax);
      f[exact_idx(i)] = fi;
      const double wf = (i == 0 ? 0.5 : 1.0) * fi;
      ax = ax + x[j] * wf; ay = ay + y[j] * wf; af = af + wf;
    }
  }
  // ... and one more sweep for the three points left over: the grid's last (lane 63; the lanes 2 .. 62 make it too and drop
  // it), the point before the window (lane 0), the point behind it (lane 1)
  {
    const int i = lane == 0 ? -1 : (lane == 1 ? EXACT_G + 1 : EXACT_G);
    double t[1], g[1], x[1], y[1];
    t[0] = T.tL + h * static_cast<double>(i);
    exact_paired_eval<1>(s, p, mbuf, lane, t, g, x, y, seg2);
    const double fi = miso_det_exp(g[0] - T.gmax);
    if (lane == 63) {
      f[exact_idx(EXACT_G)] = fi;
      const double wf = 0.5 * fi;
      ax = ax + x[0] * wf; ay = ay + y[0] * wf; af = af + wf;
    } else if (lane < 2) {
      fext[lane] = fi;
    }
  }
  __syncthreads();
  // a cell's mass: the derivative-free fourth-order rule h/24 (-f[-1] + 13 f[0] + 13 f[1] - f[2])
  double acc = 0.0;
  double fm = i0 == 0 ? fext[0] : f[exact_idx(i0 - 1)], f0 = f[exact_idx(i0)], f1 = f[exact_idx(i0 + 1)];
  for (int j = 0; j < EXACT_CELLS; j++) {
    const int i = i0 + j;
    const double f2 = i + 2 > EXACT_G ? fext[1] : f[exact_idx(i + 2)];
    double cell = h24 * ((13.0 * (f0 + f1) - fm) - f2);
    cell = cell < 0.0 ? 0.0 : cell;
    acc = acc + cell;
    F[exact_idx(i + 1)] = acc;
    fm = f0; f0 = f1; f1 = f2;
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

}  // namespace miso
