// detmath_n.hpp -- miso_detmath.h's exp / log for N arguments at once, coefficients in the caller's registers (device code).
#pragma once
#include "miso_detmath.h"

#pragma clang fp contract(off)

namespace miso {
namespace {

// ---- several arguments through one routine, statement by statement (round 5) ----
// A chain per lane is ONE dependency chain: with 625 wavefronts on 1024 SIMDs nothing else issues on a wavefront's
// SIMD, and the eleven transcendental routines of a Metropolis-Hastings step (miso.c:449-552) -- Horner chains of a dozen
// fused multiply-adds each -- ran one after the other at the latency of a dependent f64 operation, ~10 cycles per
// instruction (hipcc does not interleave two calls of miso_det_log: each reads its coefficient table behind a volatile
// barrier).  det_log_n / det_exp_n evaluate N arguments with the operations of miso_det_log / miso_det_exp
// (include/miso_detmath.h) in the same order PER ARGUMENT -- the same bits -- but step by step across the arguments, so
// that N independent chains are in flight.  The coefficients come from the CALLER's registers (kept in VGPRs for the whole
// run: sampler_lane<true>): miso_detmath.h reads them from constant memory at every call so that kernels with two or three
// wavefronts per SIMD keep their occupancy, but a wavefront alone on its SIMD then waits out a scalar-cache round trip
// two or three times per call -- 119 scalar loads and 78 waits in the kernel, most of them in the iteration loop.
template <int N> __device__ __forceinline__ void det_exp_n(const double (&x)[N], double (&out)[N], const double (&te)[12]) {
  const double LOG2E = 1.4426950408889634074;
  const double LN2_HI = 6.93147180369123816490e-01;
  const double LN2_LO = 1.90821492927058770002e-10;
  double xm[N], kd[N], r[N], p[N];
  int k[N];
#pragma unroll
  for (int j = 0; j < N; j++) {
    xm[j] = (x[j] != x[j]) ? 0.0 : x[j];
    xm[j] = (xm[j] > 710.0) ? 710.0 : xm[j];
    xm[j] = (xm[j] < -746.0) ? -746.0 : xm[j];
    kd[j] = __builtin_floor(xm[j] * LOG2E + 0.5);
    k[j] = static_cast<int>(kd[j]);
    r[j] = miso_fma(-kd[j], LN2_HI, xm[j]);
    r[j] = miso_fma(-kd[j], LN2_LO, r[j]);
  }
#pragma unroll
  for (int j = 0; j < N; j++) p[j] = te[0];
#pragma unroll
  for (int i = 1; i < 12; i++) {
#pragma unroll
    for (int j = 0; j < N; j++) p[j] = miso_fma(p[j], r[j], te[i]);
  }
#pragma unroll
  for (int j = 0; j < N; j++) {
    p[j] = miso_fma(p[j], r[j], 1.0);
    p[j] = miso_fma(p[j], r[j], 1.0);
    const int k1 = k[j] / 2, k2 = k[j] - k1;
    double res = p[j] * miso_pow2i(k1) * miso_pow2i(k2);
    res = (x[j] > 709.782712893384) ? miso_u2d(0x7FF0000000000000ull) : res;
    res = (x[j] < -745.2) ? 0.0 : res;
    res = (x[j] != x[j]) ? x[j] : res;
    out[j] = res;
  }
}

template <int N> __device__ __forceinline__ void det_log_n(const double (&x)[N], double (&out)[N], const double (&tl)[12]) {
  const double LN2_HI = 6.93147180369123816490e-01;
  const double LN2_LO = 1.90821492927058770002e-10;
  const double SQRT2 = 1.41421356237309504880;
  double f[N], s[N], z[N], q[N], ed[N];
#pragma unroll
  for (int j = 0; j < N; j++) {
    const int sub = (miso_d2u(x[j]) >> 52) == 0;
    const double xs = sub ? x[j] * 18014398509481984.0 : x[j];
    const uint64_t u = miso_d2u(xs);
    int e = static_cast<int>((u >> 52) & 0x7FF) - 1023 + (sub ? -54 : 0);
    double m = miso_u2d((u & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);
    const int big = m > SQRT2;
    m = big ? m * 0.5 : m;
    e += big ? 1 : 0;
    f[j] = m - 1.0;
    s[j] = f[j] / (2.0 + f[j]);
    z[j] = s[j] * s[j];
    ed[j] = static_cast<double>(e);
  }
#pragma unroll
  for (int j = 0; j < N; j++) q[j] = tl[0];
#pragma unroll
  for (int i = 1; i < 12; i++) {
#pragma unroll
    for (int j = 0; j < N; j++) q[j] = miso_fma(q[j], z[j], tl[i]);
  }
#pragma unroll
  for (int j = 0; j < N; j++) {
    const double R = z[j] * q[j];
    double res = miso_fma(ed[j], LN2_HI, f[j] - (s[j] * (f[j] - R) - ed[j] * LN2_LO));
    res = (miso_d2u(x[j]) == 0x7FF0000000000000ull) ? x[j] : res;
    res = (x[j] == 0.0) ? miso_u2d(0xFFF0000000000000ull) : res;
    res = (x[j] < 0.0) ? miso_u2d(0x7FF8000000000000ull) : res;
    res = (x[j] != x[j]) ? x[j] : res;
    out[j] = res;
  }
}

// miso_det_sqrt for a positive, normal, finite argument (the only kind the binomial's set-up has: n r q >= 5): the same
// operations without the special cases' branches, so that it sits in one basic block with what runs beside it
__device__ __forceinline__ double det_sqrt_pos(double x) {
  const uint64_t u = miso_d2u(x);
  int e = static_cast<int>(u >> 52) - 1023;
  const int odd = e & 1;
  e = (e - odd) / 2;
  const double m = miso_u2d((u & 0x000FFFFFFFFFFFFFull) | (static_cast<uint64_t>(1023 + odd) << 52));
  double y = 1.1547 - 0.1634 * m;
  y = y * (1.5 - 0.5 * m * y * y);
  y = y * (1.5 - 0.5 * m * y * y);
  y = y * (1.5 - 0.5 * m * y * y);
  y = y * (1.5 - 0.5 * m * y * y);
  y = y * (1.5 - 0.5 * m * y * y);
  double g = m * y;
  const double h = 0.5 * y;
  double d = miso_fma(-g, g, m);
  g = miso_fma(d, h, g);
  d = miso_fma(-g, g, m);
  g = miso_fma(d, h, g);
  return g * miso_pow2i(e);
}

// the two coefficient tables into VGPRs, pinned (the empty asm keeps the compiler from re-reading them from constant memory
// where they are used)
__device__ __forceinline__ void det_tables_to_registers(double (&te)[12], double (&tl)[12]) {
#pragma unroll
  for (int i = 0; i < 12; i++) {
    double ve = miso_tab_exp[i], vl = miso_tab_log[i];
    asm volatile("" : "+v"(ve), "+v"(vl));
    te[i] = ve; tl[i] = vl;
  }
}
__device__ __forceinline__ double det_exp_t(double x, const double (&te)[12]) {
  const double in[1] = {x};
  double o[1];
  det_exp_n<1>(in, o, te);
  return o[0];
}
__device__ __forceinline__ double det_log_t(double x, const double (&tl)[12]) {
  const double in[1] = {x};
  double o[1];
  det_log_n<1>(in, o, tl);
  return o[0];
}

// ---- the Metropolis-Hastings step's exp / log without the special cases, where none applies ----
// det_exp_fast / det_log_fast are det_exp_n<1> / det_log_n<1> statement for statement, less the selects whose condition is
// false on the routine's domain: identities, not approximations -- on the domain the result has the full routine's bits
// (tests/test_gpu_fast_detmath.py).  det_exp_r / det_log_r choose the route per wavefront.
//
// det_exp_fast: |x| <= 700 (a NaN fails the compare).
//   * xm = (x != x) ? 0 : x               x is not a NaN
//   * xm = (xm > 710) ? 710 : xm          x <= 700
//   * xm = (xm < -746) ? -746 : xm        x >= -700: so xm == x
//   * res = (x > 709.78...) ? +inf : res  x <= 700
//   * res = (x < -745.2) ? 0 : res        x >= -700
//   * res = (x != x) ? x : res            x is not a NaN
//   k = floor(x log2(e) + 0.5) lies in [-1010, 1010], so k1, k2 lie in [-505, 505] and miso_pow2i's argument is in range.
__device__ __forceinline__ double det_exp_fast(double x, const double (&te)[12]) {
  const double LOG2E = 1.4426950408889634074;
  const double LN2_HI = 6.93147180369123816490e-01;
  const double LN2_LO = 1.90821492927058770002e-10;
  const double kd = __builtin_floor(x * LOG2E + 0.5);
  const int k = static_cast<int>(kd);
  double r = miso_fma(-kd, LN2_HI, x);
  r = miso_fma(-kd, LN2_LO, r);
  double p = te[0];
#pragma unroll
  for (int i = 1; i < 12; i++) p = miso_fma(p, r, te[i]);
  p = miso_fma(p, r, 1.0);
  p = miso_fma(p, r, 1.0);
  const int k1 = k / 2, k2 = k - k1;
  return p * miso_pow2i(k1) * miso_pow2i(k2);
}

// det_log_fast: x positive, normal and finite (class "positive normal").
//   * sub = (bits >> 52) == 0             the exponent field of a normal number is not 0: sub == 0, so xs == x and e takes no -54
//   * res = (bits == +inf) ? x : res      x is finite
//   * res = (x == 0) ? -inf : res         x is normal, not 0
//   * res = (x < 0) ? NaN : res           x is positive
//   * res = (x != x) ? x : res            x is not a NaN
//   The `big` select (m > sqrt 2) belongs to the ordinary path and stays.
__device__ __forceinline__ double det_log_fast(double x, const double (&tl)[12]) {
  const double LN2_HI = 6.93147180369123816490e-01;
  const double LN2_LO = 1.90821492927058770002e-10;
  const double SQRT2 = 1.41421356237309504880;
  const uint64_t u = miso_d2u(x);
  int e = static_cast<int>((u >> 52) & 0x7FF) - 1023;
  double m = miso_u2d((u & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);
  const int big = m > SQRT2;
  m = big ? m * 0.5 : m;
  e += big ? 1 : 0;
  const double f = m - 1.0;
  const double s = f / (2.0 + f);
  const double z = s * s;
  const double ed = static_cast<double>(e);
  double q = tl[0];
#pragma unroll
  for (int i = 1; i < 12; i++) q = miso_fma(q, z, tl[i]);
  const double R = z * q;
  return miso_fma(ed, LN2_HI, f - (s * (f - R) - ed * LN2_LO));
}

// The route, per wavefront: the fast routine when EVERY active lane's argument is in its domain (one compare; its lane mask
// is tested on the scalar side), the full routine for the whole wavefront otherwise.  Call in wave-uniform control flow only.
// full: whether the wavefront took the full route (tests, MISO_K2_ROUTE_COUNT).
// force_full (KernelArgs::k2_full_math, tests: every call down the full route) is not a mask of its own OR-ed into the
// test -- a 64-bit scalar that a kernel short of scalar registers fetched back with two v_readlane before every call -- but
// folded into the operand the compare reads anyway, made once per kernel (DetRoute) and held in vector registers: exp's
// bound, which under the hook is negative, so that every |x| fails it; log's class mask, which under the hook names
// every class.
struct DetRoute {
  double exp_bound;     // |x| <= exp_bound: det_exp_fast
  uint32_t log_outside; // classes (v_cmp_class) that send det_log_r down the full route
};
__device__ __forceinline__ DetRoute det_route(bool force_full) {
  DetRoute r;
  r.exp_bound = force_full ? -1.0 : 700.0;
  r.log_outside = force_full ? 0x3FFu : (0x3FFu & ~0x100u);   // every class but "positive normal" (0x100)
  asm volatile("" : "+v"(r.exp_bound), "+v"(r.log_outside));  // vector registers, not rebuilt from the scalar flag at the calls
  return r;
}
__device__ __forceinline__ double det_exp_r(double x, const double (&te)[12], const DetRoute &rt, bool &full) {
  full = __builtin_amdgcn_ballot_w64(!(__builtin_fabs(x) <= rt.exp_bound)) != 0;
  if (!full) return det_exp_fast(x, te);
  return det_exp_t(x, te);
}
__device__ __forceinline__ double det_log_r(double x, const double (&tl)[12], const DetRoute &rt, bool &full) {
  // every class but "positive normal": NaNs, infinities, negatives, zeros, subnormals.  Written as the one
  // instruction it is: the ballot of __builtin_amdgcn_class compiles to three (compare, select 0 / 1, compare).
  // The compare reads EXEC implicitly: an inactive lane's bit is 0, so it counts as inside the domain, as in a ballot.
  // (Not volatile: device inline assembly is convergent, and every caller is in wave-uniform control flow.)
  uint64_t outside;
  asm("v_cmp_class_f64_e64 %0, %1, %2" : "=s"(outside) : "v"(x), "v"(rt.log_outside));
  full = outside != 0;
  if (!full) return det_log_fast(x, tl);
  return det_log_t(x, tl);
}

}  // namespace
}  // namespace miso
