// kernels_selftest.hip -- the device functions the samplers are built from, callable one element per thread over host
// arrays (include/miso_amd.h miso_selftest_*; tests/test_gpu_primitives.py).  This unit includes the samplers' .inl files
// for their anonymous-namespace routines and instantiates none of their kernels: test-only surface, no sampler's code
// changes with it.  One thread per element, 256 threads per workgroup, bounded work per thread.  Also here: the summaries'
// "%.4f" rounding (text_digits.hpp, shared with kernels_summary.hip; tests/test_gpu_text_digits.py).
#include "kernels_k2.inl"
#include "kernels_flat.inl"
#include "kernels_grp.inl"

#include <vector>

#include "hip_host.hpp"
#include "host.hpp"
#include "text_digits.hpp"

#pragma clang fp contract(off)

namespace miso {

namespace {

// argument j of element i is point (i + j stride) mod n: a mix-up between the interleaved chains of det_*_n shows
template <int N, bool LOG> __device__ __forceinline__ void st_detmath_n(const double *x, int n, int stride, int i, double *out,
                                                                         const double (&te)[12], const double (&tl)[12]) {
  double in[N], o[N];
#pragma unroll
  for (int j = 0; j < N; j++) in[j] = x[static_cast<int>((static_cast<long long>(i) + static_cast<long long>(j) * stride) % n)];
  if (LOG) det_log_n<N>(in, o, tl);
  else det_exp_n<N>(in, o, te);
#pragma unroll
  for (int j = 0; j < N; j++) out[static_cast<size_t>(i) * N + j] = o[j];
}

}  // namespace

__global__ void __launch_bounds__(256) selftest_detmath_n_kernel(int fn, int width, const double *x, int n, int stride, double *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double te[12], tl[12];
  det_tables_to_registers(te, tl);
  if (i >= n) return;
  switch (fn * 8 + width) {
  case MISO_SELFTEST_EXP_N * 8 + 1: st_detmath_n<1, false>(x, n, stride, i, out, te, tl); break;
  case MISO_SELFTEST_EXP_N * 8 + 2: st_detmath_n<2, false>(x, n, stride, i, out, te, tl); break;
  case MISO_SELFTEST_EXP_N * 8 + 3: st_detmath_n<3, false>(x, n, stride, i, out, te, tl); break;
  case MISO_SELFTEST_EXP_N * 8 + 5: st_detmath_n<5, false>(x, n, stride, i, out, te, tl); break;
  case MISO_SELFTEST_LOG_N * 8 + 1: st_detmath_n<1, true>(x, n, stride, i, out, te, tl); break;
  case MISO_SELFTEST_LOG_N * 8 + 2: st_detmath_n<2, true>(x, n, stride, i, out, te, tl); break;
  case MISO_SELFTEST_LOG_N * 8 + 3: st_detmath_n<3, true>(x, n, stride, i, out, te, tl); break;
  case MISO_SELFTEST_LOG_N * 8 + 5: st_detmath_n<5, true>(x, n, stride, i, out, te, tl); break;
  case MISO_SELFTEST_EXP_T * 8 + 1: out[i] = det_exp_t(x[i], te); break;
  case MISO_SELFTEST_LOG_T * 8 + 1: out[i] = det_log_t(x[i], tl); break;
  case MISO_SELFTEST_SQRT_POS * 8 + 1: out[i] = det_sqrt_pos(x[i]); break;
  default: break;
  }
}

// det_exp_r / det_log_r as the two-isoform kernel's k2_exp / k2_log call them.  Element order = thread order; every thread of a
// wavefront with an element stays active through the call (the route is the wavefront's), the ones behind the last element
// with an argument both fast routes accept.
__global__ void __launch_bounds__(256) selftest_detmath_routed_kernel(int fn, int force_full, const double *x, int n, double *out, int32_t *route) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  double te[12], tl[12];
  det_tables_to_registers(te, tl);
  const bool on = i < n;
  const double v = on ? x[i] : 1.0;
  const DetRoute rt = det_route(force_full != 0);
  bool full = false;
  double y;
  if (fn == MISO_SELFTEST_LOG_R) y = det_log_r(v, tl, rt, full);
  else y = det_exp_r(v, te, rt, full);
  if (on) { out[i] = y; route[i] = full ? MISO_SELFTEST_ROUTE_FULL : MISO_SELFTEST_ROUTE_FAST; }
}

// Element order = thread order: elements 64 w .. 64 w + 63 share a wavefront, so the caller decides what a wavefront-uniform
// choice of route (__all / __any) sees.  Threads behind the last element carry an input that every fast route accepts.
__global__ void __launch_bounds__(256) selftest_threshold_kernel(int routine, const double *c_in, const double *T_in, int n, uint64_t *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool on = i < n;
  const double c = on ? c_in[i] : 0.5, T = on ? T_in[i] : 1.0;
  uint64_t t = 0;
  switch (routine) {
  case MISO_SELFTEST_K2_THRESHOLD: t = k2_threshold(c, T); break;
  case MISO_SELFTEST_K2_THRESHOLD_EXACT: t = k2_threshold_exact(c, T); break;
  case MISO_SELFTEST_FLAT_LT:
  case MISO_SELFTEST_FLAT_LE: {   // as sampler_flat's threshold pass forms the estimate and chooses the routine
    const bool le = routine == MISO_SELFTEST_FLAT_LE;
    const double inv = 4294967296.0 / T;
    const bool tnormal = T >= 1e-280 && T <= 1e280;
    const double est = c * inv;
    double r;
    if (__any(on && !(tnormal && est >= 2.0 && est <= 4294967293.0))) r = flat_threshold(le, c, T, est);
    else r = flat_threshold_fast(le, c, T, est);
    t = static_cast<uint64_t>(r);
    break;
  }
  case MISO_SELFTEST_FLAT_GENERAL_LT:
  case MISO_SELFTEST_FLAT_GENERAL_LE:
    t = static_cast<uint64_t>(flat_threshold(routine == MISO_SELFTEST_FLAT_GENERAL_LE, c, T, c * (4294967296.0 / T)));
    break;
  case MISO_SELFTEST_FLAT_FAST_LT:
  case MISO_SELFTEST_FLAT_FAST_LE:   // (the caller keeps to the routine's precondition)
    t = static_cast<uint64_t>(flat_threshold_fast(routine == MISO_SELFTEST_FLAT_FAST_LE, c, T, c * (4294967296.0 / T)));
    break;
  case MISO_SELFTEST_DRAW_LT: t = draw_threshold<false>(c, T, c * (4294967296.0 / T)); break;   // est as sampler_grp forms it
  case MISO_SELFTEST_DRAW_LE: t = draw_threshold<true>(c, T, c * (4294967296.0 / T)); break;
  default: break;
  }
  if (on) out[i] = t;
}

__global__ void __launch_bounds__(256) selftest_count_below_kernel(const int32_t *D0, const uint32_t *w4, const uint32_t *T, int n, int32_t *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int D = D0[i];
  const uint32_t *w = w4 + 4 * static_cast<size_t>(i);
  count_below(D, w[0], w[1], w[2], w[3], T[i]);
  out[i] = D;
}

// k2_flag.hpp: element i is one lane's read loop, its trips the pairs start[i] .. start[i + 1] - 1 of (m, k)
__global__ void __launch_bounds__(256) selftest_k2_flag_kernel(const uint32_t *m, const uint32_t *k, const int32_t *start, int n,
                                                               int32_t *code, uint32_t *pos) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  K2Flag f;
  for (int j = start[i]; j < start[i + 1]; j++) k2_flag_note(f, m[j], k[j]);
  uint32_t p = 0;
  code[i] = k2_flag_read(f, p);
  pos[i] = p;
}

// k2_count.hpp's assembly statements: element i is one lane, its words u[start[i]] .. u[start[i + 1] - 1] (an even number) taken
// two per statement as the read loop takes them, the first pair in the form that starts o; masked[i]: the tail's form with inv
__global__ void __launch_bounds__(256) selftest_k2_count_kernel(const uint32_t *th, const int32_t *start, const uint32_t *u,
                                                                const uint32_t *inv, const int32_t *masked, int n, uint32_t *acc_out,
                                                                uint32_t *o_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t P = k2_count_p(th[i]), two = K2_COUNT_TWO;
  uint32_t acc = 0, o = 0;
  const int j0 = start[i], j1 = start[i + 1];
  if (masked[i]) {
    if (j0 < j1) k2_count_pair_masked<true>(acc, o, P, two, u[j0], u[j0 + 1], inv[j0], inv[j0 + 1]);
    for (int j = j0 + 2; j < j1; j += 2) k2_count_pair_masked<false>(acc, o, P, two, u[j], u[j + 1], inv[j], inv[j + 1]);
  } else {
    if (j0 < j1) k2_count_pair<true>(acc, o, P, two, u[j0], u[j0 + 1]);
    for (int j = j0 + 2; j < j1; j += 2) k2_count_pair<false>(acc, o, P, two, u[j], u[j + 1]);
  }
  acc_out[i] = acc;
  o_out[i] = o;
}

// kernels_k2.inl k2_finish_lane, the code behind the single-end read loop, with a caller-given threshold t: element i is a
// chain on ONE lane (GE = 1) of n_draw[i] reads at iteration iter[i]; its sum and flag come from k2_count.hpp's plain functions
// over its blocks, in trips of two blocks and a single step as the loop takes them.  out[i] = the reads with uniform below t[i].
__global__ void __launch_bounds__(64) selftest_k2_finish_kernel(uint64_t seed, const uint32_t *event_id, const uint32_t *chain,
                                                                 const uint32_t *iter, const int32_t *n_draw, const uint64_t *t,
                                                                 int settle_all, int n, int32_t *out) {
  const int i0 = blockIdx.x * blockDim.x + threadIdx.x;
  const bool used = i0 < n;
  const int i = used ? i0 : n - 1;   // (every lane of the wavefront goes through the wave-wide vote)
  constexpr int UQ = 2;
  const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  const uint32_t ev = event_id[i], ch = chain[i], it = iter[i];
  const uint32_t th = static_cast<uint32_t>(t[i] >> 16), tl = static_cast<uint32_t>(t[i]) & 0xFFFFu;
  const int nfq = n_draw[i] >> 3, rem = n_draw[i] & 7, nblk = nfq + (rem != 0 ? 1 : 0), npos = nblk, uq_trips = npos / UQ;
  auto draw = [&](int q, bool low) {
    return miso_philox4x32(static_cast<uint32_t>(q), it, (low ? MISO_SITE_GIBBS_LOW : MISO_SITE_GIBBS) | (ch << 8), ev, k0, k1);
  };
  const uint32_t P = k2_count_p(th);
  int A = 0; K2Flag amb;
  for (int k = 0; k < npos;) {
    const int nb = k < UQ * uq_trips ? UQ : 1;
    uint32_t acc = 0, o = 0;
    for (int b = 0; b < nb; b++) {
      const miso_u32x4 u = draw(k + b, false);
      for (int w = 0; w < 4; w++) k2_count_step(acc, o, P, u.v[w], (k + b) < nfq ? 0u : k2_part_inv(rem, w));
    }
    A += k2_count_sum(acc);
    k2_flag_note_z(amb, k2_count_flag(o), static_cast<uint32_t>(k));
    k += nb;
  }
  const int d0 = k2_finish_lane<UQ>(A, amb, th, tl, 0, 1, nfq, rem, nblk, npos, uq_trips, used, settle_all != 0, draw);
  if (used) out[i] = d0;
}

__global__ void __launch_bounds__(256) selftest_text_digits_kernel(const double *x, int n, int64_t *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = text_digits(x[i]);
}

namespace {

// One read's draw as pe_dense makes it.  The lines between the record's bytes and pe_all_tests are RESTATED from pe_dense's
// body (cumulative weights from -0.0, rnd, the rule's adjustment, "not exact here"): lifting them into a helper both call
// would touch every paired-end sampler's code.  The table offsets are the isoform numbers, so fsel is the pick.
template <int KK>
__device__ __forceinline__ void st_pe_pick(const uint8_t *f, const double *psi, const double *fp_rep, int il2, uint32_t rule_le,
                                           uint32_t word, int32_t *out) {
  uint32_t pk[KK]; int64_t cb[KK];
  int over[KK - 1];
#pragma unroll
  for (int k = 0; k < KK - 1; k++) over[k] = 0;
  double T = -0.0;
#pragma unroll
  for (int k = 0; k < KK; k++) {
    pk[k] = static_cast<uint32_t>(k);
    T = T + psi[k] * fp_rep[f[k]];
    cb[k] = __double_as_longlong(T);
  }
  const double rnd = miso_u01(word) * T;
  const bool ok = rnd < T;
  int64_t rb = __double_as_longlong(rnd) - static_cast<int64_t>(rule_le & 1u);
  rb = ok ? rb : INT64_MIN;
  uint32_t fsel = pk[0];
  pe_all_tests<KK>(rb, cb, pk, fsel, over);
  out[0] = ok ? static_cast<int32_t>(fsel) : -1;
#pragma unroll
  for (int k = 0; k < KK - 1; k++) out[1 + k] = over[k];
  out[KK] = pe_pick_exact(f, KK, il2, psi, fp_rep, (rule_le & 1u) == 0, word);
}

}  // namespace

// f: n x KK fragment indices (il2 - 2 = incompatible, whose fp_rep entry is -0.0), psi: n x KK, fp_rep: il2 entries, rule:
// 1 = `!(rnd > c)`, 0 = `rnd < c` then unconditional; out: n x (KK + 1) = {dense pick or -1 where pe_dense would hand the read
// to pe_pick_exact, over[KK - 1], pe_pick_exact's pick}
__global__ void __launch_bounds__(256) selftest_pe_pick_kernel(int KK, const uint8_t *f, const double *psi, const double *fp_rep, int il2,
                                                               const uint32_t *rule_le, const uint32_t *word, int n, int32_t *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint8_t *fi = f + static_cast<size_t>(i) * KK;
  const double *pi = psi + static_cast<size_t>(i) * KK;
  int32_t *o = out + static_cast<size_t>(i) * (KK + 1);
  switch (KK) {
  case 2: st_pe_pick<2>(fi, pi, fp_rep, il2, rule_le[i], word[i], o); break;
  case 3: st_pe_pick<3>(fi, pi, fp_rep, il2, rule_le[i], word[i], o); break;
  case 4: st_pe_pick<4>(fi, pi, fp_rep, il2, rule_le[i], word[i], o); break;
  case 5: st_pe_pick<5>(fi, pi, fp_rep, il2, rule_le[i], word[i], o); break;
  case 6: st_pe_pick<6>(fi, pi, fp_rep, il2, rule_le[i], word[i], o); break;
  case 7: st_pe_pick<7>(fi, pi, fp_rep, il2, rule_le[i], word[i], o); break;
  case 8: st_pe_pick<8>(fi, pi, fp_rep, il2, rule_le[i], word[i], o); break;
  case 9: st_pe_pick<9>(fi, pi, fp_rep, il2, rule_le[i], word[i], o); break;
  case 10: st_pe_pick<10>(fi, pi, fp_rep, il2, rule_le[i], word[i], o); break;
  default: break;
  }
}

// draw i of chain 0 (iteration i) by the G lanes [G i, G i + G) of the grid: all lanes of a chain call binomial_coop together;
// the lanes behind the last draw repeat it and store nothing
template <int G>
__global__ void __launch_bounds__(256) selftest_binomial_kernel(uint64_t seed, uint32_t event_id, int32_t n, double p, int count,
                                                                const double *lf, int32_t *out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int sub = t % G, lane = threadIdx.x & 63;
  const int i = min(t / G, count - 1);
  const int32_t y = binomial_coop<G>(seed, event_id, 0u, static_cast<uint32_t>(i), n, p, lf, sub, lane - sub);
  if (t / G < count && sub == 0) out[i] = y;
}

// ---- the law of miso_binomial.h's draws by enumeration of the 32-bit words they are functions of (miso_selftest_binomial_law) ----
namespace {

// a stream whose `next` is 1 takes its next words from w1, w2, w3 without a Philox block: ONE trial of the header's own routines
// (a trial past the given words goes on with Philox words of stream (0, 0, 0, 0); its result is not used)
__device__ __forceinline__ void law_stream(miso_ustream *s, uint32_t U, uint32_t V) {
  miso_ustream_init(s, 0, 0, 0, 0, MISO_SITE_COUNTS);
  s->next = 1; s->w1 = U; s->w2 = V;
}
// trial 0 of miso_binomial_btrs on the words (U, V): its k, acc = trial 0 accepted
__device__ __forceinline__ int32_t law_btrs_trial(int32_t n, double r, const double *lf, uint32_t U, uint32_t V, bool &acc) {
  miso_ustream s;
  law_stream(&s, U, V);
  const int32_t k = miso_binomial_btrs(&s, n, r, lf);
  acc = s.next == 3;
  return k;
}
// miso_binomial_inversion on the word U: its x, or -1 where the search ran past its bound and took another word
__device__ __forceinline__ int32_t law_inversion_word(int32_t n, double r, uint32_t U, int32_t &x_any) {
  miso_ustream s;
  law_stream(&s, U, 0);
  x_any = miso_binomial_inversion(&s, n, r);
  return s.next == 2 ? x_any : -1;
}
// One word U of BTRS: count = #{V : trial 0 accepts (U, V)}, returns the trial's k, or -1 with count = 0 when k is outside
// 0 .. n (V = 0 passes every acceptance test, so it is refused only there).  The accepted V are taken to be [0, V*], V* by 32
// steps of bisection on the routine itself; check: the segment probed at V* - 2 .. V* + 3 (bad_near counts the words that
// disagree) and at 16 further V spread over either side (bad_far).
__device__ __forceinline__ int32_t law_btrs_word(int32_t n, double r, const double *lf, uint32_t U, bool check, uint64_t &count,
                                                 uint32_t &bad_near, uint32_t &bad_far) {
  bool acc;
  const int32_t k = law_btrs_trial(n, r, lf, U, 0u, acc);
  count = 0;
  if (!acc) return -1;
  uint64_t lo = 0, hi = 1ull << 32;
  for (int step = 0; step < 32; step++) {
    const uint64_t mid = (lo + hi) >> 1;
    law_btrs_trial(n, r, lf, U, static_cast<uint32_t>(mid), acc);
    if (acc) lo = mid; else hi = mid;
  }
  count = lo + 1;
  if (check) {
    for (int d = -2; d <= 3; d++) {
      const int64_t v = static_cast<int64_t>(lo) + d;
      if (v < 0 || v > 0xFFFFFFFFll) continue;
      law_btrs_trial(n, r, lf, U, static_cast<uint32_t>(v), acc);
      if (acc != (d <= 0)) bad_near++;
    }
    for (int j = 1; j <= 16; j++) {
      const uint64_t below = lo * static_cast<uint64_t>(j) / 17, above = lo + 1 + (0xFFFFFFFFull - lo) * static_cast<uint64_t>(j) / 16;
      law_btrs_trial(n, r, lf, U, static_cast<uint32_t>(below), acc);
      if (!acc) bad_far++;
      if (above <= 0xFFFFFFFFull) {
        law_btrs_trial(n, r, lf, U, static_cast<uint32_t>(above), acc);
        if (acc) bad_far++;
      }
    }
  }
  return k;
}

}  // namespace

// Thread t takes the enumerated words run t .. run t + run - 1 (word i is U = stride / 2 + i stride).  k(U) does not decrease, so a
// thread's bin changes rarely: counted in registers, added to hist (n + 1 entries) when k changes and at the end.  info:
// MISO_SELFTEST_LAW_* sums (regime and enumerated are the host's).  Bounded: the run, 32 bisection steps and 38 probes per
// word, the header's own trial caps.
__global__ void __launch_bounds__(256) selftest_binomial_law_kernel(int32_t n, double r, int btrs, uint32_t stride, uint64_t enumerated,
                                                                    uint32_t run, const double *lf, unsigned long long *hist,
                                                                    unsigned long long *info) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const uint64_t i0 = t * run;
  if (i0 >= enumerated) return;
  const uint64_t i1 = min(i0 + run, enumerated);
  auto word = [&](uint64_t i) { return static_cast<uint32_t>(stride / 2 + i * stride); };
  int32_t prev = -1, any;
  if (i0 > 0) {   // the k of the word before this run, for the order check
    bool acc;
    if (btrs) { prev = law_btrs_trial(n, r, lf, word(i0 - 1), 0u, acc); if (!acc) prev = -1; }
    else prev = law_inversion_word(n, r, word(i0 - 1), any);
  }
  int32_t bin = -1;
  uint64_t in_bin = 0, total = 0;
  uint32_t restarts = 0, out_of_range = 0, not_monotone = 0, checked = 0, bad_near = 0, bad_far = 0;
  auto flush = [&]() { if (bin >= 0 && bin <= n && in_bin != 0) atomicAdd(&hist[bin], static_cast<unsigned long long>(in_bin)); };
  for (uint64_t i = i0; i < i1; i++) {
    uint64_t count = 1;
    int32_t x;
    if (btrs) {
      const bool check = (i & 255) == 128;
      x = law_btrs_word(n, r, lf, word(i), check, count, bad_near, bad_far);
      if (check && x >= 0) checked++;
      if (x < 0) out_of_range++;
    } else {
      x = law_inversion_word(n, r, word(i), any);
      if (x < 0) {   // a Philox word's x: counted, and told in info
        restarts++; total++; count = 0;
        if (any >= 0 && any <= n) atomicAdd(&hist[any], 1ull);
      }
    }
    if (x >= 0) {
      if (x != bin) { flush(); bin = x; in_bin = 0; }
      in_bin += count;
    }
    total += count;
    if (prev >= 0 && x >= 0 && x < prev) not_monotone++;
    prev = x;
  }
  flush();
  if (total) atomicAdd(&info[MISO_SELFTEST_LAW_TOTAL], static_cast<unsigned long long>(total));
  if (restarts) atomicAdd(&info[MISO_SELFTEST_LAW_RESTARTS], static_cast<unsigned long long>(restarts));
  if (out_of_range) atomicAdd(&info[MISO_SELFTEST_LAW_OUT_OF_RANGE], static_cast<unsigned long long>(out_of_range));
  if (not_monotone) atomicAdd(&info[MISO_SELFTEST_LAW_NOT_MONOTONE], static_cast<unsigned long long>(not_monotone));
  if (checked) atomicAdd(&info[MISO_SELFTEST_LAW_SEGMENT_CHECKED], static_cast<unsigned long long>(checked));
  if (bad_near) atomicAdd(&info[MISO_SELFTEST_LAW_SEGMENT_BAD_NEAR], static_cast<unsigned long long>(bad_near));
  if (bad_far) atomicAdd(&info[MISO_SELFTEST_LAW_SEGMENT_BAD_FAR], static_cast<unsigned long long>(bad_far));
}

namespace {

// device copies of host arrays for one launch, freed on every way out
struct StBuffers {
  std::vector<void *> ptrs;
  ~StBuffers() { for (void *p : ptrs) (void) hipFree(p); }
  template <class T> T *in(const T *host, size_t count) {
    T *d = out<T>(count);
    if (count) HIP_OK(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
    return d;
  }
  template <class T> T *out(size_t count) {
    void *d = nullptr;
    HIP_OK(hipMalloc(&d, std::max<size_t>(count, 1) * sizeof(T)));
    ptrs.push_back(d);
    return static_cast<T *>(d);
  }
  template <class T> void back(T *host, const T *dev, size_t count) {
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    if (count) HIP_OK(hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost));
  }
};

void st_need_device(int n) {
  if (n < 0) MISO_FAIL(MISO_EINVAL, "negative element count");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device");
}
dim3 st_grid(size_t threads) { return dim3(static_cast<unsigned>((threads + 255) / 256)); }

}  // namespace

void selftest_detmath_n(int fn, int width, const double *x, int n, int stride, double *out) {
  const bool wide = fn == MISO_SELFTEST_EXP_N || fn == MISO_SELFTEST_LOG_N;
  if (wide ? !(width == 1 || width == 2 || width == 3 || width == 5)
           : !((fn == MISO_SELFTEST_EXP_T || fn == MISO_SELFTEST_LOG_T || fn == MISO_SELFTEST_SQRT_POS) && width == 1))
    MISO_FAIL(MISO_EINVAL, "no such detmath_n routine / width");
  if (stride < 0) MISO_FAIL(MISO_EINVAL, "negative stride");
  st_need_device(n);
  if (n == 0) return;
  StBuffers b;
  const double *dx = b.in(x, static_cast<size_t>(n));
  double *dout = b.out<double>(static_cast<size_t>(n) * width);
  hipLaunchKernelGGL(selftest_detmath_n_kernel, st_grid(n), dim3(256), 0, 0, fn, width, dx, n, stride, dout);
  b.back(out, dout, static_cast<size_t>(n) * width);
}

void selftest_detmath_routed(int fn, int force_full, const double *x, int n, double *out, int32_t *route) {
  if (fn != MISO_SELFTEST_EXP_R && fn != MISO_SELFTEST_LOG_R) MISO_FAIL(MISO_EINVAL, "no such routed detmath routine");
  st_need_device(n);
  if (n == 0) return;
  StBuffers b;
  const double *dx = b.in(x, static_cast<size_t>(n));
  double *dout = b.out<double>(static_cast<size_t>(n));
  int32_t *droute = b.out<int32_t>(static_cast<size_t>(n));
  hipLaunchKernelGGL(selftest_detmath_routed_kernel, st_grid(n), dim3(256), 0, 0, fn, force_full, dx, n, dout, droute);
  b.back(out, dout, static_cast<size_t>(n));
  b.back(route, droute, static_cast<size_t>(n));
}

void selftest_threshold(int routine, const double *c, const double *T, int n, uint64_t *out) {
  if (routine < 0 || routine > MISO_SELFTEST_DRAW_LE) MISO_FAIL(MISO_EINVAL, "no such threshold routine");
  st_need_device(n);
  if (n == 0) return;
  StBuffers b;
  const double *dc = b.in(c, static_cast<size_t>(n)), *dT = b.in(T, static_cast<size_t>(n));
  uint64_t *dout = b.out<uint64_t>(static_cast<size_t>(n));
  hipLaunchKernelGGL(selftest_threshold_kernel, st_grid(n), dim3(256), 0, 0, routine, dc, dT, n, dout);
  b.back(out, dout, static_cast<size_t>(n));
}

void selftest_count_below(const int32_t *D, const uint32_t *w4, const uint32_t *T, int n, int32_t *out) {
  st_need_device(n);
  if (n == 0) return;
  StBuffers b;
  const int32_t *dD = b.in(D, static_cast<size_t>(n));
  const uint32_t *dw = b.in(w4, 4 * static_cast<size_t>(n)), *dT = b.in(T, static_cast<size_t>(n));
  int32_t *dout = b.out<int32_t>(static_cast<size_t>(n));
  hipLaunchKernelGGL(selftest_count_below_kernel, st_grid(n), dim3(256), 0, 0, dD, dw, dT, n, dout);
  b.back(out, dout, static_cast<size_t>(n));
}

void selftest_pe_pick(int KK, const uint8_t *f, const double *psi, const double *fp_rep, int il2, const uint32_t *rule_le,
                      const uint32_t *word, int n, int32_t *out) {
  if (KK < 2 || KK > 10) MISO_FAIL(MISO_EINVAL, "isoforms: 2 .. 10");
  if (il2 < 3 || il2 > 256) MISO_FAIL(MISO_EINVAL, "fragment table: 3 .. 256 entries");
  st_need_device(n);
  const size_t nk = static_cast<size_t>(n) * KK;
  for (size_t i = 0; i < nk; i++) if (f[i] >= il2) MISO_FAIL(MISO_EINVAL, "fragment index outside the table");
  if (n == 0) return;
  StBuffers b;
  const uint8_t *df = b.in(f, nk);
  const double *dpsi = b.in(psi, nk), *dfp = b.in(fp_rep, static_cast<size_t>(il2));
  const uint32_t *drule = b.in(rule_le, static_cast<size_t>(n)), *dword = b.in(word, static_cast<size_t>(n));
  int32_t *dout = b.out<int32_t>(static_cast<size_t>(n) * (KK + 1));
  hipLaunchKernelGGL(selftest_pe_pick_kernel, st_grid(n), dim3(256), 0, 0, KK, df, dpsi, dfp, il2, drule, dword, n, dout);
  b.back(out, dout, static_cast<size_t>(n) * (KK + 1));
}

void selftest_k2_flag(const uint32_t *m, const uint32_t *k, const int32_t *start, int n, int32_t *code, uint32_t *pos) {
  st_need_device(n);
  if (n == 0) return;
  if (start[0] != 0) MISO_FAIL(MISO_EINVAL, "start[0] must be 0");
  for (int i = 0; i < n; i++) if (start[i + 1] < start[i]) MISO_FAIL(MISO_EINVAL, "start must not decrease");
  const size_t total = static_cast<size_t>(start[n]);
  StBuffers b;
  const uint32_t *dm = b.in(m, total), *dk = b.in(k, total);
  const int32_t *dstart = b.in(start, static_cast<size_t>(n) + 1);
  int32_t *dcode = b.out<int32_t>(static_cast<size_t>(n));
  uint32_t *dpos = b.out<uint32_t>(static_cast<size_t>(n));
  hipLaunchKernelGGL(selftest_k2_flag_kernel, st_grid(n), dim3(256), 0, 0, dm, dk, dstart, n, dcode, dpos);
  b.back(code, dcode, static_cast<size_t>(n));
  b.back(pos, dpos, static_cast<size_t>(n));
}

void selftest_k2_count(const uint32_t *th, const int32_t *start, const uint32_t *u, const uint32_t *inv, const int32_t *masked, int n,
                       uint32_t *acc, uint32_t *o) {
  st_need_device(n);
  if (n == 0) return;
  if (start[0] != 0) MISO_FAIL(MISO_EINVAL, "start[0] must be 0");
  for (int i = 0; i < n; i++) {
    if (start[i + 1] < start[i] || ((start[i + 1] - start[i]) & 1)) MISO_FAIL(MISO_EINVAL, "start must not decrease; two words per statement");
    if (th[i] > 65536u) MISO_FAIL(MISO_EINVAL, "th: 0 .. 65536");
    if (!masked[i]) for (int j = start[i]; j < start[i + 1]; j++) if (inv[j] != 0) MISO_FAIL(MISO_EINVAL, "the steady form has no masks");
  }
  const size_t total = static_cast<size_t>(start[n]);
  StBuffers b;
  const uint32_t *dth = b.in(th, static_cast<size_t>(n)), *du = b.in(u, total), *dinv = b.in(inv, total);
  const int32_t *dstart = b.in(start, static_cast<size_t>(n) + 1), *dmasked = b.in(masked, static_cast<size_t>(n));
  uint32_t *dacc = b.out<uint32_t>(static_cast<size_t>(n)), *do_ = b.out<uint32_t>(static_cast<size_t>(n));
  hipLaunchKernelGGL(selftest_k2_count_kernel, st_grid(n), dim3(256), 0, 0, dth, dstart, du, dinv, dmasked, n, dacc, do_);
  b.back(acc, dacc, static_cast<size_t>(n));
  b.back(o, do_, static_cast<size_t>(n));
}

void selftest_k2_finish(uint64_t seed, const uint32_t *event_id, const uint32_t *chain, const uint32_t *iter, const int32_t *n_draw,
                        const uint64_t *t, int settle_all, int n, int32_t *out) {
  st_need_device(n);
  if (n == 0) return;
  for (int i = 0; i < n; i++) {
    if (n_draw[i] < 0 || n_draw[i] > (1 << 20)) MISO_FAIL(MISO_EINVAL, "n_draw: 0 .. 2^20");
    if (t[i] > 4294967296ull) MISO_FAIL(MISO_EINVAL, "t: 0 .. 2^32");
    if (chain[i] >= (1u << 24)) MISO_FAIL(MISO_EINVAL, "chain: below 2^24");
  }
  StBuffers b;
  const uint32_t *dev = b.in(event_id, static_cast<size_t>(n)), *dch = b.in(chain, static_cast<size_t>(n)), *dit = b.in(iter, static_cast<size_t>(n));
  const int32_t *dn = b.in(n_draw, static_cast<size_t>(n));
  const uint64_t *dt = b.in(t, static_cast<size_t>(n));
  int32_t *dout = b.out<int32_t>(static_cast<size_t>(n));
  hipLaunchKernelGGL(selftest_k2_finish_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, seed, dev, dch, dit, dn, dt, settle_all, n, dout);
  b.back(out, dout, static_cast<size_t>(n));
}

void selftest_text_digits(const double *x, int n, int64_t *out) {
  st_need_device(n);
  if (n == 0) return;
  StBuffers b;
  const double *dx = b.in(x, static_cast<size_t>(n));
  int64_t *dout = b.out<int64_t>(static_cast<size_t>(n));
  hipLaunchKernelGGL(selftest_text_digits_kernel, st_grid(n), dim3(256), 0, 0, dx, n, dout);
  b.back(out, dout, static_cast<size_t>(n));
}

void selftest_binomial(int G, uint64_t seed, uint32_t event_id, int32_t n, double p, int count, int32_t *out) {
  if (!(G == 1 || G == 2 || G == 4 || G == 8)) MISO_FAIL(MISO_EINVAL, "lanes per chain: 1, 2, 4, 8");
  if (n < 0 || n > (1 << 24)) MISO_FAIL(MISO_EINVAL, "n: 0 .. 2^24");
  st_need_device(count);
  if (count == 0) return;
  std::vector<double> lf(static_cast<size_t>(n) + 2);
  miso_logfact_fill(lf.data(), static_cast<int32_t>(lf.size()));   // as miso_batch::upload builds the batch's table
  StBuffers b;
  const double *dlf = b.in(lf.data(), lf.size());
  int32_t *dout = b.out<int32_t>(static_cast<size_t>(count));
  const dim3 grid = st_grid(static_cast<size_t>(count) * G);
  switch (G) {
  case 1: hipLaunchKernelGGL(selftest_binomial_kernel<1>, grid, dim3(256), 0, 0, seed, event_id, n, p, count, dlf, dout); break;
  case 2: hipLaunchKernelGGL(selftest_binomial_kernel<2>, grid, dim3(256), 0, 0, seed, event_id, n, p, count, dlf, dout); break;
  case 4: hipLaunchKernelGGL(selftest_binomial_kernel<4>, grid, dim3(256), 0, 0, seed, event_id, n, p, count, dlf, dout); break;
  default: hipLaunchKernelGGL(selftest_binomial_kernel<8>, grid, dim3(256), 0, 0, seed, event_id, n, p, count, dlf, dout); break;
  }
  b.back(out, dout, static_cast<size_t>(count));
}

void selftest_binomial_law(int32_t n, double p, uint32_t stride, uint64_t *hist, uint64_t *info, float *kernel_ms) {
  if (n < 1 || n > (1 << 24)) MISO_FAIL(MISO_EINVAL, "n: 1 .. 2^24");
  if (!(p > 0.0) || p >= 1.0) MISO_FAIL(MISO_EINVAL, "p: inside (0, 1)");
  if (stride == 0 || (stride & (stride - 1)) != 0) MISO_FAIL(MISO_EINVAL, "stride: a power of two");
  st_need_device(0);
  const double r = p > 0.5 ? 1.0 - p : p;                     // as miso_binomial reduces p and chooses the routine
  const bool btrs = !(static_cast<double>(n) * r < 10.0);
  const uint64_t enumerated = (1ull << 32) / stride;
  // a run per thread: 2^18 threads where the words allow it, at most 4096 words each
  const uint32_t run = static_cast<uint32_t>(std::min<uint64_t>(4096, std::max<uint64_t>(1, enumerated >> 18)));
  const uint64_t threads = (enumerated + run - 1) / run;
  std::vector<double> lf(static_cast<size_t>(n) + 2);
  miso_logfact_fill(lf.data(), static_cast<int32_t>(lf.size()));   // as miso_batch::upload builds the batch's table
  std::vector<uint64_t> zero(static_cast<size_t>(n) + 1, 0), info0(MISO_SELFTEST_LAW_INFO_N, 0);
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit atomics");
  HipCall c(nullptr);
  const double *dlf = c.upload(lf.data(), lf.size() * sizeof(double));
  unsigned long long *dhist = c.upload(reinterpret_cast<const unsigned long long *>(zero.data()), zero.size() * sizeof(uint64_t));
  unsigned long long *dinfo = c.upload(reinterpret_cast<const unsigned long long *>(info0.data()), info0.size() * sizeof(uint64_t));
  c.start();
  hipLaunchKernelGGL(selftest_binomial_law_kernel, st_grid(threads), dim3(256), 0, c.st, n, r, btrs ? 1 : 0, stride, enumerated, run, dlf,
                     dhist, dinfo);
  c.stop();
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(hist, dhist, zero.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, c.st));
  HIP_OK(hipMemcpyAsync(info, dinfo, info0.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, c.st));
  HIP_OK(hipStreamSynchronize(c.st));
  info[MISO_SELFTEST_LAW_REGIME] = btrs ? MISO_SELFTEST_LAW_BTRS : MISO_SELFTEST_LAW_INVERSION;
  info[MISO_SELFTEST_LAW_ENUMERATED] = enumerated;
  if (kernel_ms) *kernel_ms = c.elapsed_ms();
}

}  // namespace miso
