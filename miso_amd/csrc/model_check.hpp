// model_check.hpp -- the posterior predictive model check of single-end events: what its kernel takes, the
// kernel's body, and the host driver's interface.  The arithmetic of one row is include/miso_model_check.h's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "miso_amd.h"
#include "miso_model_check.h"

namespace miso {

constexpr int MC_BLOCK = 256;

// Every pointer on the device.  Per event: K isoforms, C classes at class_off[ev] of pattern / m / n, N = sum n, S sample rows
// of K doubles at samples + sample_off[ev], the Philox event id, and the host's verdict (MISO_FIT_OK: the kernel works on it).
struct ModelCheckArgs {
  const int32_t *K, *C, *N, *S, *status;
  const int64_t *class_off;
  const uint64_t *pattern;
  const double *m;
  const int32_t *n;
  const uint64_t *sample_off;
  const uint32_t *event_id;
  const double *samples;
  const double *lf;        // log factorials, (largest N) + 1 entries
  uint64_t seed;
  // results: per event {rows, bad_rows, exceed} and {sum D_obs, sum D_rep}; per class sum_s p_c's mean times N, and the tails
  int32_t *ev_int;
  double *ev_dbl;
  double *expected;
  int32_t *ge, *le;
};

// a predicate's count over the wavefront, added once per wavefront (block = MC_BLOCK threads in one dimension: lane = t & 63)
__device__ __forceinline__ void mc_wave_count(bool pred, int32_t *lds_counter) {
  const unsigned long long b = __ballot(pred);
  if ((threadIdx.x & 63u) == 0 && b) atomicAdd(lds_counter, static_cast<int32_t>(__popcll(b)));
}

// One workgroup, one event.  acc: dynamic LDS, C x MC_BLOCK doubles -- thread t's running sum of p_c at acc[c * MC_BLOCK + t].
// Order of the double sums (two runs give the same bits): every thread adds its own rows t, t + 256, ... in ascending order;
// then the 256 partial sums are folded in halves, x[t] += x[t + h] for h = 128, 64, ..., 1.
__device__ __forceinline__ void model_check_event(const ModelCheckArgs &a, int ev, double *acc) {
  __shared__ uint64_t s_pat[MISO_FIT_MAX_CLASSES];
  __shared__ double s_m[MISO_FIT_MAX_CLASSES], s_rootn[MISO_FIT_MAX_CLASSES];
  __shared__ int32_t s_n[MISO_FIT_MAX_CLASSES], s_ge[MISO_FIT_MAX_CLASSES], s_le[MISO_FIT_MAX_CLASSES];
  __shared__ int32_t s_cnt[3];                 // rows, bad rows, exceed
  __shared__ double s_red[2][MC_BLOCK];        // D_obs, D_rep
  const int t = static_cast<int>(threadIdx.x);
  const int K = a.K[ev], C = a.C[ev], N = a.N[ev], S = a.S[ev];
  const int64_t co = a.class_off[ev];
  if (t < C) {
    s_pat[t] = a.pattern[co + t];
    s_m[t] = a.m[co + t];
    s_n[t] = a.n[co + t];
    s_rootn[t] = miso_det_sqrt(static_cast<double>(a.n[co + t]));
    s_ge[t] = 0;
    s_le[t] = 0;
  }
  if (t < 3) s_cnt[t] = 0;
  for (int c = 0; c < C; c++) acc[c * MC_BLOCK + t] = 0.0;
  __syncthreads();

  const double *x = a.samples + a.sample_off[ev];
  const uint64_t seed = a.seed;
  const uint32_t event_id = a.event_id[ev];
  const double dN = static_cast<double>(N);
  double sum_obs = 0.0, sum_rep = 0.0;
  for (int base = 0; base < S; base += MC_BLOCK) {
    const int s = base + t;
    const bool has = s < S;
    const double *psi = x + static_cast<size_t>(has ? s : 0) * static_cast<size_t>(K);
    const double T0 = miso_fit_suffix(s_pat, s_m, C, 0, psi);
    const bool live = has && miso_fit_row_ok(T0);
    mc_wave_count(live, &s_cnt[0]);
    mc_wave_count(has && !live, &s_cnt[1]);
    miso_ustream st;
    miso_ustream_init(&st, seed, event_id, 0u, static_cast<uint32_t>(s), MISO_SITE_FIT);
    int32_t rem = live ? N : 0;                // (no reads left: miso_binomial returns at once, no word is drawn)
    double d_obs = 0.0, d_rep = 0.0;
    for (int c = 0; c < C; c++) {              // uniform: only the inside of miso_binomial diverges
      const double w = miso_fit_weight(s_pat[c], s_m[c], psi);
      const double p = w / T0;
      const double root_e = miso_det_sqrt(dN * p);
      int32_t rep = rem;
      if (c < C - 1) {
        const double Tc = c == 0 ? T0 : miso_fit_suffix(s_pat, s_m, C, c, psi);
        rep = miso_binomial(&st, rem, w / Tc, a.lf);
        rem -= rep;
      }
      d_obs = d_obs + miso_fit_term(s_rootn[c], root_e);
      d_rep = d_rep + miso_fit_term(miso_det_sqrt(static_cast<double>(rep)), root_e);
      if (live) acc[c * MC_BLOCK + t] = acc[c * MC_BLOCK + t] + p;
      mc_wave_count(live && rep >= s_n[c], &s_ge[c]);
      mc_wave_count(live && rep <= s_n[c], &s_le[c]);
    }
    if (live) {
      sum_obs = sum_obs + d_obs;
      sum_rep = sum_rep + d_rep;
    }
    mc_wave_count(live && d_rep >= d_obs, &s_cnt[2]);
  }

  s_red[0][t] = sum_obs;
  s_red[1][t] = sum_rep;
  for (int h = MC_BLOCK / 2; h > 0; h >>= 1) {
    __syncthreads();
    if (t < h) {
      s_red[0][t] = s_red[0][t] + s_red[0][t + h];
      s_red[1][t] = s_red[1][t] + s_red[1][t + h];
      for (int c = 0; c < C; c++) acc[c * MC_BLOCK + t] = acc[c * MC_BLOCK + t] + acc[c * MC_BLOCK + t + h];
    }
  }
  __syncthreads();
  const int rows = s_cnt[0];
  if (t < C) {
    a.expected[co + t] = rows > 0 ? (dN * acc[t * MC_BLOCK]) / static_cast<double>(rows) : 0.0;
    a.ge[co + t] = s_ge[t];
    a.le[co + t] = s_le[t];
  }
  if (t == 0) {
    a.ev_int[3 * ev] = rows;
    a.ev_int[3 * ev + 1] = s_cnt[1];
    a.ev_int[3 * ev + 2] = s_cnt[2];
    a.ev_dbl[2 * ev] = s_red[0][0];
    a.ev_dbl[2 * ev + 1] = s_red[1][0];
  }
}

// ---- the host driver (kernels_model_check.hip) ----
// The call's tables on the host; the samples on the host (h_samples, uploaded) or already on the device (d_samples, a batch's
// pool).  n_sample_doubles: the extent every event's rows must lie inside.
struct ModelCheckInput {
  int n = 0;
  const int32_t *K = nullptr, *C = nullptr;
  const int64_t *class_off = nullptr;      // n + 1 entries
  const uint64_t *pattern = nullptr;
  const int64_t *m = nullptr;
  const int32_t *counts = nullptr;
  const uint64_t *sample_off = nullptr;
  const int32_t *S = nullptr;
  const uint32_t *event_id = nullptr;
  const int32_t *status_in = nullptr;      // may be null; an entry other than MISO_FIT_OK is kept and the event left out
  const double *h_samples = nullptr, *d_samples = nullptr;
  uint64_t n_sample_doubles = 0;
  uint64_t seed = 0;
};
// per event / per class (class_off's layout); everything but status is zero where status != MISO_FIT_OK
struct ModelCheckOutput {
  int32_t *status, *rows, *bad_rows, *exceed;
  double *sum_obs, *sum_rep;
  double *expected;
  int32_t *ge, *le;
};
// runs the kernel on the current device, on `st` (null: a stream of the call's own); returns the kernel time
float model_check_run(const ModelCheckInput &in, const ModelCheckOutput &out, hipStream_t st);

}  // namespace miso
