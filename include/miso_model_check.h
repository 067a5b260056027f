/*
 * miso_model_check.h -- the arithmetic contract of the posterior predictive model check of single-end events
 * (csrc/kernels_model_check.hip runs it, tests/_model_check_ref.py restates it).
 *
 * The model behind every psi (miso.c:124-182): a read of isoform k starts at one of its e_k positions with equal
 * probability.  The gene's read classes -- the sets of isoforms that share an alignment -- have m_c start positions each
 * (csrc/host.cpp assignment_matrix), so under the model a read falls into class c with probability
 *
 *     p_c = w_c / T_0,    w_c = m_c * sum_{k in pattern_c} psi_k  (k ascending, from 0.0),
 *     T_c = w_c + T_{c+1},  T_{C-1} = w_{C-1}   (suffix sums, accumulated from the last class down).
 *
 * The likelihood never sees m_c (constant in psi), so the class counts n_c test what the fit did not use.  Discrepancy
 * (Freeman-Tukey): D(n, p) = sum_c (sqrt(n_c) - sqrt(N p_c))^2, c ascending, miso_det_sqrt, no contraction.
 *
 * The replicate of posterior row s: Multinomial(N, p) as a chain of binomials on ONE word stream,
 *     miso_ustream_init(seed, event_id, chain 0, iteration s, MISO_SITE_FIT),
 *     c = 0 .. C-2:  n_c = miso_binomial(stream, rem, w_c / T_c, lf),  rem -= n_c;   the last class takes rem
 * (a ratio 0/0 is not a number and draws 0 by miso_binomial's own rule).  Site 6 is this pass's alone: no draw of
 * miso_philox.h's list moves, the counter-mode contract's version stays.
 */
#ifndef MISO_MODEL_CHECK_H
#define MISO_MODEL_CHECK_H

#include "miso_binomial.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#define MISO_SITE_FIT 6u
#define MISO_FIT_MAX_CLASSES 64   /* csrc/host.cpp gene_classes: patterns are 64-bit sets, at most 64 columns */

/* w_c of one row: psi = the row's K values */
MISO_HD double miso_fit_weight(uint64_t pattern, double m, const double *psi) {
  double sum = 0.0;
  while (pattern) {
    const int k = __builtin_ctzll(pattern);
    sum = sum + psi[k];
    pattern &= pattern - 1;
  }
  return m * sum;
}

/* T_c of one row, accumulated from the last class down.  Recomputed where it is needed rather than kept: a thread of the
   kernel holds no per-class state, and the classes of an event are few (three for two isoforms). */
MISO_HD double miso_fit_suffix(const uint64_t *pattern, const double *m, int C, int c, const double *psi) {
  double T = miso_fit_weight(pattern[C - 1], m[C - 1], psi);
  int j;
  for (j = C - 2; j >= c; j--) T = miso_fit_weight(pattern[j], m[j], psi) + T;
  return T;
}

/* a row takes part: T_0 positive and finite */
MISO_HD int miso_fit_row_ok(double T0) { return T0 > 0.0 && T0 < __builtin_inf(); }

/* one class's term of D: root_n = miso_det_sqrt(count), root_e = miso_det_sqrt(N p_c) */
MISO_HD double miso_fit_term(double root_n, double root_e) {
  const double d = root_n - root_e;
  return d * d;
}

#endif /* MISO_MODEL_CHECK_H */
