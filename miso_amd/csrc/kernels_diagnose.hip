// kernels_diagnose.hip -- chain diagnostics on the device: split R-hat, effective sample size and Monte-Carlo standard
// error of every (event, isoform) column of the resident samples.  No reference counterpart: the
// reference compares its chains only in stop = CONVERGENT_MEAN (host.cpp convergent_mean), a stopping rule restated
// with its defects, not a diagnostic.
//
// The split-sequence layout, the order of every operation and the moments-and-Geyer stage itself are in diagnose_column.hpp,
// which the rank-normalised pass (kernels_diagnose_rank.hip) includes too.  CACHED here: N <= 256 * SUMMARY_CACHE = 8192.
#include <hip/hip_runtime.h>

#include "device.hpp"
#include "diagnose_column.hpp"

namespace miso {

// scratch (dynamic LDS): [cached ? N : 0] centred values, then m[M], a0[M], a1[M]
template <bool CACHED>
__device__ __forceinline__ void diagnose_column(const double *x, const DiagShape sh, double log10N, double *o,
                                                double *lds) {
  const int N = 2 * sh.C * sh.h;
  if (CACHED) {
    diag_load(x, sh, lds);
    __syncthreads();
  }
  diag_moments<CACHED>(x, sh, log10N, o, lds, lds + (CACHED ? N : 0));
}

// Grid (events, kmax), one workgroup per column; out: four doubles {rhat, ess, mcse, lag} per (event, isoform) at
// diag_off[ev] + 4 k.  cached: the host's choice (N <= 256 * SUMMARY_CACHE), which also sized the dynamic LDS.
__global__ __launch_bounds__(256) void diagnose_kernel(const DevEvent *events, const unsigned char *out_pool, int n_events,
                                                       int C, int n, int h, double log10N, int cached,
                                                       const uint64_t *diag_off, double *out) {
  extern __shared__ double diag_lds[];
  const int ev = blockIdx.x, k = blockIdx.y;
  if (ev >= n_events) return;
  const DevEvent E = events[ev];
  if (k >= E.K) return;
  const double *x = reinterpret_cast<const double *>(out_pool + E.off_samples) + k;
  double *o = out + diag_off[ev] + 4 * k;
  const DiagShape sh{C, n, h, E.K};
  if (cached) diagnose_column<true>(x, sh, log10N, o, diag_lds);
  else diagnose_column<false>(x, sh, log10N, o, diag_lds);
}

}  // namespace miso
