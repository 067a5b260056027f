// kernels_compare_pairs_groups.hip -- the posterior of delta psi = psi_1 - psi_2 between two GROUPS of replicate samples
// (miso_batch_compare_pairs_groups, include/miso_amd.h): kernel and host driver.
//
// Per (event, isoform): A = the multiset union of the n1 group-1 samples' columns (N1 = n1 S draws), B the same of group 2
// (N2 = n2 S), D the multiset of the M = N1 N2 IEEE doubles fl(a - b).  Everything else is DESIGN.md 19's definition over
// this D: three order statistics at the host's ranks and the exact counts #{d > 0}, #{d < 0}, #{d >= tau} + #{d <= -tau}.
// The counts are the sums of the n1 n2 pairwise passes' counts; the order statistics are no function of the pairwise ones,
// which is why the pooled law has a pass of its own.
//
// One 256-thread workgroup per (event, isoform), as compare_pairs_kernel, and its routines (compare_pairs_device.hpp): a
// group of one against a group of one gives that kernel's bits.  Two pooled groups do not fit the LDS together (2 x 16384
// draws are 256 KB of 160), so only one stays there:
//   group 1 is gathered from its samples' pools into LDS as order_keys, sorted, and written as doubles to this
//   workgroup's row of a global workspace; group 2 is gathered into the same LDS, sorted, and stays as doubles.
// A count reads a[t], a[t + 256], ... from the row (coalesced; the row is this workgroup's own, written before a barrier)
// and searches b in LDS.  Dynamic LDS: max(N1, N2) * 8 bytes, 128 KB at the limit.
// Plain C++, f64 subtraction and comparison only, no atomics; every barrier in workgroup-uniform control flow.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "batch.hpp"
#include "column_pass.hpp"
#include "compare_pairs.hpp"
#include "compare_pairs_device.hpp"
#include "order_key.hpp"
#include "text_digits.hpp"

namespace miso {

// n columns of S draws each (sample c's at pools[c] + evs[c][ev].off_samples, isoform kk of K) into keys[0 .. n S) as
// order_keys; returns whether this thread met a NaN or an infinity.
// as_text: a draw as its `.miso` file prints it and a reader parses it back (text_digits.hpp).
// (x + 0.0: -0.0 becomes +0.0; the differences compare the same)
__device__ __forceinline__ int pairs_gather(const DevEvent *const *evs, const unsigned char *const *pools, int n, int ev, int kk,
                                            int K, int S, int as_text, uint64_t *keys) {
  const double inf = __longlong_as_double(0x7FF0000000000000ll);
  int bad = 0;
  for (int c = 0; c < n; c++) {
    // (a pointer that was itself loaded from memory is a flat one to the compiler: said to be global, as compare_column.hpp)
    using GlobalColumn = const __attribute__((address_space(1))) double *;
    const GlobalColumn x = (GlobalColumn) reinterpret_cast<uint64_t>(pools[c] + evs[c][ev].off_samples) + kk;
    uint64_t *dst = keys + static_cast<size_t>(c) * S;
    for (int e = threadIdx.x; e < S; e += 256) {
      double v = x[static_cast<size_t>(e) * K];
      if (as_text && text_rounds(v)) v = static_cast<double>(text_digits(v)) / 10000.0;
      bad |= !(fabs(v) < inf);
      dst[e] = order_key(v + 0.0);
    }
  }
  return bad;
}

// Grid (events of this launch, kmax).  evs / pools: the n1 + n2 batches' event tables and sample pools, group 1 first.
// The launch covers events [ev0, ev0 + n_events); out and col_off as compare_pairs_kernel's (col_off[ev] with
// PAIRS_SKIP_EVENT set: some batch never decoded the event, nothing of it is read); work: kmax rows of n1 * S doubles
// per event of the launch.  The host refuses n1 * S, n2 * S outside [1, PAIRS_GROUP_MAX_DRAWS] and sizes the dynamic LDS.
__global__ __launch_bounds__(256) void compare_pairs_groups_kernel(const DevEvent *const *__restrict__ evs,
                                                                   const unsigned char *const *__restrict__ pools, int n1,
                                                                   int n2, int S, int ev0, int n_events, int kmax,
                                                                   PairsArgs pa, int as_text, const uint64_t *col_off,
                                                                   uint64_t *out, double *work) {
  extern __shared__ uint64_t pairs_lds[];
  __shared__ PairsScratch sc;
  const int kk = blockIdx.y, t = threadIdx.x;
  if (static_cast<int>(blockIdx.x) >= n_events) return;
  const int ev = ev0 + static_cast<int>(blockIdx.x);
  const int K = evs[0][ev].K;
  if (kk >= K) return;
  const int N1 = n1 * S, N2 = n2 * S;
  const int W = PAIRS_FIXED_WORDS + pa.n_tau;
  const uint64_t first_col = col_off[ev];
  uint64_t *o = out + ((first_col & ~PAIRS_SKIP_EVENT) + kk) * W;
  double *A = work + (static_cast<size_t>(blockIdx.x) * kmax + kk) * N1;

  // (workgroup-uniform: a skipped event is every thread's; the gathers' flags go through __syncthreads_or)
  bool bad = (first_col & PAIRS_SKIP_EVENT) != 0;
  if (!bad) bad = __syncthreads_or(pairs_gather(evs, pools, n1, ev, kk, K, S, as_text, pairs_lds)) != 0;
  if (!bad) {
    pairs_sort(pairs_lds, N1);
    for (int e = t; e < N1; e += 256) A[e] = key_value(pairs_lds[e]);
    __syncthreads();                                  // every thread is done with group 1's keys; the row is written
    bad = __syncthreads_or(pairs_gather(evs + n1, pools + n1, n2, ev, kk, K, S, as_text, pairs_lds)) != 0;
  }
  if (bad) {
    if (t == 0) pairs_not_finite(o, pa.n_tau);
    return;
  }
  pairs_sort(pairs_lds, N2);
  double *B = reinterpret_cast<double *>(pairs_lds);
  for (int e = t; e < N2; e += 256) B[e] = key_value(pairs_lds[e]);   // (each thread its own words, in place)
  __syncthreads();

  pairs_statistics(A, N1, B, N2, pa, o, sc);
}

// The workspace of one launch, bytes at most: a launch covers as many events as fit (one at least), so what a call holds
// on the device does not grow with its events.  At the limit (16384 draws, 128 KB a row) 256 MiB are 2048 workgroups
// a launch -- eight for each of an MI355X's 256 CUs, of which the LDS lets one be resident: launches stay long enough
// that their tails do not count.
constexpr size_t PAIRS_GROUP_WORK_BYTES = size_t{256} << 20;

void compare_pairs_groups(miso_batch *const *g1, int n1, miso_batch *const *g2, int n2, double confidence_level, const double *tau,
                          int n_tau, bool as_text, uint64_t *out, int64_t out_len, int64_t *n_pairs, float *kernel_ms) {
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device: the comparison has no CPU path");
  const std::vector<miso_batch *> all = same_events_groups(g1, n1, g2, n2);
  miso_batch &r = *all[0];
  const int n = static_cast<int>(r.events.size()), S = r.S(), nb = n1 + n2;
  if (S < 1) MISO_FAIL(MISO_EINVAL, "Too few samples to compare");
  for (int g = 0; g < 2; g++) {
    const int64_t N = static_cast<int64_t>(g ? n2 : n1) * S;
    if (N > PAIRS_GROUP_MAX_DRAWS)
      MISO_FAIL(MISO_EINVAL, "group " + std::to_string(g + 1) + ": Too many samples for the pooled all-pairs comparison: " +
                                 std::to_string(g ? n2 : n1) + " batches of " + std::to_string(S) + " are " + std::to_string(N) +
                                 " draws, 16384 per event and group at most");
  }
  const int N1 = n1 * S, N2 = n2 * S;
  const int64_t M = static_cast<int64_t>(N1) * N2;
  const PairsArgs pa = pairs_args(M, confidence_level, tau, n_tau);
  ColumnLayout l = column_layout(r, 1);
  const int kmax = l.kmax;
  const size_t W = static_cast<size_t>(pairs_words(n_tau));
  const uint64_t need_len = l.total * W;
  if (out_len < 0 || static_cast<uint64_t>(out_len) < need_len) MISO_FAIL(MISO_EINVAL, "out is too short for pairs_words(n_tau) words per column");
  if (need_len && !out) MISO_FAIL(MISO_EINVAL, "out is NULL");
  if (n_pairs) *n_pairs = M;
  if (kernel_ms) *kernel_ms = 0.f;
  if (n == 0) return;
  HIP_OK(hipSetDevice(r.device));
  for (miso_batch *b : all) { finish_rounds(*b); HIP_OK(hipStreamSynchronize(b->stream)); }
  // an event whose sample text some batch did not decode (adopt_text): the kernel does not touch its columns
  for (int i = 0; i < n; i++)
    for (miso_batch *b : all)
      if (b->event_unread(i)) l.off[i] |= PAIRS_SKIP_EVENT;

  const size_t dyn = static_cast<size_t>(std::max(N1, N2)) * sizeof(uint64_t);   // what is live, not the limit
  const size_t row = static_cast<size_t>(kmax) * N1 * sizeof(double);           // an event's rows of the workspace
  const int per_launch = static_cast<int>(std::min<size_t>(n, std::max<size_t>(1, PAIRS_GROUP_WORK_BYTES / row)));

  const std::vector<const void *> ptrs = group_pointers(all);
  HipCall call(r.stream);
  const void *const *d_ptrs = call.upload(ptrs.data(), ptrs.size() * sizeof(void *));
  double *d_work = call.alloc(row * per_launch);
  // (the launches follow one another in the stream, each with the whole workspace: one pair of events times their sum)
  const float ms = column_pass(call, fn(compare_pairs_groups_kernel), dim3(n, kmax), dyn, l.off, need_len, out,
                               [&](dim3 grid, const uint64_t *d_off, uint64_t *d_res) {
                                 for (int e0 = 0; e0 < n; e0 += per_launch) {
                                   const int ne = std::min(per_launch, n - e0);
                                   hipLaunchKernelGGL(compare_pairs_groups_kernel, dim3(ne, grid.y), dim3(256), dyn, call.st,
                                                      reinterpret_cast<const DevEvent *const *>(d_ptrs),
                                                      reinterpret_cast<const unsigned char *const *>(d_ptrs) + nb, n1, n2, S, e0, ne, kmax,
                                                      pa, as_text ? 1 : 0, d_off, d_res, d_work);
                                   HIP_OK(hipGetLastError());
                                 }
                               });
  if (kernel_ms) *kernel_ms = ms;
}

}  // namespace miso
