// kernels_summary.hip -- posterior summaries on the device.
//
// The reference summarises an event from its .miso file (misopy/samples_utils.py:263-329 ->
// credible_intervals.py:4-72): posterior mean of every isoform's psi and the Chen-Shao interval,
// i.e. the order statistics number round(alpha/2 n) and round((1-alpha/2) n) of the sorted samples.
// Doing that where the samples already are avoids shipping 8(K+1)S bytes per event over PCIe
// (4.8 GB for the 40 000-event benchmark batch) just to reduce them to 3K numbers.
//
// One workgroup per (event, isoform) column:
//   * mean: thread t sums samples t, t+256, ... in order, then a fixed binary tree over the 256
//     partial sums -- a deterministic order the CPU checker reproduces exactly;
//   * order statistics: exact radix select (8 passes of 8 bits over order-preserving 64-bit keys),
//     no sort, no extra memory; the value returned IS one of the samples.
#include <hip/hip_runtime.h>

#include "compare_column.hpp"
#include "device.hpp"
#include "miso_detmath.h"
#include "order_key.hpp"
#include "text_digits.hpp"

namespace miso {

// TEXT: summarise what summarize_miso READS, not what the sampler computed: every sample as "%.4f" prints it
// (text_digits.hpp text_digits).
template <bool CACHED, bool TEXT>
__device__ __forceinline__ void summarize_column(const double *x, int K, int S, int rank_lo, int rank_hi,
                                                 double *o) {
  __shared__ double part[256];
  __shared__ long long ipart[256];
  __shared__ int s_nonfinite;
  if (TEXT) { if (threadIdx.x == 0) s_nonfinite = 0; __syncthreads(); }
  long long iacc = 0;
  auto as_read = [&](double v) {   // TEXT: the sample as the `.miso` file hands it on
    if (!TEXT) return v;
    if (!text_rounds(v)) { s_nonfinite = 1; return v; }     // "nan" / "inf" / an integer of 16 digits stay what they are
    const long long k = text_digits(v);
    iacc += k;
    return static_cast<double>(k) / 10000.0;
  };
  __shared__ unsigned hist2[2][256];
  __shared__ unsigned wave_tot2[2][4];
  __shared__ uint64_t s_prefix2[2];
  __shared__ int s_rank2[2];
  __shared__ int s_single2[2];
  const int t = threadIdx.x;

  uint64_t keys[CACHED ? SUMMARY_CACHE : 1];
  double acc = 0.0;
  if (CACHED) {
#pragma unroll
    for (int j = 0; j < SUMMARY_CACHE; j++) {
      const int s = t + 256 * j;
      if (s < S) {
        const double v = as_read(x[static_cast<size_t>(s) * K]);
        acc = acc + v;
        keys[j] = order_key(v);
      } else {
        keys[j] = 0;
      }
    }
  } else {
    for (int s = t; s < S; s += 256) acc = acc + as_read(x[static_cast<size_t>(s) * K]);
  }
  part[t] = acc;
  if (TEXT) ipart[t] = iacc;
  __syncthreads();
  for (int stride = 128; stride >= 1; stride >>= 1) {
    if (t < stride) { part[t] = part[t] + part[t + stride]; if (TEXT) ipart[t] = ipart[t] + ipart[t + stride]; }
    __syncthreads();
  }
  const double mean = !TEXT ? part[0] / static_cast<double>(S)
                            : (s_nonfinite ? part[0] / static_cast<double>(S)
                                           : static_cast<double>(ipart[0]) / (static_cast<double>(S) * 10000.0));

  // both order statistics in the same eight passes: two prefixes, two histograms (the keys are
  // tested against both; while the two ranks still share a prefix the two histograms are equal)
  double stat[2];
  if (t < 2) { s_prefix2[t] = 0; s_rank2[t] = t == 0 ? rank_lo : rank_hi; s_single2[t] = 0; }
  __syncthreads();
  for (int byte = 7; byte >= 0; byte--) {
    hist2[0][t] = 0; hist2[1][t] = 0;
    __syncthreads();
    const uint64_t p0 = s_prefix2[0], p1 = s_prefix2[1];
    const uint64_t mask = (byte == 7) ? 0ull : (~0ull << (8 * (byte + 1)));
    if (CACHED) {
      // psi lies in [0, 1]: the leading bytes of all keys coincide, so in the first passes every key
      // of the column lands in ONE bin and 5000 same-address LDS atomics serialise.  Each thread
      // therefore adds runs of equal bins at once, and a wavefront whose pending runs all name the
      // same bin adds their total with a single atomic.
      unsigned cb[2] = {0u, 0u}, cn[2] = {0u, 0u};
#pragma unroll
      for (int j = 0; j < SUMMARY_CACHE; j++) {
        if (t + 256 * j < S) {
          const uint64_t km = keys[j] & mask;
          const unsigned bin = static_cast<unsigned>(keys[j] >> (8 * byte)) & 0xFFu;
#pragma unroll
          for (int w = 0; w < 2; w++) {
            if (km == (w == 0 ? p0 : p1)) {
              if (cn[w] && cb[w] != bin) { atomicAdd(&hist2[w][cb[w]], cn[w]); cn[w] = 0; }
              cb[w] = bin; cn[w]++;
            }
          }
        }
      }
#pragma unroll
      for (int w = 0; w < 2; w++) {
        const unsigned long long have = __ballot(cn[w] != 0);
        if (have) {
          const unsigned b0 = static_cast<unsigned>(__shfl(static_cast<int>(cb[w]), __ffsll(static_cast<long long>(have)) - 1));
          if (__all(cn[w] == 0 || cb[w] == b0)) {
            unsigned tot = cn[w];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) tot += __shfl_xor(static_cast<int>(tot), off);
            if ((t & 63) == 0) atomicAdd(&hist2[w][b0], tot);
          } else if (cn[w]) {
            atomicAdd(&hist2[w][cb[w]], cn[w]);
          }
        }
      }
    } else {
      for (int s = t; s < S; s += 256) {
        const double vq = x[static_cast<size_t>(s) * K];
        const uint64_t key = order_key((TEXT && text_rounds(vq)) ? static_cast<double>(text_digits(vq)) / 10000.0 : vq);
        const uint64_t km = key & mask;
        const unsigned bin = static_cast<unsigned>(key >> (8 * byte)) & 0xFFu;
        if (km == p0) atomicAdd(&hist2[0][bin], 1u);
        if (km == p1) atomicAdd(&hist2[1][bin], 1u);
      }
    }
    __syncthreads();
    {
      // which bin holds the wanted rank: inclusive prefix sums of the 256 bins, one bin per thread
      // (wave scan + the earlier waves' totals through LDS) -- thread 0 walking the bins one LDS
      // read at a time was ~25 k cycles per pass
      unsigned h[2], inc[2];
#pragma unroll
      for (int w = 0; w < 2; w++) {
        h[w] = hist2[w][t]; inc[w] = h[w];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const unsigned v = __shfl_up(inc[w], off);
          if ((t & 63) >= off) inc[w] += v;
        }
        if ((t & 63) == 63) wave_tot2[w][t >> 6] = inc[w];
      }
      const int r0[2] = {s_rank2[0], s_rank2[1]};
      __syncthreads();
#pragma unroll
      for (int w = 0; w < 2; w++) {
        unsigned before = 0;
        for (int q = 0; q < (t >> 6); q++) before += wave_tot2[w][q];
        const unsigned incl = inc[w] + before, exc = incl - h[w];
        const unsigned r = static_cast<unsigned>(r0[w]);
        // the first bin whose running total exceeds the rank; the last bin takes what is left
        if ((r >= exc && r < incl) || (t == 255 && r >= incl)) {
          s_rank2[w] = static_cast<int>(r - exc);
          s_prefix2[w] = (w == 0 ? p0 : p1) | (static_cast<uint64_t>(t) << (8 * byte));
          s_single2[w] = h[w] == 1u;   // one key left under this prefix: it IS the order statistic
        }
      }
    }
    __syncthreads();
    // Early exit: 5000 keys rarely share more than their leading four or five bytes, so after that many
    // passes each wanted rank is alone in its bin; the remaining passes would only spell out its low bytes.
    // The lone key is fetched from the registers instead (the value returned is still one of the samples).
    if (CACHED && byte > 0 && s_single2[0] && s_single2[1]) {
      const uint64_t q0 = s_prefix2[0], q1 = s_prefix2[1];
      const uint64_t m2 = ~0ull << (8 * byte);
      __syncthreads();
#pragma unroll
      for (int j = 0; j < SUMMARY_CACHE; j++) {
        if (t + 256 * j < S) {
          if ((keys[j] & m2) == q0) s_prefix2[0] = keys[j];
          if ((keys[j] & m2) == q1) s_prefix2[1] = keys[j];
        }
      }
      __syncthreads();
      break;
    }
  }
  stat[0] = key_value(s_prefix2[0]);
  stat[1] = key_value(s_prefix2[1]);
  if (t == 0) { o[0] = mean; o[1] = stat[0]; o[2] = stat[1]; }
}

__global__ __launch_bounds__(256) void summarize_kernel(const DevEvent *events, const unsigned char *out_pool,
                                                        int n_events, int S, int rank_lo, int rank_hi,
                                                        const uint64_t *sum_off, double *summary, int as_text) {
  const int ev = blockIdx.x, k = blockIdx.y;
  if (ev >= n_events) return;
  const DevEvent E = events[ev];
  if (k >= E.K) return;
  const double *x = reinterpret_cast<const double *>(out_pool + E.off_samples) + k;
  double *o = summary + sum_off[ev] + 3 * k;
  if (as_text) {
    if (S <= 256 * SUMMARY_CACHE) summarize_column<true, true>(x, E.K, S, rank_lo, rank_hi, o);
    else summarize_column<false, true>(x, E.K, S, rank_lo, rank_hi, o);
  } else if (S <= 256 * SUMMARY_CACHE) summarize_column<true, false>(x, E.K, S, rank_lo, rank_hi, o);
  else summarize_column<false, false>(x, E.K, S, rank_lo, rank_hi, o);
}


// ---- two-sample comparison --------------------------------------------
// compare_column (compare_column.hpp, shared with the group pass of kernels_compare_groups.hip) per (event, isoform).
__global__ __launch_bounds__(256) void compare_kernel(const DevEvent *ev1, const unsigned char *pool1,
                                                      const DevEvent *ev2, const unsigned char *pool2,
                                                      int n_events, int S, double smoothing,
                                                      const uint64_t *cmp_off, double *out) {
  const int ev = blockIdx.x, k = blockIdx.y;
  if (ev >= n_events) return;
  const DevEvent E1 = ev1[ev], E2 = ev2[ev];
  const int K = E1.K;
  if (k >= K) return;
  const double *x1 = reinterpret_cast<const double *>(pool1 + E1.off_samples) + k;
  const double *x2 = reinterpret_cast<const double *>(pool2 + E2.off_samples) + k;
  double *o = out + cmp_off[ev] + 4 * k;
  __shared__ CompareScratch sc;
  if (S <= 256 * SUMMARY_CACHE) compare_column<true>(x1, K, x2, K, S, smoothing, o, sc);
  else compare_column<false>(x1, K, x2, K, S, smoothing, o, sc);
}

}  // namespace miso
