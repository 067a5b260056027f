// kernels_coverage.hip -- per-interval read coverage on the device: what `miso --run --prefilter` needs
// `bedtools intersect -abam BAM -b genes.gff -f 1 -ubam | bedtools coverage -abam - -b genes.gff -counts` for
// (misopy/exon_utils.py:198-250, run_events_analysis.py:28-68).
//
//   host tables  per reference, the intervals sorted by start - 1 with a prefix maximum of their ends (is a record held
//                whole by SOME interval: one binary search), and two sorted arrays of rank keys, A = the intervals'
//                key(ref, end) and B = their key(ref, start) (start 1-based).
//   record pass  one thread per record: kept or not; for a kept record a = upper_bound(A, key(ref, pos)) and
//                b = upper_bound(B, key(ref, bam_endpos)), added to two histograms hA[a], hB[b] with integer atomics
//                aggregated per wavefront (neighbouring records of a sorted file share their bins).  The columns
//                stream through in chunks, two in flight on two streams, so device memory is bounded by the chunk
//                size and the interval count; every chunk adds into the same histograms.  (The keys, the histogram
//                add, the chunk loop and the rank step are record_pass.hpp's, shared with kernels_rpkm.hip.)
//   rank step    inclusive prefix sums: PA[j] = kept records with key(ref, pos) < A[j], PB[j] = kept records with
//                key(ref, bam_endpos) < B[j]; interval i's count is PA[its place in A] - PB[its place in B].
//                Records on lower references are in both terms and cancel; a span that ends at or before start - 1
//                also begins before end, so the difference counts exactly the spans that overlap [start - 1, end).
// Integer work throughout: the counts do not depend on the chunk size or the order of the records in the file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "hip_host.hpp"
#include "host.hpp"
#include "miso_alnio.h"
#include "record_pass.hpp"

namespace miso {

int device_count();
void set_device(int d);

namespace {

using namespace record_pass;   // rank_key, upper_bound_u64, wave_bin_add, Scratch, the chunk loop

// ref_id < 0 for a record that cannot be kept (unmapped); s0 / pmax: the intervals of reference r in
// [ref_off[r], ref_off[r + 1]), sorted by s0 = start - 1, pmax = the largest end up to and including each one
__global__ __launch_bounds__(kBlock) void coverage_record_kernel(const int32_t *ref_id, const int32_t *pos,
                                                                const int32_t *end, int n, const int64_t *ref_off,
                                                                int n_refs, const int64_t *s0, const int64_t *pmax,
                                                                const uint64_t *keys_a, int64_t n_a,
                                                                const uint64_t *keys_b, int64_t n_b,
                                                                unsigned long long *hist_a,
                                                                unsigned long long *hist_b,
                                                                unsigned long long *n_kept) {
  const int i = static_cast<int>(blockIdx.x) * kBlock + static_cast<int>(threadIdx.x);
  int64_t a = -1, b = -1;
  bool kept = false;
  if (i < n) {
    const int rid = ref_id[i];
    if (rid >= 0 && rid < n_refs) {
      const int32_t p = pos[i], e = end[i];
      int64_t lo = ref_off[rid], hi = ref_off[rid + 1];
      const int64_t first = lo;
      while (lo < hi) {                              // the first interval with s0 > pos
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (s0[mid] <= p) lo = mid + 1;
        else hi = mid;
      }
      kept = lo > first && pmax[lo - 1] >= e;
      if (kept) {
        a = upper_bound_u64(keys_a, n_a, rank_key(rid, p));
        b = upper_bound_u64(keys_b, n_b, rank_key(rid, e));
        if (a == n_a) a = -1;                        // above every A key: no interval counts it
        if (b == n_b) b = -1;
      }
    }
  }
  const uint64_t km = __ballot(kept);
  if (km && static_cast<int>(__lane_id()) == __ffsll(static_cast<unsigned long long>(km)) - 1)
    atomicAdd(n_kept, static_cast<unsigned long long>(__popcll(km)));
  wave_bin_add(hist_a, a);
  wave_bin_add(hist_b, b);
}

struct Tables {
  std::vector<int64_t> ref_off, s0, pmax;   // containment, per reference
  RankKeys rank;                            // A = key(ref, end), B = key(ref, start), start 1-based
};

Tables build_tables(const miso_alnfile_t *f, int n_iv, const char *const *seqid, const int64_t *start,
                    const int64_t *end) {
  const int nref = miso_aln_n_refs(f);
  Tables t;
  const std::vector<int> rid = interval_refs(f, n_iv, seqid);
  t.ref_off.assign(static_cast<size_t>(nref) + 1, 0);
  for (int i = 0; i < n_iv; i++)
    if (rid[i] >= 0) t.ref_off[rid[i] + 1]++;
  for (int r = 0; r < nref; r++) t.ref_off[r + 1] += t.ref_off[r];
  std::vector<int32_t> order(static_cast<size_t>(t.ref_off[nref]));
  std::vector<int64_t> fill(t.ref_off.begin(), t.ref_off.end() - 1);
  for (int i = 0; i < n_iv; i++)
    if (rid[i] >= 0) order[static_cast<size_t>(fill[rid[i]]++)] = i;
  t.s0.resize(order.size());
  t.pmax.resize(order.size());
  for (int r = 0; r < nref; r++) {
    std::sort(order.begin() + t.ref_off[r], order.begin() + t.ref_off[r + 1],
              [&](int32_t a, int32_t b) { return start[a] < start[b]; });
    int64_t m = INT64_MIN;
    for (int64_t j = t.ref_off[r]; j < t.ref_off[r + 1]; j++) {
      const int32_t i = order[static_cast<size_t>(j)];
      t.s0[j] = start[i] - 1;
      t.pmax[j] = m = std::max(m, end[i]);
    }
  }
  t.rank = build_rank_keys(n_iv, rid, start, end, 0);
  return t;
}

}  // namespace

void region_counts(const miso_alnfile_t *f, int device, int n_iv, const char *const *seqid, const int64_t *start,
                   const int64_t *end, int64_t chunk, int64_t *counts, miso_region_stats_t *stats) {
  const auto t_call = std::chrono::steady_clock::now();
  if (!f) MISO_FAIL(MISO_EINVAL, "alignment file must not be NULL");
  if (n_iv < 0) MISO_FAIL(MISO_EINVAL, "interval count out of range");
  if (n_iv > 0 && (!seqid || !start || !end || !counts)) MISO_FAIL(MISO_EINVAL, "interval arrays must not be NULL");
  if (miso_aln_n_refs(f) >= (1 << 30)) MISO_FAIL(MISO_EINVAL, "too many references for the rank keys");
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device: the coverage pass has no CPU path");
  set_device(device);
  miso_aln_columns_t c;
  if (miso_aln_columns(f, &c) != 0) MISO_FAIL(MISO_EINVAL, miso_aln_last_error());
  miso_region_stats_t st{};
  auto t0 = std::chrono::steady_clock::now();
  const Tables t = build_tables(f, n_iv, seqid, start, end);
  st.sort_ms = ms_since(t0);
  const int nref = static_cast<int>(t.ref_off.size()) - 1;
  const int64_t n_a = static_cast<int64_t>(t.rank.keys_a.size()), n_b = static_cast<int64_t>(t.rank.keys_b.size());

  Scratch s;
  const int64_t *d_off = s.upload(t.ref_off), *d_s0 = s.upload(t.s0), *d_pmax = s.upload(t.pmax);
  const uint64_t *d_ka = s.upload(t.rank.keys_a), *d_kb = s.upload(t.rank.keys_b);
  // hA | hB | kept, one allocation, zeroed once: every chunk adds into it
  const size_t n_bins = static_cast<size_t>(n_a + n_b + 1);
  unsigned long long *d_bins = s.alloc<unsigned long long>(n_bins);
  unsigned long long *d_ha = d_bins, *d_hb = d_bins + n_a, *d_kept = d_bins + n_a + n_b;
  HIP_OK(hipMemset(d_bins, 0, n_bins * 8));

  // three planes per chunk: reference (-1 when unmapped), pos, bam_endpos
  st.chunks = for_record_chunks(
      s, c.n, chunk_size(chunk), &st.records_ms,
      [&](int64_t first, int64_t lo, int64_t hi, int32_t *h_rid, int32_t *h_pos, int32_t *h_end) {
        std::memcpy(h_pos + lo, c.pos + first + lo, static_cast<size_t>(hi - lo) * 4);
        std::memcpy(h_end + lo, c.end + first + lo, static_cast<size_t>(hi - lo) * 4);
        for (int64_t k = lo; k < hi; k++) h_rid[k] = (c.flag[first + k] & 0x4) ? -1 : c.ref_id[first + k];
      },
      [&](const int32_t *d_rid, const int32_t *d_pos, const int32_t *d_end, int n, hipStream_t stream) {
        coverage_record_kernel<<<record_grid(n), dim3(kBlock), 0, stream>>>(d_rid, d_pos, d_end, n, d_off, nref, d_s0,
                                                                           d_pmax, d_ka, n_a, d_kb, n_b, d_ha, d_hb,
                                                                           d_kept);
      });

  // rank step: the histograms back, prefix sums, one difference per interval
  t0 = std::chrono::steady_clock::now();
  std::vector<unsigned long long> bins(n_bins);
  HIP_OK(hipMemcpy(bins.data(), d_bins, n_bins * 8, hipMemcpyDeviceToHost));
  rank_counts(t.rank, bins, n_iv, counts);
  st.rank_ms = ms_since(t0);
  st.kept = static_cast<int64_t>(bins[n_bins - 1]);
  st.total_ms = ms_since(t_call);
  if (stats) *stats = st;
}

}  // namespace miso
