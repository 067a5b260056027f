// kernels_rpkm.hip -- bamfile.fetch(chrom, start, end) counted for many intervals in one pass over the records: what
// `sam_rpkm --compute-rpkm` needs for every constitutive exon of an annotation (misopy/sam_rpkm.py:138-154, one index
// look-up per exon there).  include/miso_alnio.h (miso_fetch_counts) has the rule: the records on the interval's
// reference with pos < end && bam_endpos > start, the numbers used as given, no flag considered.
//
//   host tables  two sorted arrays of rank keys over the valid intervals (reference in the file, start <= end):
//                A = key(ref, end) and B = key(ref, start + 1).
//   record pass  one thread per record with a reference: a = upper_bound(A, key(ref, pos)) and
//                b = upper_bound(B, key(ref, bam_endpos)), added to two histograms hA[a], hB[b] with integer atomics
//                aggregated per wavefront (neighbouring records of a sorted file share their bins).  The columns stream
//                through in chunks, two in flight on two streams; every chunk adds into the same histograms.
//   rank step    inclusive prefix sums: PA[j] = records with key(ref, pos) < A[j], PB[j] = records with
//                key(ref, bam_endpos) < B[j], that is bam_endpos <= start on the interval's reference, or a lower
//                reference.  Interval i counts PA[its place in A] - PB[its place in B].
// Why the difference is the fetch count: records on lower references are in both terms and cancel, records on higher
// ones are in neither.  On the interval's own reference pos < bam_endpos always (alnio: bam_endpos >= pos + 1), so with
// start <= end a record with bam_endpos <= start also has pos < end: the second set lies inside the first, and what is
// left is pos < end && bam_endpos > start.  No containment test, unlike the coverage pass, and B is one higher than
// there (start, not start - 1, is the last position a record may end on without overlapping).
// The keys, the histogram add, the chunk loop and the rank step are record_pass.hpp's, shared with kernels_coverage.hip.
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

using namespace record_pass;

// ref_id < 0: a record without a reference counts nowhere.  A rank equal to the key count (above every key) is no bin.
__global__ __launch_bounds__(kBlock) void fetch_record_kernel(const int32_t *ref_id, const int32_t *pos,
                                                             const int32_t *end, int n, int n_refs,
                                                             const uint64_t *keys_a, int64_t n_a,
                                                             const uint64_t *keys_b, int64_t n_b,
                                                             unsigned long long *hist_a,
                                                             unsigned long long *hist_b) {
  const int i = static_cast<int>(blockIdx.x) * kBlock + static_cast<int>(threadIdx.x);
  int64_t a = -1, b = -1;
  if (i < n) {
    const int rid = ref_id[i];
    if (rid >= 0 && rid < n_refs) {
      a = upper_bound_u64(keys_a, n_a, rank_key(rid, pos[i]));
      b = upper_bound_u64(keys_b, n_b, rank_key(rid, end[i]));
      if (a == n_a) a = -1;
      if (b == n_b) b = -1;
    }
  }
  wave_bin_add(hist_a, a);
  wave_bin_add(hist_b, b);
}

}  // namespace

void fetch_counts(const miso_alnfile_t *f, int device, int n_iv, const char *const *seqid, const int64_t *start,
                  const int64_t *end, int64_t chunk, int64_t *counts, miso_region_stats_t *stats) {
  const auto t_call = std::chrono::steady_clock::now();
  if (!f) MISO_FAIL(MISO_EINVAL, "alignment file must not be NULL");
  if (n_iv < 0) MISO_FAIL(MISO_EINVAL, "interval count out of range");
  if (n_iv > 0 && (!seqid || !start || !end || !counts)) MISO_FAIL(MISO_EINVAL, "interval arrays must not be NULL");
  const int nref = miso_aln_n_refs(f);
  if (nref >= (1 << 30)) MISO_FAIL(MISO_EINVAL, "too many references for the rank keys");
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device: the fetch-count pass has no CPU path");
  set_device(device);
  miso_aln_columns_t c;
  if (miso_aln_columns(f, &c) != 0) MISO_FAIL(MISO_EINVAL, miso_aln_last_error());
  miso_region_stats_t st{};
  auto t0 = std::chrono::steady_clock::now();
  const RankKeys t = build_rank_keys(n_iv, interval_refs(f, n_iv, seqid), start, end, 1);
  st.sort_ms = ms_since(t0);
  const int64_t n_a = static_cast<int64_t>(t.keys_a.size()), n_b = static_cast<int64_t>(t.keys_b.size());

  Scratch s;
  const uint64_t *d_ka = s.upload(t.keys_a), *d_kb = s.upload(t.keys_b);
  // hA | hB, one allocation, zeroed once: every chunk adds into it
  const size_t n_bins = static_cast<size_t>(n_a + n_b);
  unsigned long long *d_bins = s.alloc<unsigned long long>(n_bins);
  unsigned long long *d_ha = d_bins, *d_hb = d_bins + n_a;
  HIP_OK(hipMemset(d_bins, 0, std::max<size_t>(n_bins, 1) * 8));

  // three planes per chunk: reference, pos, bam_endpos, as the file has them
  st.chunks = for_record_chunks(
      s, c.n, chunk_size(chunk), &st.records_ms,
      [&](int64_t first, int64_t lo, int64_t hi, int32_t *h_rid, int32_t *h_pos, int32_t *h_end) {
        std::memcpy(h_rid + lo, c.ref_id + first + lo, static_cast<size_t>(hi - lo) * 4);
        std::memcpy(h_pos + lo, c.pos + first + lo, static_cast<size_t>(hi - lo) * 4);
        std::memcpy(h_end + lo, c.end + first + lo, static_cast<size_t>(hi - lo) * 4);
      },
      [&](const int32_t *d_rid, const int32_t *d_pos, const int32_t *d_end, int n, hipStream_t stream) {
        fetch_record_kernel<<<record_grid(n), dim3(kBlock), 0, stream>>>(d_rid, d_pos, d_end, n, nref, d_ka, n_a, d_kb,
                                                                        n_b, d_ha, d_hb);
      });

  // rank step: the histograms back, prefix sums, one difference per interval
  t0 = std::chrono::steady_clock::now();
  std::vector<unsigned long long> bins(n_bins);
  if (n_bins) HIP_OK(hipMemcpy(bins.data(), d_bins, n_bins * 8, hipMemcpyDeviceToHost));
  rank_counts(t, bins, n_iv, counts);
  st.rank_ms = ms_since(t0);
  st.kept = c.n;   // nothing is filtered: every record of the file went through the pass
  st.total_ms = ms_since(t_call);
  if (stats) *stats = st;
}

}  // namespace miso
