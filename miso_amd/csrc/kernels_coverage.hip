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
//                size and the interval count; every chunk adds into the same histograms.
//   rank step    inclusive prefix sums: PA[j] = kept records with key(ref, pos) < A[j], PB[j] = kept records with
//                key(ref, bam_endpos) < B[j]; interval i's count is PA[its place in A] - PB[its place in B].
//                Records on lower references are in both terms and cancel; a span that ends at or before start - 1
//                also begins before end, so the difference counts exactly the spans that overlap [start - 1, end).
// Integer work throughout: the counts do not depend on the chunk size or the order of the records in the file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "hip_host.hpp"
#include "host.hpp"
#include "miso_alnio.h"

namespace miso {

int device_count();
void set_device(int d);

namespace {

constexpr int kBlock = 256;
constexpr int64_t kDefaultChunk = int64_t{1} << 22;

// (reference, coordinate) as one ordered 64-bit key: the coordinate biased into 33 bits (every record coordinate is an
// int32; interval coordinates beyond the range clamp to keys outside every record's)
__host__ __device__ inline uint64_t rank_key(int64_t ref, int64_t x) {
  const int64_t lim = int64_t{1} << 32;
  x = x < -lim ? -lim : (x > lim - 1 ? lim - 1 : x);
  return (static_cast<uint64_t>(ref) << 33) + static_cast<uint64_t>(x + lim);
}

__device__ inline int64_t upper_bound_u64(const uint64_t *v, int64_t n, uint64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (v[mid] <= key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// adds 1 to bins[k] for every lane with k >= 0: one atomic per distinct bin and wavefront
__device__ inline void wave_bin_add(unsigned long long *bins, int64_t k) {
  const int lane = static_cast<int>(__lane_id());
  uint64_t todo = __ballot(k >= 0);
  while (todo) {
    const int leader = __ffsll(static_cast<unsigned long long>(todo)) - 1;
    const int64_t lk = __shfl(k, leader);
    const uint64_t same = __ballot(k == lk);
    if (lane == leader) atomicAdd(bins + lk, static_cast<unsigned long long>(__popcll(same)));
    todo &= ~same;
  }
}

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

template <class F> void parallel_for(int64_t n, int T, F &&body) {
  T = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(T, n / 65536 + 1)));
  std::vector<std::thread> th;
  for (int t = 1; t < T; t++) th.emplace_back([&, t] { body(n * t / T, n * (t + 1) / T); });
  body(0, n / T);
  for (auto &x : th) x.join();
}

// everything the pass allocates, released however it ends
struct Scratch {
  std::vector<void *> dev, pinned;
  std::vector<hipStream_t> streams;
  std::vector<hipEvent_t> events;
  template <class T> T *alloc(size_t count) {
    void *p = nullptr;
    HIP_OK(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)));
    dev.push_back(p);
    return static_cast<T *>(p);
  }
  template <class T> T *upload(const std::vector<T> &v) {
    T *d = alloc<T>(v.size());
    if (!v.empty()) HIP_OK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
  }
  template <class T> T *host(size_t count) {
    void *p = nullptr;
    HIP_OK(hipHostMalloc(&p, std::max<size_t>(count, 1) * sizeof(T), hipHostMallocDefault));
    pinned.push_back(p);
    return static_cast<T *>(p);
  }
  hipStream_t stream() {
    hipStream_t s = nullptr;
    HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    streams.push_back(s);
    return s;
  }
  hipEvent_t event() {
    hipEvent_t e = nullptr;
    HIP_OK(hipEventCreate(&e));
    events.push_back(e);
    return e;
  }
  ~Scratch() {
    for (hipStream_t s : streams) { (void) hipStreamSynchronize(s); (void) hipStreamDestroy(s); }
    for (hipEvent_t e : events) (void) hipEventDestroy(e);
    for (void *p : dev) (void) hipFree(p);
    for (void *p : pinned) (void) hipHostFree(p);
  }
};

struct Tables {
  std::vector<int64_t> ref_off, s0, pmax;   // containment, per reference
  std::vector<uint64_t> keys_a, keys_b;     // sorted rank keys of the valid intervals
  std::vector<int64_t> at_a, at_b;          // interval i's place in keys_a / keys_b (-1: counts 0)
};

Tables build_tables(const miso_alnfile_t *f, int n_iv, const char *const *seqid, const int64_t *start,
                    const int64_t *end) {
  const int nref = miso_aln_n_refs(f);
  Tables t;
  std::vector<int> rid(static_cast<size_t>(n_iv));
  t.ref_off.assign(static_cast<size_t>(nref) + 1, 0);
  for (int i = 0; i < n_iv; i++) {
    if (!seqid[i]) MISO_FAIL(MISO_EINVAL, "interval seqid must not be NULL");
    rid[i] = miso_aln_ref_id(f, seqid[i]);
    if (rid[i] >= 0) t.ref_off[rid[i] + 1]++;
  }
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
  t.at_a.assign(static_cast<size_t>(n_iv), -1);
  t.at_b.assign(static_cast<size_t>(n_iv), -1);
  for (int i = 0; i < n_iv; i++)
    if (rid[i] >= 0 && start[i] <= end[i]) {
      t.keys_a.push_back(rank_key(rid[i], end[i]));
      t.keys_b.push_back(rank_key(rid[i], start[i]));
    }
  std::sort(t.keys_a.begin(), t.keys_a.end());
  std::sort(t.keys_b.begin(), t.keys_b.end());
  for (int i = 0; i < n_iv; i++)
    if (rid[i] >= 0 && start[i] <= end[i]) {
      t.at_a[i] = std::lower_bound(t.keys_a.begin(), t.keys_a.end(), rank_key(rid[i], end[i])) - t.keys_a.begin();
      t.at_b[i] = std::lower_bound(t.keys_b.begin(), t.keys_b.end(), rank_key(rid[i], start[i])) - t.keys_b.begin();
    }
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
  const int64_t N = c.n;
  const int64_t C = std::min<int64_t>(chunk > 0 ? chunk : kDefaultChunk, int64_t{1} << 30);
  const int64_t n_a = static_cast<int64_t>(t.keys_a.size()), n_b = static_cast<int64_t>(t.keys_b.size());

  Scratch s;
  const int64_t *d_off = s.upload(t.ref_off), *d_s0 = s.upload(t.s0), *d_pmax = s.upload(t.pmax);
  const uint64_t *d_ka = s.upload(t.keys_a), *d_kb = s.upload(t.keys_b);
  // hA | hB | kept, one allocation, zeroed once: every chunk adds into it
  const size_t n_bins = static_cast<size_t>(n_a + n_b + 1);
  unsigned long long *d_bins = s.alloc<unsigned long long>(n_bins);
  unsigned long long *d_ha = d_bins, *d_hb = d_bins + n_a, *d_kept = d_bins + n_a + n_b;
  HIP_OK(hipMemset(d_bins, 0, n_bins * 8));

  const int64_t slot_n = std::min<int64_t>(C, std::max<int64_t>(N, 1));
  struct Slot { int32_t *h_in, *d_in; hipStream_t st; hipEvent_t e0, e1; bool busy; };
  Slot slot[2];
  for (Slot &q : slot) {
    q.h_in = s.host<int32_t>(3 * slot_n);
    q.d_in = s.alloc<int32_t>(3 * slot_n);
    q.st = s.stream(); q.e0 = s.event(); q.e1 = s.event(); q.busy = false;
  }
  auto drain = [&](Slot &q) {
    HIP_OK(hipStreamSynchronize(q.st));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, q.e0, q.e1));
    st.records_ms += ms;
    q.busy = false;
  };
  const int T = std::min(miso_usable_threads(), 16);
  int64_t chunks = 0;
  for (int64_t first = 0; first < N; first += C, chunks++) {
    Slot &q = slot[chunks & 1];
    if (q.busy) drain(q);
    const int64_t cn = std::min(C, N - first);
    // three planes of slot_n: reference (-1 when unmapped), pos, bam_endpos
    int32_t *h_rid = q.h_in, *h_pos = q.h_in + slot_n, *h_end = q.h_in + 2 * slot_n;
    parallel_for(cn, T, [&](int64_t lo, int64_t hi) {
      std::memcpy(h_pos + lo, c.pos + first + lo, static_cast<size_t>(hi - lo) * 4);
      std::memcpy(h_end + lo, c.end + first + lo, static_cast<size_t>(hi - lo) * 4);
      for (int64_t k = lo; k < hi; k++) h_rid[k] = (c.flag[first + k] & 0x4) ? -1 : c.ref_id[first + k];
    });
    HIP_OK(hipEventRecord(q.e0, q.st));
    for (int p = 0; p < 3; p++)
      HIP_OK(hipMemcpyAsync(q.d_in + p * slot_n, q.h_in + p * slot_n, static_cast<size_t>(cn) * 4,
                                hipMemcpyHostToDevice, q.st));
    const int n = static_cast<int>(cn);
    coverage_record_kernel<<<dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, q.st>>>(
        q.d_in, q.d_in + slot_n, q.d_in + 2 * slot_n, n, d_off, nref, d_s0, d_pmax, d_ka, n_a, d_kb, n_b, d_ha, d_hb,
        d_kept);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(q.e1, q.st));
    q.busy = true;
  }
  for (Slot &q : slot)
    if (q.busy) drain(q);

  // rank step: the histograms back, prefix sums, one difference per interval
  t0 = std::chrono::steady_clock::now();
  std::vector<unsigned long long> bins(n_bins);
  HIP_OK(hipMemcpy(bins.data(), d_bins, n_bins * 8, hipMemcpyDeviceToHost));
  std::partial_sum(bins.begin(), bins.begin() + n_a, bins.begin());
  std::partial_sum(bins.begin() + n_a, bins.begin() + n_a + n_b, bins.begin() + n_a);
  for (int i = 0; i < n_iv; i++)
    counts[i] = t.at_a[i] < 0 ? 0
                              : static_cast<int64_t>(bins[static_cast<size_t>(t.at_a[i])]) -
                                    static_cast<int64_t>(bins[static_cast<size_t>(n_a + t.at_b[i])]);
  st.rank_ms = ms_since(t0);
  st.kept = static_cast<int64_t>(bins[n_bins - 1]);
  st.chunks = chunks;
  st.total_ms = ms_since(t_call);
  if (stats) *stats = st;
}

}  // namespace miso
