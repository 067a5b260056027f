// record_pass.hpp -- what the passes that rank every record of an alignment file among sorted interval keys share: the
// coverage pass of `miso --run --prefilter` (kernels_coverage.hip) and the fetch counts of `sam_rpkm --compute-rpkm`
// (kernels_rpkm.hip).  The ordered (reference, coordinate) key, its binary search, the wavefront-aggregated histogram
// add, the pooled allocations of one call and the loop that streams the record columns through the device in chunks, two
// in flight on two streams.  (The Scratch objects of the density, text and insert passes are their own.)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <thread>
#include <vector>

#include "hip_host.hpp"
#include "host.hpp"
#include "miso_alnio.h"

namespace miso {
namespace record_pass {

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

// records per chunk for a caller's chunk_records (<= 0: the default), at most 2^30 so that a chunk's index is an int
inline int64_t chunk_size(int64_t chunk) { return std::min<int64_t>(chunk > 0 ? chunk : kDefaultChunk, int64_t{1} << 30); }

// The two-slot chunk loop over N records, C per chunk.  Each slot holds three int32 planes of one chunk (reference, pos,
// bam_endpos) in pinned and in device memory, a stream and an event pair.  Per chunk:
//   fill(first, lo, hi, h_rid, h_pos, h_end)   on host threads: records first + [lo, hi) into the planes at [lo, hi)
//   launch(d_rid, d_pos, d_end, n, stream)     the chunk's kernel, queued behind the planes' copies
// While one slot's copies and kernel run, the host fills the other.  *records_ms gains the device time of every chunk
// (copies and kernel, by the events); the number of chunks is returned, every one of them finished.
template <class Fill, class Launch>
int64_t for_record_chunks(Scratch &s, int64_t N, int64_t C, double *records_ms, Fill &&fill, Launch &&launch) {
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
    *records_ms += ms;
    q.busy = false;
  };
  const int T = std::min(miso_usable_threads(), 16);
  int64_t chunks = 0;
  for (int64_t first = 0; first < N; first += C, chunks++) {
    Slot &q = slot[chunks & 1];
    if (q.busy) drain(q);
    const int64_t cn = std::min(C, N - first);
    int32_t *h_rid = q.h_in, *h_pos = q.h_in + slot_n, *h_end = q.h_in + 2 * slot_n;
    parallel_for(cn, T, [&](int64_t lo, int64_t hi) { fill(first, lo, hi, h_rid, h_pos, h_end); });
    HIP_OK(hipEventRecord(q.e0, q.st));
    for (int p = 0; p < 3; p++)
      HIP_OK(hipMemcpyAsync(q.d_in + p * slot_n, q.h_in + p * slot_n, static_cast<size_t>(cn) * 4,
                                hipMemcpyHostToDevice, q.st));
    launch(q.d_in, q.d_in + slot_n, q.d_in + 2 * slot_n, static_cast<int>(cn), q.st);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(q.e1, q.st));
    q.busy = true;
  }
  for (Slot &q : slot)
    if (q.busy) drain(q);
  return chunks;
}

// launch grid of one thread per record
inline dim3 record_grid(int n) { return dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)); }

// each interval's reference in the file (-1: the file does not name it)
inline std::vector<int> interval_refs(const miso_alnfile_t *f, int n_iv, const char *const *seqid) {
  std::vector<int> rid(static_cast<size_t>(n_iv));
  for (int i = 0; i < n_iv; i++) {
    if (!seqid[i]) MISO_FAIL(MISO_EINVAL, "interval seqid must not be NULL");
    rid[i] = miso_aln_ref_id(f, seqid[i]);
  }
  return rid;
}

// The rank keys of the valid intervals (reference in the file, start <= end), sorted: A = key(ref, end) and
// B = key(ref, start + b_shift); at_a / at_b: interval i's place in them, the first of equal keys (-1: it counts 0).
struct RankKeys {
  std::vector<uint64_t> keys_a, keys_b;
  std::vector<int64_t> at_a, at_b;
};

inline RankKeys build_rank_keys(int n_iv, const std::vector<int> &rid, const int64_t *start, const int64_t *end,
                                int64_t b_shift) {
  RankKeys t;
  auto key_b = [&](int i) { return rank_key(rid[i], start[i] > INT64_MAX - b_shift ? INT64_MAX : start[i] + b_shift); };
  t.at_a.assign(static_cast<size_t>(n_iv), -1);
  t.at_b.assign(static_cast<size_t>(n_iv), -1);
  for (int i = 0; i < n_iv; i++)
    if (rid[i] >= 0 && start[i] <= end[i]) {
      t.keys_a.push_back(rank_key(rid[i], end[i]));
      t.keys_b.push_back(key_b(i));
    }
  std::sort(t.keys_a.begin(), t.keys_a.end());
  std::sort(t.keys_b.begin(), t.keys_b.end());
  for (int i = 0; i < n_iv; i++)
    if (rid[i] >= 0 && start[i] <= end[i]) {
      t.at_a[i] = std::lower_bound(t.keys_a.begin(), t.keys_a.end(), rank_key(rid[i], end[i])) - t.keys_a.begin();
      t.at_b[i] = std::lower_bound(t.keys_b.begin(), t.keys_b.end(), key_b(i)) - t.keys_b.begin();
    }
  return t;
}

// The rank step on the host.  bins: the histograms as the record kernels left them, hA (one bin per A key: the records
// whose key(ref, pos) ranks there by upper_bound) then hB (the same for key(ref, bam_endpos) among the B keys), then
// whatever else the pass counts.  After the inclusive prefix sums PA[j] = the records with key(ref, pos) < A[j] and
// PB[j] = those with key(ref, bam_endpos) < B[j]; interval i counts PA[at_a[i]] - PB[at_b[i]].
inline void rank_counts(const RankKeys &t, std::vector<unsigned long long> &bins, int n_iv, int64_t *counts) {
  const size_t n_a = t.keys_a.size(), n_b = t.keys_b.size();
  std::partial_sum(bins.begin(), bins.begin() + n_a, bins.begin());
  std::partial_sum(bins.begin() + n_a, bins.begin() + n_a + n_b, bins.begin() + n_a);
  for (int i = 0; i < n_iv; i++)
    counts[i] = t.at_a[i] < 0 ? 0
                              : static_cast<int64_t>(bins[static_cast<size_t>(t.at_a[i])]) -
                                    static_cast<int64_t>(bins[n_a + static_cast<size_t>(t.at_b[i])]);
}

}  // namespace record_pass
}  // namespace miso
