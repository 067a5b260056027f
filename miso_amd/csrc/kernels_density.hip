// kernels_density.hip -- per-base read density and junction counts of many regions in one pass over an alignment file:
// what sashimi_plot draws (misopy/sashimi_plot/plot_utils/plot_gene.py:48-57, 398-444, readsToWiggle_pysam), for a whole
// list of events at once.  The rules are in include/miso_alnio.h (miso_region_densities).
//
//   host tables  per reference, the regions sorted by tx_start with a prefix maximum of tx_end: a record that no region
//                fetches leaves after one binary search.
//   mark pass    one thread per record: is it fetched by some region; its CIGAR once for the number of N ops, I / D, qlen
//                and whether it has an aligned position.  The qlen values that occur go into a bitmap (atomicOr), the
//                counters of the stats into integer atomics.  The class table holds only the qlen that occur.
//   group pass   the regions are cut into groups whose accumulators fit the byte budget.  Per group the records stream
//                through again; a fetched record walks its CIGAR once per region it touches and adds, per aligned block
//                [s, e), +1 and -1 to a difference array diff[region][class][L + 1] (two integer atomics per block), and
//                appends its junction keys (region, leftss, rightss) to a list whose capacity is checked (a list that
//                would overrun is only counted; the group is then run again with the counted capacity).
//   scan         one workgroup per (region, class) row: differences -> depths of that qlen class.
//   finish       depth = sum over the classes; wiggle = sum over the classes in ascending qlen of depth_q / q in double.
//   junctions    keys back to the host, sorted and run-length counted there (a few per spliced record of the regions:
//                small beside the record pass).
// The columns stream through two pinned buffers on two streams; a chunk is bounded in records and in CIGAR words, so
// device memory is bounded by the chunk and the budget.  Integer accumulators only: no result depends on the chunk size,
// the grouping or the order of the records.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
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
constexpr int64_t kDefaultBudget = int64_t{1} << 30;
constexpr int kWordsPerRecord = 4;             // CIGAR words a chunk holds per record slot (a longer CIGAR ends the chunk early)
constexpr int kMaxQlen = 1 << 16;              // qlen values the bitmap holds: 1 .. kMaxQlen - 1
constexpr int64_t kCoordLimit = int64_t{1} << 40;
constexpr int64_t kFirstJxnCap = int64_t{1} << 20;

// counters of the mark pass
enum { kFetched = 0, kMultiN, kNoCigar, kIndel, kQlenOver, kNCounters };

struct RecordInfo {
  int n_skip;       // N ops
  bool indel;       // an I or a D op
  bool aligned;     // at least one M / = / X base
  int64_t qlen;     // M + I + = + X
};

__device__ inline RecordInfo cigar_info(const uint32_t *cg, uint32_t n_ops) {
  RecordInfo r{0, false, false, 0};
  for (uint32_t k = 0; k < n_ops; k++) {
    const uint32_t w = cg[k], op = w & 15u, len = w >> 4;
    if (op == 0 || op == 7 || op == 8) { r.qlen += len; r.aligned |= len > 0; }
    else if (op == 1) { r.qlen += len; r.indel = true; }
    else if (op == 2) r.indel = true;
    else if (op == 3) r.n_skip++;
  }
  return r;
}

// the regions of reference rid are [ref_off[rid], ref_off[rid + 1]), sorted by start; returns the first index whose
// start is not below e (the regions before it have tx_start < bam_endpos)
__device__ inline int64_t first_start_ge(const int64_t *r_start, int64_t lo, int64_t hi, int64_t e) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (r_start[mid] < e) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kBlock) void density_mark_kernel(const int32_t *ref_id, const int32_t *pos,
                                                             const int32_t *end, const uint32_t *cig_off,
                                                             const uint32_t *cigar, int n, const int64_t *ref_off,
                                                             int n_refs, const int64_t *r_start, const int64_t *r_pmax,
                                                             unsigned int *qlen_bits, unsigned long long *counters) {
  const int i = static_cast<int>(blockIdx.x) * kBlock + static_cast<int>(threadIdx.x);
  if (i >= n) return;
  const int rid = ref_id[i];
  if (rid < 0 || rid >= n_refs) return;
  const int64_t p = pos[i], e = end[i];
  const int64_t first = ref_off[rid];
  const int64_t stop = first_start_ge(r_start, first, ref_off[rid + 1], e);
  if (stop == first || r_pmax[stop - 1] <= p) return;          // no region with tx_start < endpos && tx_end > pos
  atomicAdd(counters + kFetched, 1ull);
  const uint32_t c0 = cig_off[i], n_ops = cig_off[i + 1] - c0;
  if (n_ops == 0) { atomicAdd(counters + kNoCigar, 1ull); return; }
  const RecordInfo r = cigar_info(cigar + c0, n_ops);
  if (r.n_skip > 1) { atomicAdd(counters + kMultiN, 1ull); return; }
  if (r.indel) atomicAdd(counters + kIndel, 1ull);
  if (!r.aligned) return;
  if (r.qlen >= kMaxQlen) { atomicMax(counters + kQlenOver, static_cast<unsigned long long>(r.qlen)); return; }
  atomicOr(qlen_bits + (r.qlen >> 5), 1u << (r.qlen & 31));
}

// one slot of the junction list for every calling lane: one atomic per wavefront and call
__device__ inline unsigned long long wave_list_slot(unsigned long long *counter) {
  const uint64_t active = __ballot(1);
  const int lane = static_cast<int>(__lane_id());
  const int leader = __ffsll(static_cast<unsigned long long>(active)) - 1;
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(counter, static_cast<unsigned long long>(__popcll(active)));
  base = __shfl(base, leader);
  return base + static_cast<unsigned long long>(__popcll(active & ((uint64_t{1} << lane) - 1)));
}

// the group's regions: r_start / r_end (tx_start, tx_end as given), r_pmax, r_acc (first element of the region's
// difference rows), r_len (L = tx_end - tx_start + 1), r_index (the caller's region number)
__global__ __launch_bounds__(kBlock) void density_record_kernel(
    const int32_t *ref_id, const int32_t *pos, const int32_t *end, const uint32_t *cig_off, const uint32_t *cigar, int n,
    const int64_t *ref_off, int n_refs, const int64_t *r_start, const int64_t *r_end, const int64_t *r_pmax,
    const int64_t *r_acc, const int64_t *r_len, const int32_t *r_index, const int32_t *class_of_qlen, int *diff,
    int32_t *jx_region, uint64_t *jx_sites, unsigned long long jx_cap, unsigned long long *jx_count) {
  const int i = static_cast<int>(blockIdx.x) * kBlock + static_cast<int>(threadIdx.x);
  if (i >= n) return;
  const int rid = ref_id[i];
  if (rid < 0 || rid >= n_refs) return;
  const int64_t p = pos[i], e = end[i];
  const int64_t first = ref_off[rid];
  const int64_t stop = first_start_ge(r_start, first, ref_off[rid + 1], e);
  if (stop == first || r_pmax[stop - 1] <= p) return;
  const uint32_t c0 = cig_off[i], n_ops = cig_off[i + 1] - c0;
  if (n_ops == 0) return;
  const uint32_t *cg = cigar + c0;
  const RecordInfo info = cigar_info(cg, n_ops);
  if (info.n_skip > 1 || !info.aligned || info.qlen >= kMaxQlen) return;
  const int cls = class_of_qlen[info.qlen];
  if (cls < 0) return;                                            // cannot happen: the mark pass saw this record
  for (int64_t j = stop - 1; j >= first && r_pmax[j] > p; j--) {
    const int64_t t0 = r_start[j], t1 = r_end[j];
    if (!(t1 > p)) continue;                                      // fetched: pos < tx_end && endpos > tx_start
    const int64_t L = r_len[j];
    int *row = diff + r_acc[j] + static_cast<int64_t>(cls) * (L + 1);
    int64_t x = p, last = 0;                                      // last: the previous aligned position, once there is one
    bool have_last = false;
    for (uint32_t k = 0; k < n_ops; k++) {
      const uint32_t w = cg[k], op = w & 15u;
      const int64_t len = w >> 4;
      if (op == 0 || op == 7 || op == 8) {
        if (len == 0) continue;
        if (have_last && x > last + 1 && last >= t0 && last <= t1) {
          const int64_t ls = last + 1, rs = x + 1;
          if (ls > t0 && ls < t1 && rs > t0 && rs < t1) {
            const unsigned long long slot = wave_list_slot(jx_count);
            if (slot < jx_cap) {
              jx_region[slot] = r_index[j];
              jx_sites[slot] = (static_cast<uint64_t>(ls) << 32) | static_cast<uint64_t>(static_cast<uint32_t>(rs));
            }
          }
        }
        const int64_t lo = x > t0 ? x : t0, hi = (x + len - 1) < t1 ? (x + len - 1) : t1;
        if (lo <= hi) {
          atomicAdd(row + (lo - t0), 1);
          atomicAdd(row + (hi - t0 + 1), -1);                     // <= L: the row has L + 1 entries
        }
        x += len;
        last = x - 1;
        have_last = true;
      } else if (op == 2 || op == 3) {
        x += len;
      }
    }
  }
}

// in-place inclusive prefix sum of one (region, class) row of L + 1 differences: entry b becomes the depth at base b
__global__ __launch_bounds__(kBlock) void density_scan_kernel(const int64_t *r_acc, const int64_t *r_len, int n_classes,
                                                             int *diff) {
  __shared__ int part[kBlock];
  const int64_t region = blockIdx.x / static_cast<unsigned>(n_classes);
  const int cls = static_cast<int>(blockIdx.x % static_cast<unsigned>(n_classes));
  const int64_t len = r_len[region] + 1;
  int *row = diff + r_acc[region] + static_cast<int64_t>(cls) * len;
  const int t = static_cast<int>(threadIdx.x);
  int carry = 0;
  for (int64_t base = 0; base < len; base += 4 * kBlock) {
    const int64_t at = base + 4 * t;
    int v[4];
    for (int k = 0; k < 4; k++) v[k] = at + k < len ? row[at + k] : 0;
    v[1] += v[0]; v[2] += v[1]; v[3] += v[2];
    part[t] = v[3];
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {                        // Hillis-Steele over the 256 partial sums
      const int add = t >= d ? part[t - d] : 0;
      __syncthreads();
      part[t] += add;
      __syncthreads();
    }
    const int before = carry + (t > 0 ? part[t - 1] : 0);
    const int total = part[kBlock - 1];
    for (int k = 0; k < 4; k++)
      if (at + k < len) row[at + k] = v[k] + before;
    carry += total;
    __syncthreads();
  }
}

// one workgroup per region: depth and wiggle of its bases from the class rows; qlen_of_class ascending
__global__ __launch_bounds__(kBlock) void density_finish_kernel(const int64_t *r_acc, const int64_t *r_len,
                                                               const int64_t *r_out, int n_classes,
                                                               const int32_t *qlen_of_class, const int *diff,
                                                               int32_t *depth, double *wiggle) {
  const int64_t region = blockIdx.x;
  const int64_t L = r_len[region];
  const int *rows = diff + r_acc[region];
  int32_t *d = depth + r_out[region];
  double *w = wiggle + r_out[region];
  for (int64_t b = threadIdx.x; b < L; b += kBlock) {
    int32_t total = 0;
    double sum = 0.0;
    for (int c = 0; c < n_classes; c++) {
      const int dq = rows[static_cast<int64_t>(c) * (L + 1) + b];
      total += dq;
      sum += static_cast<double>(dq) / static_cast<double>(qlen_of_class[c]);
    }
    d[b] = total;
    w[b] = sum;
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
  void release(void *p) {
    dev.erase(std::find(dev.begin(), dev.end(), p));
    (void) hipFree(p);
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

// the lookup tables of a set of regions (numbers into the caller's list), per reference sorted by tx_start
struct Tables {
  std::vector<int64_t> ref_off, start, end, pmax;
  std::vector<int32_t> index;
};

Tables build_tables(int nref, const std::vector<int32_t> &regions, const std::vector<int> &rid, const int64_t *start,
                    const int64_t *end) {
  Tables t;
  t.ref_off.assign(static_cast<size_t>(nref) + 1, 0);
  for (int32_t i : regions) t.ref_off[rid[i] + 1]++;
  for (int r = 0; r < nref; r++) t.ref_off[r + 1] += t.ref_off[r];
  t.index.resize(regions.size());
  std::vector<int64_t> fill(t.ref_off.begin(), t.ref_off.end() - 1);
  for (int32_t i : regions) t.index[static_cast<size_t>(fill[rid[i]]++)] = i;
  t.start.resize(regions.size());
  t.end.resize(regions.size());
  t.pmax.resize(regions.size());
  for (int r = 0; r < nref; r++) {
    std::stable_sort(t.index.begin() + t.ref_off[r], t.index.begin() + t.ref_off[r + 1],
                     [&](int32_t a, int32_t b) { return start[a] < start[b]; });
    int64_t m = INT64_MIN;
    for (int64_t j = t.ref_off[r]; j < t.ref_off[r + 1]; j++) {
      const int32_t i = t.index[static_cast<size_t>(j)];
      t.start[j] = start[i];
      t.end[j] = end[i];
      t.pmax[j] = m = std::max(m, end[i]);
    }
  }
  return t;
}

}  // namespace

void region_densities(const miso_alnfile_t *f, int device, int n_regions, const char *const *seqid, const int64_t *start,
                      const int64_t *end, int64_t chunk, int64_t accum_bytes, int32_t *depth, double *wiggle,
                      int64_t out_cap, int32_t *jxn_region, int64_t *jxn_left, int64_t *jxn_right, int64_t *jxn_count,
                      int64_t jxn_cap, int64_t *n_jxn, miso_density_stats_t *stats) {
  const auto t_call = std::chrono::steady_clock::now();
  if (!f) MISO_FAIL(MISO_EINVAL, "alignment file must not be NULL");
  if (n_regions < 0) MISO_FAIL(MISO_EINVAL, "region count out of range");
  if (n_regions > 0 && (!seqid || !start || !end)) MISO_FAIL(MISO_EINVAL, "region arrays must not be NULL");
  if (!n_jxn) MISO_FAIL(MISO_EINVAL, "n_jxn must not be NULL");
  if (jxn_cap < 0 || (jxn_cap > 0 && (!jxn_region || !jxn_left || !jxn_right || !jxn_count)))
    MISO_FAIL(MISO_EINVAL, "junction arrays must not be NULL when jxn_cap > 0");
  // the output layout: region i at out_off[i], L_i entries
  std::vector<int64_t> out_off(static_cast<size_t>(n_regions) + 1, 0);
  for (int i = 0; i < n_regions; i++) {
    if (!seqid[i]) MISO_FAIL(MISO_EINVAL, "region seqid must not be NULL");
    if (start[i] < -kCoordLimit || start[i] > kCoordLimit || end[i] < -kCoordLimit || end[i] > kCoordLimit)
      MISO_FAIL(MISO_EINVAL, "region " + std::to_string(i) + ": coordinate out of range");
    out_off[i + 1] = out_off[i] + (start[i] <= end[i] ? end[i] - start[i] + 1 : 0);
  }
  const int64_t total_out = out_off[static_cast<size_t>(n_regions)];
  if (total_out > out_cap) MISO_FAIL(MISO_EINVAL, "depth / wiggle hold " + std::to_string(out_cap) + " entries, the regions need " + std::to_string(total_out));
  if (total_out > 0 && (!depth || !wiggle)) MISO_FAIL(MISO_EINVAL, "depth and wiggle must not be NULL");
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device: the density pass has no CPU path");
  set_device(device);
  miso_aln_columns_t c;
  if (miso_aln_columns(f, &c) != 0) MISO_FAIL(MISO_EINVAL, miso_aln_last_error());
  miso_density_stats_t st{};
  if (total_out > 0) {
    std::memset(depth, 0, static_cast<size_t>(total_out) * sizeof(int32_t));
    std::memset(wiggle, 0, static_cast<size_t>(total_out) * sizeof(double));
  }
  *n_jxn = 0;

  // ---- host tables over every region the file can serve ----
  auto t0 = std::chrono::steady_clock::now();
  const int nref = miso_aln_n_refs(f);
  std::vector<int> rid(static_cast<size_t>(n_regions), -1);
  std::vector<int32_t> valid;
  for (int i = 0; i < n_regions; i++) {
    rid[i] = miso_aln_ref_id(f, seqid[i]);
    if (rid[i] >= 0 && start[i] <= end[i]) valid.push_back(i);
  }
  const Tables all = build_tables(nref, valid, rid, start, end);
  st.tables_ms = ms_since(t0);
  const int64_t N = c.n;
  if (valid.empty() || N == 0) {
    st.total_ms = ms_since(t_call);
    if (stats) *stats = st;
    return;
  }

  // ---- chunks: at most C records and at most W CIGAR words each ----
  const int64_t C = std::min<int64_t>(chunk > 0 ? chunk : kDefaultChunk, int64_t{1} << 28);
  const int64_t slot_n = std::min<int64_t>(C, N);
  uint64_t longest = 0;
  for (int64_t i = 0; i < N; i++) longest = std::max(longest, c.cigar_off[i + 1] - c.cigar_off[i]);
  if (longest >= (uint64_t{1} << 31)) MISO_FAIL(MISO_EINVAL, "a CIGAR too long for the density pass");
  const int64_t W = std::max<int64_t>(kWordsPerRecord * slot_n, static_cast<int64_t>(longest));
  std::vector<int64_t> chunk_first{0};
  while (chunk_first.back() < N) {
    const int64_t first = chunk_first.back();
    const uint64_t *fit = std::upper_bound(c.cigar_off + first, c.cigar_off + N + 1, c.cigar_off[first] + static_cast<uint64_t>(W));
    const int64_t by_words = (fit - c.cigar_off) - 1;             // the last record whose CIGAR still ends within W
    chunk_first.push_back(std::min<int64_t>(std::min(first + C, N), std::max(by_words, first + 1)));
  }
  const int64_t n_chunks = static_cast<int64_t>(chunk_first.size()) - 1;

  Scratch s;
  struct Slot { int32_t *h_in, *d_in; hipStream_t st; hipEvent_t e0, e1; bool busy; };
  Slot slot[2];
  const size_t slot_words = static_cast<size_t>(4 * slot_n + 1 + W);   // ref | pos | end | cigar_off (n + 1) | cigar
  for (Slot &q : slot) {
    q.h_in = s.host<int32_t>(slot_words);
    q.d_in = s.alloc<int32_t>(slot_words);
    q.st = s.stream(); q.e0 = s.event(); q.e1 = s.event(); q.busy = false;
  }
  double device_ms = 0.0;
  auto drain = [&](Slot &q) {
    HIP_OK(hipStreamSynchronize(q.st));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, q.e0, q.e1));
    device_ms += ms;
    q.busy = false;
  };
  const int T = std::min(miso_usable_threads(), 16);
  // streams every chunk through the two slots; `launch` enqueues the kernel of the pass on the slot's stream
  auto stream_records = [&](auto &&launch) {
    for (int64_t k = 0; k < n_chunks; k++) {
      Slot &q = slot[k & 1];
      if (q.busy) drain(q);
      const int64_t first = chunk_first[k], cn = chunk_first[k + 1] - first;
      const uint64_t w0 = c.cigar_off[first];
      const int64_t wn = static_cast<int64_t>(c.cigar_off[first + cn] - w0);
      int32_t *h_rid = q.h_in, *h_pos = q.h_in + slot_n, *h_end = q.h_in + 2 * slot_n;
      uint32_t *h_off = reinterpret_cast<uint32_t *>(q.h_in + 3 * slot_n);
      uint32_t *h_cig = reinterpret_cast<uint32_t *>(q.h_in + 4 * slot_n + 1);
      parallel_for(cn, T, [&](int64_t lo, int64_t hi) {
        std::memcpy(h_rid + lo, c.ref_id + first + lo, static_cast<size_t>(hi - lo) * 4);
        std::memcpy(h_pos + lo, c.pos + first + lo, static_cast<size_t>(hi - lo) * 4);
        std::memcpy(h_end + lo, c.end + first + lo, static_cast<size_t>(hi - lo) * 4);
        for (int64_t r = lo; r < hi; r++) h_off[r] = static_cast<uint32_t>(c.cigar_off[first + r] - w0);
        const uint64_t a = c.cigar_off[first + lo] - w0, b = c.cigar_off[first + hi] - w0;
        std::memcpy(h_cig + a, c.cigar + w0 + a, static_cast<size_t>(b - a) * 4);
      });
      h_off[cn] = static_cast<uint32_t>(wn);
      HIP_OK(hipEventRecord(q.e0, q.st));
      for (int p = 0; p < 3; p++)
        HIP_OK(hipMemcpyAsync(q.d_in + p * slot_n, q.h_in + p * slot_n, static_cast<size_t>(cn) * 4,
                                  hipMemcpyHostToDevice, q.st));
      HIP_OK(hipMemcpyAsync(q.d_in + 3 * slot_n, q.h_in + 3 * slot_n, static_cast<size_t>(cn + 1) * 4,
                                hipMemcpyHostToDevice, q.st));
      if (wn > 0)
        HIP_OK(hipMemcpyAsync(q.d_in + 4 * slot_n + 1, q.h_in + 4 * slot_n + 1, static_cast<size_t>(wn) * 4,
                                  hipMemcpyHostToDevice, q.st));
      launch(q.d_in, q.d_in + slot_n, q.d_in + 2 * slot_n, reinterpret_cast<const uint32_t *>(q.d_in + 3 * slot_n),
             reinterpret_cast<const uint32_t *>(q.d_in + 4 * slot_n + 1), static_cast<int>(cn), q.st);
      HIP_OK(hipGetLastError());
      HIP_OK(hipEventRecord(q.e1, q.st));
      q.busy = true;
    }
    for (Slot &q : slot)
      if (q.busy) drain(q);
  };
  auto blocks_of = [](int n) { return dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)); };

  // ---- mark pass: the stats and the qlen classes ----
  int64_t *d_ref_off = s.alloc<int64_t>(static_cast<size_t>(nref) + 1);
  int64_t *d_start = s.alloc<int64_t>(valid.size()), *d_end = s.alloc<int64_t>(valid.size());
  int64_t *d_pmax = s.alloc<int64_t>(valid.size()), *d_acc = s.alloc<int64_t>(valid.size());
  int64_t *d_len = s.alloc<int64_t>(valid.size()), *d_out = s.alloc<int64_t>(valid.size());
  int32_t *d_index = s.alloc<int32_t>(valid.size());
  auto put = [&](auto *dst, const auto &v) {
    if (!v.empty()) HIP_OK(hipMemcpy(dst, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice));
  };
  put(d_ref_off, all.ref_off); put(d_start, all.start); put(d_pmax, all.pmax);
  unsigned int *d_bits = s.alloc<unsigned int>(kMaxQlen / 32);
  unsigned long long *d_counters = s.alloc<unsigned long long>(kNCounters);
  HIP_OK(hipMemset(d_bits, 0, kMaxQlen / 32 * sizeof(unsigned int)));
  HIP_OK(hipMemset(d_counters, 0, kNCounters * sizeof(unsigned long long)));
  stream_records([&](const int32_t *r, const int32_t *p, const int32_t *e, const uint32_t *off, const uint32_t *cg, int n,
                     hipStream_t q) {
    density_mark_kernel<<<blocks_of(n), dim3(kBlock), 0, q>>>(r, p, e, off, cg, n, d_ref_off, nref, d_start, d_pmax,
                                                             d_bits, d_counters);
  });
  st.mark_ms = device_ms;
  device_ms = 0.0;
  std::vector<unsigned int> bits(kMaxQlen / 32);
  unsigned long long counters[kNCounters];
  HIP_OK(hipMemcpy(bits.data(), d_bits, bits.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(counters, d_counters, sizeof(counters), hipMemcpyDeviceToHost));
  if (counters[kQlenOver])
    MISO_FAIL(MISO_EINVAL, "a fetched record has qlen " + std::to_string(counters[kQlenOver]) + ": the density pass holds qlen up to " + std::to_string(kMaxQlen - 1));
  st.fetched = static_cast<int64_t>(counters[kFetched]);
  st.skipped_multi_n = static_cast<int64_t>(counters[kMultiN]);
  st.skipped_no_cigar = static_cast<int64_t>(counters[kNoCigar]);
  st.with_indel = static_cast<int64_t>(counters[kIndel]);
  st.chunks = n_chunks;
  std::vector<int32_t> class_of(kMaxQlen, -1), qlen_of;
  for (int q = 1; q < kMaxQlen; q++)
    if (bits[q >> 5] >> (q & 31) & 1u) { class_of[q] = static_cast<int32_t>(qlen_of.size()); qlen_of.push_back(q); }
  const int n_classes = static_cast<int>(qlen_of.size());
  st.qlen_classes = n_classes;
  if (n_classes == 0) {                                           // nothing aligned inside any region: all zero
    st.total_ms = ms_since(t_call);
    if (stats) *stats = st;
    return;
  }
  const int32_t *d_class_of = s.upload(class_of), *d_qlen_of = s.upload(qlen_of);

  // ---- groups of regions whose accumulators fit the budget ----
  const int64_t budget = accum_bytes > 0 ? accum_bytes : kDefaultBudget;
  auto region_bytes = [&](int32_t i) {
    const int64_t L = end[i] - start[i] + 1;
    return (static_cast<int64_t>(n_classes) * (L + 1)) * 4 + L * 12;   // difference rows, depth, wiggle
  };
  std::vector<size_t> group_first{0};
  int64_t max_diff = 0, max_out = 0;
  {
    int64_t bytes = 0, dn = 0, on = 0;
    for (size_t v = 0; v < valid.size(); v++) {
      const int64_t need = region_bytes(valid[v]), L = end[valid[v]] - start[valid[v]] + 1;
      if (v > group_first.back() && bytes + need > budget) {
        group_first.push_back(v);
        bytes = dn = on = 0;
      }
      bytes += need; dn += static_cast<int64_t>(n_classes) * (L + 1); on += L;
      max_diff = std::max(max_diff, dn); max_out = std::max(max_out, on);
    }
    group_first.push_back(valid.size());
  }
  st.groups = static_cast<int64_t>(group_first.size()) - 1;
  int *d_diff = s.alloc<int>(static_cast<size_t>(max_diff));
  int32_t *d_depth = s.alloc<int32_t>(static_cast<size_t>(max_out));
  double *d_wiggle = s.alloc<double>(static_cast<size_t>(max_out));
  std::vector<int32_t> h_depth(static_cast<size_t>(max_out));
  std::vector<double> h_wiggle(static_cast<size_t>(max_out));
  unsigned long long *d_jx_count = s.alloc<unsigned long long>(1);
  int64_t jx_cap = kFirstJxnCap;
  int32_t *d_jx_region = s.alloc<int32_t>(static_cast<size_t>(jx_cap));
  uint64_t *d_jx_sites = s.alloc<uint64_t>(static_cast<size_t>(jx_cap));
  struct Key { int32_t region; uint64_t sites; };
  std::vector<Key> keys;
  std::vector<int32_t> h_jx_region;
  std::vector<uint64_t> h_jx_sites;

  for (size_t g = 0; g + 1 < group_first.size(); g++) {
    t0 = std::chrono::steady_clock::now();
    const std::vector<int32_t> members(valid.begin() + group_first[g], valid.begin() + group_first[g + 1]);
    const Tables t = build_tables(nref, members, rid, start, end);
    // accumulators and outputs in the order of the table
    std::vector<int64_t> acc(members.size()), len(members.size()), out(members.size());
    int64_t dn = 0, on = 0;
    for (size_t j = 0; j < members.size(); j++) {
      len[j] = t.end[j] - t.start[j] + 1;
      acc[j] = dn; out[j] = on;
      dn += static_cast<int64_t>(n_classes) * (len[j] + 1); on += len[j];
    }
    put(d_ref_off, t.ref_off); put(d_start, t.start); put(d_end, t.end); put(d_pmax, t.pmax);
    put(d_acc, acc); put(d_len, len); put(d_out, out); put(d_index, t.index);
    st.tables_ms += ms_since(t0);
    for (;;) {
      HIP_OK(hipMemset(d_diff, 0, static_cast<size_t>(dn) * sizeof(int)));
      HIP_OK(hipMemset(d_jx_count, 0, sizeof(unsigned long long)));
      const unsigned long long cap = static_cast<unsigned long long>(jx_cap);
      stream_records([&](const int32_t *r, const int32_t *p, const int32_t *e, const uint32_t *off, const uint32_t *cg,
                         int n, hipStream_t q) {
        density_record_kernel<<<blocks_of(n), dim3(kBlock), 0, q>>>(r, p, e, off, cg, n, d_ref_off, nref, d_start, d_end,
                                                                   d_pmax, d_acc, d_len, d_index, d_class_of, d_diff,
                                                                   d_jx_region, d_jx_sites, cap, d_jx_count);
      });
      st.records_ms += device_ms;
      device_ms = 0.0;
      unsigned long long found = 0;
      HIP_OK(hipMemcpy(&found, d_jx_count, sizeof(found), hipMemcpyDeviceToHost));
      if (found <= cap) {
        t0 = std::chrono::steady_clock::now();
        h_jx_region.resize(found); h_jx_sites.resize(found);
        if (found) {
          HIP_OK(hipMemcpy(h_jx_region.data(), d_jx_region, found * sizeof(int32_t), hipMemcpyDeviceToHost));
          HIP_OK(hipMemcpy(h_jx_sites.data(), d_jx_sites, found * sizeof(uint64_t), hipMemcpyDeviceToHost));
        }
        for (size_t k = 0; k < found; k++) keys.push_back(Key{h_jx_region[k], h_jx_sites[k]});
        st.junction_ms += ms_since(t0);
        break;
      }
      // the list would have overrun: nothing beyond its capacity was written; again with room for all of them
      s.release(d_jx_region); s.release(d_jx_sites);
      jx_cap = static_cast<int64_t>(found);
      d_jx_region = s.alloc<int32_t>(static_cast<size_t>(jx_cap));
      d_jx_sites = s.alloc<uint64_t>(static_cast<size_t>(jx_cap));
      st.junction_retries++;
    }
    // scan and finish
    hipEvent_t e0 = slot[0].e0, e1 = slot[0].e1;
    hipStream_t qs = slot[0].st;
    HIP_OK(hipEventRecord(e0, qs));
    const int64_t rows = static_cast<int64_t>(members.size()) * n_classes;
    if (rows >= (int64_t{1} << 31)) MISO_FAIL(MISO_EINVAL, "too many (region, class) rows in one group: lower the budget");
    density_scan_kernel<<<dim3(static_cast<unsigned>(rows)), dim3(kBlock), 0, qs>>>(d_acc, d_len, n_classes, d_diff);
    HIP_OK(hipGetLastError());
    density_finish_kernel<<<dim3(static_cast<unsigned>(members.size())), dim3(kBlock), 0, qs>>>(
        d_acc, d_len, d_out, n_classes, d_qlen_of, d_diff, d_depth, d_wiggle);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(e1, qs));
    HIP_OK(hipStreamSynchronize(qs));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    st.scan_ms += ms;
    t0 = std::chrono::steady_clock::now();
    HIP_OK(hipMemcpy(h_depth.data(), d_depth, static_cast<size_t>(on) * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h_wiggle.data(), d_wiggle, static_cast<size_t>(on) * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t j = 0; j < members.size(); j++) {
      const int32_t i = t.index[j];
      std::memcpy(depth + out_off[i], h_depth.data() + out[j], static_cast<size_t>(len[j]) * sizeof(int32_t));
      std::memcpy(wiggle + out_off[i], h_wiggle.data() + out[j], static_cast<size_t>(len[j]) * sizeof(double));
    }
    st.copy_ms += ms_since(t0);
  }

  // ---- junctions: sort the keys, count the runs ----
  t0 = std::chrono::steady_clock::now();
  std::sort(keys.begin(), keys.end(), [](const Key &a, const Key &b) {
    return a.region != b.region ? a.region < b.region : a.sites < b.sites;
  });
  int64_t n_out = 0;
  for (size_t k = 0; k < keys.size();) {
    size_t m = k;
    while (m < keys.size() && keys[m].region == keys[k].region && keys[m].sites == keys[k].sites) m++;
    if (n_out < jxn_cap) {
      jxn_region[n_out] = keys[k].region;
      jxn_left[n_out] = static_cast<int64_t>(keys[k].sites >> 32);
      jxn_right[n_out] = static_cast<int64_t>(keys[k].sites & 0xFFFFFFFFu);
      jxn_count[n_out] = static_cast<int64_t>(m - k);
    }
    n_out++;
    k = m;
  }
  *n_jxn = n_out;
  st.junction_ms += ms_since(t0);
  st.total_ms = ms_since(t_call);
  if (stats) *stats = st;
}

}  // namespace miso
