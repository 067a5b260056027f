// kernels_insert.hip -- the fragment length distribution of a paired-end file on the device (misopy/pe_utils.py:148-302,
// exon_utils.py:110-196, sam_utils.py:207-290): what `pe_utils --compute-insert-len` needs tagBam, samtools and a walk
// over a Python object per record for.
//
//   record pass  one thread per record: which of the given intervals contain the record's whole span (tagBam -f 1),
//                as one int32 code (include/miso_alnio.h MISO_INSERT_*).  The columns stream through in chunks, two in
//                flight on two streams, so device memory is bounded by the chunk size and the copy of chunk i + 1
//                overlaps the kernel on chunk i.
//   grouping     on the host: the tagged records paired by name (alnio.cpp miso_aln_pair_records, the grouping the
//                per-event reader uses).
//   pair pass    one thread per pair: the checks of pe_utils.py:170-189 and the insert length, into the pair's own
//                slot, plus the kept pairs per interval with wavefront-aggregated integer atomics (their sums do not
//                depend on the order the atomics arrive in).
// Integer work throughout.
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

// alnio.cpp: the name grouping of the whole-file pass
int miso_aln_pair_records(const miso_alnfile_t *f, const int64_t *idx, int64_t n, int n_threads,
                          std::vector<int64_t> &pairs, int64_t *n_unpaired);

namespace miso {

int device_count();
void set_device(int d);

namespace {

constexpr int kBlock = 256;
constexpr int64_t kDefaultChunk = int64_t{1} << 22;
constexpr uint32_t kReverse = 1u << 31;   // pair pass input: the record's 0x10, beside the code's bits

enum PairReason { KEPT = 0, SAME_STRAND = 1, SKIPPED = 2, NONPOSITIVE = 3 };

// Intervals on reference r: [ref_off[r], ref_off[r + 1]) of s0 (start - 1), e (end) and the GFF index, ordered by
// (s0, index); maxlen[r] = the largest e - s0 among them.  A record [pos, end) lies inside an interval only if
// s0 <= pos and end <= e <= s0 + maxlen, i.e. s0 in [end - maxlen, pos]: a binary search for the first, then every
// interval up to pos is checked -- nested, overlapping and duplicate intervals included.
__global__ __launch_bounds__(kBlock) void insert_record_kernel(const int32_t *ref_id, const int32_t *pos,
                                                              const int32_t *end, const int32_t *flag, int n,
                                                              const int64_t *ref_off, const int64_t *maxlen,
                                                              int n_refs, const int64_t *iv_s0, const int64_t *iv_e,
                                                              const int32_t *iv_idx, int filter, int32_t *codes) {
  const int i = static_cast<int>(blockIdx.x) * kBlock + static_cast<int>(threadIdx.x);
  if (i >= n) return;
  const int rid = ref_id[i], p = pos[i], e = end[i], fl = flag[i];   // flag: SAM FLAG | one-M-op bit << 16
  int tag = MISO_INSERT_TAG_NONE;
  if (!(fl & 0x4) && rid >= 0 && rid < n_refs) {
    int64_t lo = ref_off[rid], hi = ref_off[rid + 1];
    const int64_t last = hi, want = static_cast<int64_t>(e) - maxlen[rid];
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (iv_s0[mid] < want) lo = mid + 1;
      else hi = mid;
    }
    int hits = 0;
    for (int64_t j = lo; j < last && iv_s0[j] <= p; j++) {
      if (iv_e[j] < e) continue;
      if (hits++) { tag = MISO_INSERT_TAG_MULTI; break; }
      tag = iv_idx[j];
    }
  }
  const bool ok = !filter || (!(fl & 0x200) && !(fl & 0x4) && !(fl & 0x8) && (fl & 0x1));
  codes[i] = tag | (((fl >> 16) & 1) ? MISO_INSERT_ONE_M : 0) | (ok ? MISO_INSERT_FILTER_OK : 0);
}

// in: per pair {left code | left 0x10 << 31, right code | right 0x10 << 31, left pos, right end}; result: the insert
// (> 0) or -reason.  per_iv[interval] += kept pairs, reasons[r] += pairs of each PairReason.
__global__ __launch_bounds__(kBlock) void insert_pair_kernel(const int4 *in, int n, int32_t *result,
                                                            unsigned long long *per_iv, unsigned long long *reasons) {
  const int i = static_cast<int>(blockIdx.x) * kBlock + static_cast<int>(threadIdx.x);
  int reason = -1, iv = -1;
  if (i < n) {
    const int4 q = in[i];
    const uint32_t a = static_cast<uint32_t>(q.x), b = static_cast<uint32_t>(q.y);
    const int ta = static_cast<int>(a & MISO_INSERT_TAG_MASK), tb = static_cast<int>(b & MISO_INSERT_TAG_MASK);
    int32_t r = 0;
    if ((a & kReverse) == (b & kReverse)) {                                       // sam_utils.py:264-271
      reason = SAME_STRAND;
    } else if (ta >= MISO_INSERT_TAG_MULTI || ta != tb || !(a & MISO_INSERT_ONE_M) || !(b & MISO_INSERT_ONE_M)) {
      reason = SKIPPED;                                                           // pe_utils.py:170-189
    } else {
      r = q.w - q.z;                        // right.pos + len(right's M) - left.pos (:199-207)
      reason = r > 0 ? KEPT : NONPOSITIVE;  // :211-214
      if (r > 0) iv = ta;
    }
    result[i] = reason == KEPT ? r : -reason;
  }
  const int lane = static_cast<int>(__lane_id());
  // one atomic per reason and wavefront
  for (int k = 0; k < 4; k++) {
    const uint64_t m = __ballot(reason == k);
    if (m && lane == __ffsll(static_cast<unsigned long long>(m)) - 1) atomicAdd(reasons + k, static_cast<unsigned long long>(__popcll(m)));
  }
  // one atomic per interval and wavefront: neighbouring pairs (file order) mostly share their interval
  uint64_t todo = __ballot(iv >= 0);
  while (todo) {
    const int leader = __ffsll(static_cast<unsigned long long>(todo)) - 1;
    const int liv = __shfl(iv, leader);
    const uint64_t same = __ballot(iv == liv);
    if (lane == leader) atomicAdd(per_iv + liv, static_cast<unsigned long long>(__popcll(same)));
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

// everything a pass allocates, released however it ends
struct DeviceScratch {
  std::vector<void *> dev, pinned;
  std::vector<hipStream_t> streams;
  template <class T> T *alloc(size_t count) {
    void *p = nullptr;
    HIP_OK(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)));
    dev.push_back(p);
    return static_cast<T *>(p);
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
  ~DeviceScratch() {
    for (hipStream_t s : streams) { (void) hipStreamSynchronize(s); (void) hipStreamDestroy(s); }
    for (void *p : dev) (void) hipFree(p);
    for (void *p : pinned) (void) hipHostFree(p);
  }
};

struct Intervals {
  std::vector<int64_t> ref_off, maxlen, s0, e;
  std::vector<int32_t> idx;
};

Intervals build_intervals(const miso_alnfile_t *f, int n_iv, const char *const *seqid, const int64_t *start,
                          const int64_t *end) {
  const int nref = miso_aln_n_refs(f);
  std::vector<int> rid(n_iv);
  Intervals iv;
  iv.ref_off.assign(static_cast<size_t>(nref) + 1, 0);
  iv.maxlen.assign(std::max(nref, 1), 0);
  for (int i = 0; i < n_iv; i++) {
    if (!seqid[i]) MISO_FAIL(MISO_EINVAL, "interval seqid must not be NULL");
    rid[i] = miso_aln_ref_id(f, seqid[i]);   // a seqid the file does not name tags nothing
    if (rid[i] >= 0) iv.ref_off[rid[i] + 1]++;
  }
  for (int r = 0; r < nref; r++) iv.ref_off[r + 1] += iv.ref_off[r];
  std::vector<int32_t> order(static_cast<size_t>(iv.ref_off[nref]));
  std::vector<int64_t> fill(iv.ref_off.begin(), iv.ref_off.end() - 1);
  for (int i = 0; i < n_iv; i++)
    if (rid[i] >= 0) order[static_cast<size_t>(fill[rid[i]]++)] = i;
  for (int r = 0; r < nref; r++)
    std::sort(order.begin() + iv.ref_off[r], order.begin() + iv.ref_off[r + 1], [&](int32_t a, int32_t b) {
      return start[a] != start[b] ? start[a] < start[b] : a < b;
    });
  for (int r = 0; r < nref; r++)
    for (int64_t j = iv.ref_off[r]; j < iv.ref_off[r + 1]; j++) {
      const int32_t i = order[static_cast<size_t>(j)];
      iv.s0.push_back(start[i] - 1);
      iv.e.push_back(end[i]);
      iv.idx.push_back(i);
      iv.maxlen[r] = std::max<int64_t>(iv.maxlen[r], end[i] - (start[i] - 1));
    }
  return iv;
}

void check_args(const miso_alnfile_t *f, int n_iv, const char *const *seqid, const int64_t *start, const int64_t *end) {
  if (!f) MISO_FAIL(MISO_EINVAL, "alignment file must not be NULL");
  if (n_iv < 0 || n_iv >= MISO_INSERT_TAG_MULTI) MISO_FAIL(MISO_EINVAL, "interval count out of range");
  if (n_iv > 0 && (!seqid || !start || !end)) MISO_FAIL(MISO_EINVAL, "interval arrays must not be NULL");
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device: the insert-length pass has no CPU path");
}

}  // namespace

// the record pass: codes[n] of the whole file, chunk by chunk, two chunks in flight
void insert_tag_records(const miso_alnfile_t *f, int device, int filter, int n_iv, const char *const *seqid,
                        const int64_t *start, const int64_t *end, int64_t chunk, int32_t *codes, int64_t *n_chunks) {
  check_args(f, n_iv, seqid, start, end);
  if (!codes) MISO_FAIL(MISO_EINVAL, "codes must not be NULL");
  set_device(device);
  miso_aln_columns_t c;
  if (miso_aln_columns(f, &c) != 0) MISO_FAIL(MISO_EINVAL, miso_aln_last_error());
  const int64_t N = c.n;
  const int64_t C = std::min<int64_t>(chunk > 0 ? chunk : kDefaultChunk, int64_t{1} << 30);
  const Intervals iv = build_intervals(f, n_iv, seqid, start, end);
  const int nref = static_cast<int>(iv.ref_off.size()) - 1;
  DeviceScratch s;
  int64_t *d_off = s.alloc<int64_t>(iv.ref_off.size()), *d_max = s.alloc<int64_t>(iv.maxlen.size());
  int64_t *d_s0 = s.alloc<int64_t>(iv.s0.size()), *d_e = s.alloc<int64_t>(iv.e.size());
  int32_t *d_idx = s.alloc<int32_t>(iv.idx.size());
  HIP_OK(hipMemcpy(d_off, iv.ref_off.data(), iv.ref_off.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_max, iv.maxlen.data(), iv.maxlen.size() * 8, hipMemcpyHostToDevice));
  if (!iv.s0.empty()) {
    HIP_OK(hipMemcpy(d_s0, iv.s0.data(), iv.s0.size() * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_e, iv.e.data(), iv.e.size() * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_idx, iv.idx.data(), iv.idx.size() * 4, hipMemcpyHostToDevice));
  }
  const int64_t slot_n = std::min<int64_t>(C, std::max<int64_t>(N, 1));
  struct Slot { int32_t *h_in, *h_codes, *d_in, *d_codes; hipStream_t st; int64_t first, n; bool busy; };
  Slot slot[2];
  for (Slot &q : slot) {
    q.h_in = s.host<int32_t>(4 * slot_n); q.h_codes = s.host<int32_t>(slot_n);
    q.d_in = s.alloc<int32_t>(4 * slot_n); q.d_codes = s.alloc<int32_t>(slot_n);
    q.st = s.stream(); q.first = q.n = 0; q.busy = false;
  }
  const int T = std::min(miso_usable_threads(), 16);
  auto drain = [&](Slot &q) {
    HIP_OK(hipStreamSynchronize(q.st));
    std::memcpy(codes + q.first, q.h_codes, static_cast<size_t>(q.n) * 4);
    q.busy = false;
  };
  int64_t chunks = 0;
  for (int64_t first = 0; first < N; first += C, chunks++) {
    Slot &q = slot[chunks & 1];
    if (q.busy) drain(q);
    q.first = first;
    q.n = std::min(C, N - first);
    // the four columns as planes of slot_n; the flag carries "CIGAR is exactly one M op" in bit 16
    int32_t *h_rid = q.h_in, *h_pos = q.h_in + slot_n, *h_end = q.h_in + 2 * slot_n, *h_flag = q.h_in + 3 * slot_n;
    parallel_for(q.n, T, [&](int64_t lo, int64_t hi) {
      std::memcpy(h_rid + lo, c.ref_id + first + lo, static_cast<size_t>(hi - lo) * 4);
      std::memcpy(h_pos + lo, c.pos + first + lo, static_cast<size_t>(hi - lo) * 4);
      std::memcpy(h_end + lo, c.end + first + lo, static_cast<size_t>(hi - lo) * 4);
      for (int64_t k = lo; k < hi; k++) {
        const int64_t r = first + k;
        const bool one_m = c.cigar_off[r + 1] - c.cigar_off[r] == 1 && (c.cigar[c.cigar_off[r]] & 15u) == 0;
        h_flag[k] = (c.flag[r] & 0xFFFF) | (one_m ? 1 << 16 : 0);
      }
    });
    for (int p = 0; p < 4; p++)
      HIP_OK(hipMemcpyAsync(q.d_in + p * slot_n, q.h_in + p * slot_n, static_cast<size_t>(q.n) * 4,
                                hipMemcpyHostToDevice, q.st));
    const int n = static_cast<int>(q.n);
    insert_record_kernel<<<dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, q.st>>>(
        q.d_in, q.d_in + slot_n, q.d_in + 2 * slot_n, q.d_in + 3 * slot_n, n, d_off, d_max, nref, d_s0, d_e, d_idx,
        filter ? 1 : 0, q.d_codes);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(q.h_codes, q.d_codes, static_cast<size_t>(q.n) * 4, hipMemcpyDeviceToHost, q.st));
    q.busy = true;
  }
  for (int k = 0; k < 2; k++) {
    Slot &q = slot[(chunks + k) & 1];   // the older chunk first
    if (q.busy) drain(q);
  }
  if (n_chunks) *n_chunks = chunks;
}

void insert_len(const miso_alnfile_t *f, int device, int filter, int n_iv, const char *const *seqid,
                const int64_t *start, const int64_t *end, int64_t chunk, int32_t *iv_out, int32_t *ins_out,
                int64_t cap, int64_t *n_kept, miso_insert_stats_t *stats) {
  if (!n_kept) MISO_FAIL(MISO_EINVAL, "n_kept must not be NULL");
  if (cap > 0 && (!iv_out || !ins_out)) MISO_FAIL(MISO_EINVAL, "output arrays must not be NULL");
  check_args(f, n_iv, seqid, start, end);
  miso_aln_columns_t c;
  if (miso_aln_columns(f, &c) != 0) MISO_FAIL(MISO_EINVAL, miso_aln_last_error());
  miso_insert_stats_t st{};
  auto t0 = std::chrono::steady_clock::now();
  std::vector<int32_t> codes(static_cast<size_t>(c.n));
  insert_tag_records(f, device, filter, n_iv, seqid, start, end, chunk, codes.data(), &st.chunks);
  st.records_ms = ms_since(t0);

  // grouping: the records that join the pairing, in file order (exon_utils.py:110-196 keeps the tagged ones)
  t0 = std::chrono::steady_clock::now();
  std::vector<int64_t> idx;
  for (int64_t i = 0; i < c.n; i++) {
    const int32_t k = codes[static_cast<size_t>(i)];
    if ((k & MISO_INSERT_TAG_MASK) != MISO_INSERT_TAG_NONE && (k & MISO_INSERT_FILTER_OK)) idx.push_back(i);
  }
  st.tagged = static_cast<int64_t>(idx.size());
  std::vector<int64_t> pairs;
  if (miso_aln_pair_records(f, idx.data(), st.tagged, 0, pairs, &st.unpaired) != 0)
    MISO_FAIL(MISO_ENOMEM, miso_aln_last_error());
  std::vector<int64_t>().swap(idx);
  const int64_t P = static_cast<int64_t>(pairs.size() / 2);
  std::vector<int4> in(static_cast<size_t>(P));
  parallel_for(P, std::min(miso_usable_threads(), 16), [&](int64_t lo, int64_t hi) {
    for (int64_t k = lo; k < hi; k++) {
      const int64_t a = pairs[2 * k], b = pairs[2 * k + 1];
      in[k].x = static_cast<int>(static_cast<uint32_t>(codes[a]) | ((c.flag[a] & 0x10) ? kReverse : 0u));
      in[k].y = static_cast<int>(static_cast<uint32_t>(codes[b]) | ((c.flag[b] & 0x10) ? kReverse : 0u));
      in[k].z = c.pos[a];
      in[k].w = c.end[b];
    }
  });
  st.grouping_ms = ms_since(t0);

  // pair pass, in chunks of the record pass's size
  t0 = std::chrono::steady_clock::now();
  std::vector<int32_t> result(static_cast<size_t>(P));
  std::vector<unsigned long long> per_iv(static_cast<size_t>(std::max(n_iv, 1))), reasons(4);
  {
    const int64_t C = std::min<int64_t>(chunk > 0 ? chunk : kDefaultChunk, int64_t{1} << 30);
    const int64_t cn = std::min<int64_t>(C, std::max<int64_t>(P, 1));
    DeviceScratch s;
    int4 *d_in = s.alloc<int4>(cn);
    int32_t *d_res = s.alloc<int32_t>(cn);
    unsigned long long *d_iv = s.alloc<unsigned long long>(per_iv.size()), *d_reasons = s.alloc<unsigned long long>(4);
    hipStream_t st_ = s.stream();
    HIP_OK(hipMemsetAsync(d_iv, 0, per_iv.size() * 8, st_));
    HIP_OK(hipMemsetAsync(d_reasons, 0, 4 * 8, st_));
    for (int64_t first = 0; first < P; first += C) {
      const int n = static_cast<int>(std::min(C, P - first));
      HIP_OK(hipMemcpyAsync(d_in, in.data() + first, static_cast<size_t>(n) * sizeof(int4), hipMemcpyHostToDevice, st_));
      insert_pair_kernel<<<dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st_>>>(
          d_in, n, d_res, d_iv, d_reasons);
      HIP_OK(hipGetLastError());
      HIP_OK(hipMemcpyAsync(result.data() + first, d_res, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost, st_));
    }
    HIP_OK(hipMemcpyAsync(per_iv.data(), d_iv, per_iv.size() * 8, hipMemcpyDeviceToHost, st_));
    HIP_OK(hipMemcpyAsync(reasons.data(), d_reasons, 4 * 8, hipMemcpyDeviceToHost, st_));
    HIP_OK(hipStreamSynchronize(st_));
  }
  st.kept = static_cast<int64_t>(reasons[KEPT]);
  st.same_strand = static_cast<int64_t>(reasons[SAME_STRAND]);
  st.skipped = static_cast<int64_t>(reasons[SKIPPED]);
  st.nonpositive = static_cast<int64_t>(reasons[NONPOSITIVE]);
  if (st.kept + st.same_strand + st.skipped + st.nonpositive != P ||
      std::accumulate(per_iv.begin(), per_iv.end(), 0ull) != reasons[KEPT])
    MISO_FAIL(MISO_EINTERNAL, "insert-length pair pass: counts do not add up");
  // kept pairs by interval (GFF order), then by the left mate's place in the file
  std::vector<int64_t> at(per_iv.size(), 0);
  for (size_t k = 1; k < per_iv.size(); k++) at[k] = at[k - 1] + static_cast<int64_t>(per_iv[k - 1]);
  for (int64_t k = 0; k < P; k++) {
    if (result[k] <= 0) continue;
    const int t = static_cast<int>(static_cast<uint32_t>(in[k].x) & MISO_INSERT_TAG_MASK);
    const int64_t o = at[t]++;
    if (o < cap) { iv_out[o] = t; ins_out[o] = result[k]; }
  }
  st.pairs_ms = ms_since(t0);
  *n_kept = st.kept;
  if (stats) *stats = st;
}

}  // namespace miso
