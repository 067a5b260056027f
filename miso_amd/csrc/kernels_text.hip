// kernels_text.hip -- the sample rows of `.miso` files decoded on the device, straight into a samples batch's pool
// (summarize_miso / compare_miso over existing outputs, packed or not: miso_amd/samples_utils.py, miso_amd/miso_db.py).
//
//   text         event i's body is text[offsets[i] .. offsets[i + 1]): rows "f_1,...,f_K<TAB>g<LF>", empty lines ignored.
//   shape call   host only: isoforms and non-empty lines per event (memchr work on the host threads), so that the caller
//                can group events by sample count.
//   decode pass  the text streams through in chunks of whole events, two in flight on two streams (pinned buffer ->
//                device buffer -> kernels), so device memory is bounded by the chunk size plus the pool.  An event's text
//                is cut into tiles of kBlock x 16 bytes and every tile of the chunk is a workgroup: (1) every thread
//                loads its 16 aligned bytes and marks the non-empty line starts among them, the workgroup counts them;
//                (2) a scan over each event's tiles turns the counts into the row number each tile begins with; (3) the
//                marks again, a workgroup scan, and the thread that owns a line start decodes that row: K psi fields
//                written at row r of the event's off_samples (the file's layout, n_samples rows of K doubles), the log
//                score checked and dropped.  Neighbouring threads own neighbouring rows: a wavefront's loads cover one
//                span of text and its stores one span of the pool.
//   exactness    a psi field of at most 15 significant digits and at most 22 decimals is (double) m / 10^f: m < 2^53 and
//                10^f <= 10^22 are exact doubles, the one division is correctly rounded (no -ffast-math), so the result is
//                the correctly rounded value of the decimal -- what strtod, Python's float() and numpy give.  The sign is
//                applied last ("-0.0000" is -0.0).  Anything else sets the event's status; nothing is guessed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "batch.hpp"
#include "hip_host.hpp"

extern "C" int miso_usable_threads(void);   // alnio.cpp

namespace miso {
namespace {

constexpr int kBlock = 256;
constexpr int kSpan = 16;                        // bytes of text per thread and tile
constexpr int64_t kTile = int64_t{kBlock} * kSpan;
constexpr int64_t kDefaultChunk = int64_t{64} << 20;
constexpr int64_t kPad = 32;                     // the buffers end in padding: aligned 8- and 16-byte loads may overrun the text

__constant__ double kPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                  1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

// the text from `pos` on, one byte at a time out of aligned 8-byte loads; behind `end` it reads as LF
struct Cursor {
  const unsigned char *buf;
  int64_t pos, end;
  uint64_t w;
  __device__ Cursor(const unsigned char *b, int64_t p, int64_t e) : buf(b), pos(p), end(e), w(0) { load(); }
  __device__ void load() { w = *reinterpret_cast<const uint64_t *>(buf + (pos & ~int64_t{7})); }
  __device__ int peek() const { return pos < end ? static_cast<int>((w >> (8 * (pos & 7))) & 0xff) : '\n'; }
  __device__ void next() {
    pos++;
    if ((pos & 7) == 0 && pos < end) load();
  }
};

// -?digits[.digits]: the digits as an integer m (the first 19 significant ones), their number `sig` without leading
// zeros, the digits after the point f.  false: not of that form (the cursor stands where it stopped).
__device__ inline bool plain_decimal(Cursor &c, bool &neg, uint64_t &m, int &sig, int &f) {
  neg = false; m = 0; sig = 0; f = 0;
  if (c.peek() == '-') { neg = true; c.next(); }
  int nd = 0;
  for (int ch = c.peek(); ch >= '0' && ch <= '9'; c.next(), ch = c.peek()) {
    nd++;
    if (sig > 0 || ch != '0') { if (++sig <= 19) m = m * 10 + static_cast<uint64_t>(ch - '0'); }
  }
  if (nd == 0) return false;
  if (c.peek() != '.') return true;
  c.next();
  for (int ch = c.peek(); ch >= '0' && ch <= '9'; c.next(), ch = c.peek()) {
    f++;
    if (sig > 0 || ch != '0') { if (++sig <= 19) m = m * 10 + static_cast<uint64_t>(ch - '0'); }
  }
  return f > 0;
}

__device__ inline bool literal(Cursor &c, char a, char b, char d) {
  if (c.peek() != a) return false;
  c.next();
  if (c.peek() != b) return false;
  c.next();
  if (c.peek() != d) return false;
  c.next();
  return true;
}

// the log-score field: a plain decimal of any length, nan, inf or -inf
__device__ inline bool score_field(Cursor &c) {
  if (c.peek() == 'n') return literal(c, 'n', 'a', 'n');
  if (c.peek() == 'i') return literal(c, 'i', 'n', 'f');
  if (c.peek() == '-') {
    Cursor look = c;
    look.next();
    if (look.peek() == 'i') { c = look; return literal(c, 'i', 'n', 'f'); }
  }
  bool neg; uint64_t m; int sig, f;
  return plain_decimal(c, neg, m, sig, f);
}

// one row from its first byte: K psi values to out[0 .. K), returns the MISO_TEXT_* bits it earned (0: decoded)
__device__ inline int decode_row(Cursor c, int K, double *out) {
  for (int k = 0;; k++) {
    bool neg; uint64_t m; int sig, f;
    if (!plain_decimal(c, neg, m, sig, f) || sig > 15 || f > 22) return MISO_TEXT_EPSI;
    const int ch = c.peek();
    if (ch != ',' && ch != '\t') return ch == '\n' ? MISO_TEXT_EROW : MISO_TEXT_EPSI;   // no TAB | an exponent, a CR, ...
    if (k >= K) return MISO_TEXT_EROW;
    const double v = static_cast<double>(m) / kPow10[f];
    out[k] = neg ? -v : v;
    c.next();
    if (ch == '\t') {
      if (k + 1 != K) return MISO_TEXT_EROW;
      break;
    }
  }
  if (!score_field(c) || c.peek() != '\n') return MISO_TEXT_ESCORE;
  return 0;
}

// A tile is kTile bytes of one event's text, counted from the 16-byte boundary at or before the event's first byte; an
// empty event has one (empty) tile.  The chunk's tiles are numbered event by event: tile_first[i] is the first tile of the
// chunk's event i, tile_first[n] the number of tiles.  Which event owns tile t: the last i with tile_first[i] <= t.
struct TileOf {
  int e;                  // the event, as the batch numbers it
  bool last;              // its last tile
  int64_t begin, end;     // the event's text in buf
  int64_t p0;             // this thread's first byte
};

__device__ inline TileOf tile_of(const int32_t *tile_first, int n, int e0, const int64_t *offsets, int64_t base) {
  const int t = static_cast<int>(blockIdx.x);
  int lo = 0, hi = n;                              // tile_first[lo] <= t < tile_first[hi]
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (tile_first[mid] <= t) lo = mid;
    else hi = mid;
  }
  TileOf w;
  w.e = e0 + lo;
  w.last = t + 1 == tile_first[lo + 1];
  w.begin = offsets[w.e] - base;
  w.end = offsets[w.e + 1] - base;
  w.p0 = (w.begin & ~int64_t{kSpan - 1}) + int64_t{t - tile_first[lo]} * kTile + int64_t{threadIdx.x} * kSpan;
  return w;
}

// bit j: a non-empty line of the event starts at p0 + j
__device__ inline unsigned line_starts(const unsigned char *buf, const TileOf &w) {
  unsigned starts = 0;
  if (w.p0 < w.end) {
    const uint4 v = *reinterpret_cast<const uint4 *>(buf + w.p0);
    const unsigned words[4] = {v.x, v.y, v.z, v.w};
    int prev = w.p0 > w.begin ? buf[w.p0 - 1] : '\n';
#pragma unroll
    for (int j = 0; j < kSpan; j++) {
      const int ch = static_cast<int>((words[j >> 2] >> (8 * (j & 3))) & 0xff);
      const int64_t pos = w.p0 + j;
      if (pos >= w.begin && pos < w.end && ch != '\n' && (pos == w.begin || prev == '\n')) starts |= 1u << j;
      prev = ch;
    }
  }
  return starts;
}

__device__ inline int wave_inclusive_scan(int v) {
  const int lane = static_cast<int>(threadIdx.x) & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(v, d);
    if (lane >= d) v += up;
  }
  return v;
}

// the counts of the threads before this one in the workgroup, and the workgroup's sum
__device__ inline int block_exclusive_scan(int cnt, int *total) {
  __shared__ int wave_sum[kBlock / 64];
  const int lane = static_cast<int>(threadIdx.x) & 63, wave = static_cast<int>(threadIdx.x) >> 6;
  const int incl = wave_inclusive_scan(cnt);
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  int before = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; w++) {
    if (w < wave) before += wave_sum[w];
    sum += wave_sum[w];
  }
  *total = sum;
  return before + incl - cnt;
}

// pass 1, one workgroup per tile: tile_rows[t] = the non-empty lines that start in tile t
__global__ __launch_bounds__(kBlock) void text_count_kernel(const unsigned char *buf, const int64_t *offsets, int64_t base,
                                                           int e0, int n, const int32_t *tile_first, int32_t *tile_rows) {
  const TileOf w = tile_of(tile_first, n, e0, offsets, base);
  int total;
  block_exclusive_scan(__popc(line_starts(buf, w)), &total);
  if (threadIdx.x == 0) tile_rows[blockIdx.x] = total;
}

// pass 2, one wavefront per event: tile_rows[t] becomes the rows of the event that start before tile t
__global__ __launch_bounds__(kBlock) void text_scan_kernel(int n, const int32_t *tile_first, int32_t *tile_rows) {
  const int i = static_cast<int>(blockIdx.x) * (kBlock / 64) + (static_cast<int>(threadIdx.x) >> 6);
  if (i >= n) return;
  const int lane = static_cast<int>(threadIdx.x) & 63;
  int carry = 0;
  for (int t0 = tile_first[i]; t0 < tile_first[i + 1]; t0 += 64) {          // (uniform over the wavefront)
    const int t = t0 + lane;
    const int v = t < tile_first[i + 1] ? tile_rows[t] : 0;
    const int incl = wave_inclusive_scan(v);
    if (t < tile_first[i + 1]) tile_rows[t] = carry + incl - v;
    carry += __shfl(incl, 63);
  }
}

// pass 3, one workgroup per tile: the thread that owns a line start decodes that row.  buf holds the text from absolute
// offset `base` on and ends in kPad bytes of padding; offsets are absolute.  Writes only inside the event's n_samples x K
// pool region; an event's status collects what its tiles found, the last tile adds the row count's verdict.
__global__ __launch_bounds__(kBlock) void text_decode_kernel(const unsigned char *buf, const int64_t *offsets, int64_t base,
                                                            int e0, int n, const int32_t *tile_first,
                                                            const int32_t *tile_rows, const DevEvent *events,
                                                            unsigned char *pool, int S, int32_t *status) {
  const TileOf w = tile_of(tile_first, n, e0, offsets, base);
  const int K = events[w.e].K;
  double *out = reinterpret_cast<double *>(pool + events[w.e].off_samples);
  unsigned starts = line_starts(buf, w);
  int total;
  int r = tile_rows[blockIdx.x] + block_exclusive_scan(__popc(starts), &total);
  int bad = 0;
  while (starts) {
    const int j = __ffs(starts) - 1;
    starts &= starts - 1;
    if (r < S) bad |= decode_row(Cursor(buf, w.p0 + j, w.end), K, out + static_cast<size_t>(r) * K);
    r++;
  }
  if (w.last && threadIdx.x == 0 && tile_rows[blockIdx.x] + total != S) bad |= MISO_TEXT_ECOUNT;
  if (bad) atomicOr(status + w.e, bad);
}

// body(lo, hi) over [0, n) on up to T threads, at least `grain` items each
template <class F> void parallel_for(int64_t n, int T, int64_t grain, F &&body) {
  T = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(T, n / grain + 1)));
  std::vector<std::thread> th;
  for (int t = 1; t < T; t++) th.emplace_back([&, t] { body(n * t / T, n * (t + 1) / T); });
  body(0, n / T);
  for (auto &x : th) x.join();
}

// what the pass allocates beside the batch's own pool, released however it ends
struct Scratch {
  std::vector<void *> dev, pinned;
  std::vector<hipStream_t> streams;
  std::vector<hipEvent_t> events;
  void *alloc(size_t bytes) {
    void *p = nullptr;
    HIP_OK(hipMalloc(&p, std::max<size_t>(bytes, 16)));
    dev.push_back(p);
    return p;
  }
  void *host(size_t bytes) {
    void *p = nullptr;
    HIP_OK(hipHostMalloc(&p, std::max<size_t>(bytes, 16), hipHostMallocDefault));
    pinned.push_back(p);
    return p;
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

void check_offsets(int n, const int64_t *offsets) {
  if (n < 0) MISO_FAIL(MISO_EINVAL, "Invalid number of events");
  if (offsets[0] < 0) MISO_FAIL(MISO_EINVAL, "Text offsets must not be negative");
  for (int i = 0; i < n; i++)
    if (offsets[i + 1] < offsets[i]) MISO_FAIL(MISO_EINVAL, "Text offsets must not decrease");
}

}  // namespace

void text_shape(int n, const unsigned char *text, const int64_t *offsets, int32_t *noiso, int32_t *n_rows) {
  check_offsets(n, offsets);
  parallel_for(n, miso_usable_threads(), 64, [&](int64_t lo, int64_t hi) {
    for (int64_t i = lo; i < hi; i++) {
      const unsigned char *p = text + offsets[i], *end = text + offsets[i + 1];
      int64_t rows = 0;
      int K = 0;
      while (p < end) {
        const unsigned char *lf = static_cast<const unsigned char *>(std::memchr(p, '\n', static_cast<size_t>(end - p)));
        const unsigned char *stop = lf ? lf : end;
        if (stop > p) {
          if (rows++ == 0) {
            const unsigned char *tab = static_cast<const unsigned char *>(std::memchr(p, '\t', static_cast<size_t>(stop - p)));
            K = 1 + static_cast<int>(std::count(p, tab ? tab : stop, static_cast<unsigned char>(',')));
          }
        }
        p = stop + 1;
      }
      noiso[i] = K;
      n_rows[i] = static_cast<int32_t>(std::min<int64_t>(rows, INT32_MAX));
    }
  });
}

}  // namespace miso

using namespace miso;

void miso_batch::adopt_text(int n, const unsigned char *text, const int64_t *offsets, const int *K, int Sn, int dev,
                            int64_t chunk_bytes, int32_t *status, miso_text_stats_t *stats) {
  const auto t_call = std::chrono::steady_clock::now();
  check_offsets(n, offsets);
  adopt_pool(n, K, Sn, dev);                       // (MISO_ENODEVICE without a GPU)
  miso_text_stats_t st{};
  const int64_t C = std::max<int64_t>(chunk_bytes > 0 ? chunk_bytes : kDefaultChunk, 1);
  // chunks of whole events: [first event, one past the last)
  std::vector<std::pair<int, int>> chunks;
  int64_t slot_bytes = 0, slot_tiles = 0;
  int slot_events = 0;
  // an event's tiles, its text standing at `rel` in the chunk's buffer (kernels: tile_of)
  auto tiles_of = [&](int e, int64_t rel) {
    const int64_t span = rel + (offsets[e + 1] - offsets[e]) - (rel & ~int64_t{kSpan - 1});
    return std::max<int64_t>(1, (span + kTile - 1) / kTile);
  };
  for (int e = 0; e < n;) {
    int last = e + 1;
    while (last < n && offsets[last + 1] - offsets[e] <= C) last++;
    int64_t tiles = 0;
    for (int i = e; i < last; i++) {
      if (offsets[i + 1] - offsets[i] > INT32_MAX) MISO_FAIL(MISO_EINVAL, "An event's text is too long (2 GiB at most)");
      tiles += tiles_of(i, offsets[i] - offsets[e]);
    }
    if (tiles > INT32_MAX) MISO_FAIL(MISO_EINVAL, "chunk_bytes is too large");
    slot_bytes = std::max(slot_bytes, offsets[last] - offsets[e]);
    slot_tiles = std::max(slot_tiles, tiles);
    slot_events = std::max(slot_events, last - e);
    chunks.emplace_back(e, last);
    e = last;
  }

  Scratch s;
  int32_t *d_status = static_cast<int32_t *>(s.alloc(static_cast<size_t>(n) * 4));
  int64_t *d_offsets = static_cast<int64_t *>(s.alloc((static_cast<size_t>(n) + 1) * 8));
  HIP_OK(hipMemcpy(d_offsets, offsets, (static_cast<size_t>(n) + 1) * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(d_status, 0, std::max<size_t>(static_cast<size_t>(n) * 4, 16)));
  HIP_OK(hipMemset(d_out, 0, out_bytes));     // (the padding between regions, and what an undecoded event leaves)
  HIP_OK(hipStreamSynchronize(nullptr));      // (the chunk streams do not wait for the null stream)

  // a slot: the chunk's text, the first tile of each of its events, the rows per tile (then: before each tile)
  struct Slot { unsigned char *h, *d; int32_t *h_first, *d_first, *d_rows; hipStream_t st; hipEvent_t e0, ek, e1; bool busy; };
  Slot slot[2];
  const size_t n_slots = chunks.size() > 1 ? 2 : 1;
  for (size_t i = 0; i < n_slots; i++) {
    Slot &q = slot[i];
    q.h = static_cast<unsigned char *>(s.host(static_cast<size_t>(slot_bytes + kPad)));
    q.d = static_cast<unsigned char *>(s.alloc(static_cast<size_t>(slot_bytes + kPad)));
    q.h_first = static_cast<int32_t *>(s.host((static_cast<size_t>(slot_events) + 1) * 4));
    q.d_first = static_cast<int32_t *>(s.alloc((static_cast<size_t>(slot_events) + 1) * 4));
    q.d_rows = static_cast<int32_t *>(s.alloc(static_cast<size_t>(slot_tiles) * 4));
    q.st = s.stream(); q.e0 = s.event(); q.ek = s.event(); q.e1 = s.event(); q.busy = false;
  }
  auto drain = [&](Slot &q) {
    HIP_OK(hipStreamSynchronize(q.st));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, q.ek, q.e1));
    st.kernel_ms += ms;
    HIP_OK(hipEventElapsedTime(&ms, q.e0, q.e1));
    st.decode_ms += ms;
    q.busy = false;
  };
  const int T = std::min(miso_usable_threads(), 16);
  for (size_t ci = 0; ci < chunks.size(); ci++) {
    Slot &q = slot[ci % n_slots];
    if (q.busy) drain(q);
    const int e0 = chunks[ci].first, e1 = chunks[ci].second;
    const int64_t base = offsets[e0], bytes = offsets[e1] - base;
    parallel_for(bytes, T, int64_t{1} << 20, [&](int64_t lo, int64_t hi) {
      std::memcpy(q.h + lo, text + base + lo, static_cast<size_t>(hi - lo));
    });
    std::memset(q.h + bytes, '\n', kPad);
    const int nc = e1 - e0;
    q.h_first[0] = 0;
    for (int i = 0; i < nc; i++)
      q.h_first[i + 1] = q.h_first[i] + static_cast<int32_t>(tiles_of(e0 + i, offsets[e0 + i] - base));
    const unsigned tiles = static_cast<unsigned>(q.h_first[nc]);
    HIP_OK(hipEventRecord(q.e0, q.st));
    HIP_OK(hipMemcpyAsync(q.d, q.h, static_cast<size_t>(bytes + kPad), hipMemcpyHostToDevice, q.st));
    HIP_OK(hipMemcpyAsync(q.d_first, q.h_first, (static_cast<size_t>(nc) + 1) * 4, hipMemcpyHostToDevice, q.st));
    HIP_OK(hipEventRecord(q.ek, q.st));
    text_count_kernel<<<dim3(tiles), dim3(kBlock), 0, q.st>>>(q.d, d_offsets, base, e0, nc, q.d_first, q.d_rows);
    HIP_OK(hipGetLastError());
    text_scan_kernel<<<dim3(static_cast<unsigned>((nc + kBlock / 64 - 1) / (kBlock / 64))), dim3(kBlock), 0, q.st>>>(
        nc, q.d_first, q.d_rows);
    HIP_OK(hipGetLastError());
    text_decode_kernel<<<dim3(tiles), dim3(kBlock), 0, q.st>>>(q.d, d_offsets, base, e0, nc, q.d_first, q.d_rows, d_events,
                                                              d_out, Sn, d_status);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(q.e1, q.st));
    q.busy = true;
    st.text_bytes += bytes;
  }
  for (size_t i = 0; i < n_slots; i++)
    if (slot[i].busy) drain(slot[i]);
  if (n) HIP_OK(hipMemcpy(status, d_status, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost));
  text_status.assign(status, status + n);       // (compare_pairs: such an event's columns are not finite)
  for (int i = 0; i < n; i++) {
    if (status[i] == 0) { st.decoded++; st.sample_bytes += int64_t{8} * Sn * K[i]; }
    else st.not_decoded++;
  }
  st.chunks = static_cast<int64_t>(chunks.size());
  st.total_ms = ms_since(t_call);
  if (stats) *stats = st;
}
