// runtime.hip -- batch object: host packing -> HBM pools -> the plan of a launch -> results (the launches themselves, which
// follow that plan: launch.hip).
//
// One batch = the events one GPU samples in one go (the unit the reference hands to one worker
// process, misopy/miso.py:165-187).  All events of a batch share the sampler parameters
// (run_miso.py:68-73 passes the same settings for every event of a run).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>

#include "batch.hpp"
#include "column_pass.hpp"
#include "compare_column.hpp"
#include "compare_pairs.hpp"
#include "coop.hpp"
#include "exact_compare.hpp"
#include "exact_delta.hpp"
#include "hip_host.hpp"

namespace miso {

extern int g_hw_queues_in_effect;   // capi.hip: the host's hardware queue count as the runtime read (or will read) it, 0 = unknown

__global__ void compare_kernel(const DevEvent *, const unsigned char *, const DevEvent *, const unsigned char *, int, int,
                               double, const uint64_t *, double *);
__global__ void compare_pairs_kernel(const DevEvent *, const unsigned char *, int, const DevEvent *, const unsigned char *, int, int,
                                     PairsArgs, int, const uint64_t *, uint64_t *);
__global__ void match_kernel(const MatchEvent *, const int2 *, const int *, const int *, const int *, const int *,
                             const int *, const int *, const int *, int, int, int, int, int, uint32_t *, uint16_t *);
__global__ void summarize_kernel(const DevEvent *, const unsigned char *, int, int, int, int, const uint64_t *, double *, int);
__global__ void diagnose_kernel(const DevEvent *, const unsigned char *, int, int, int, int, double, int, const uint64_t *, double *);
__global__ void diagnose_rank_kernel(const DevEvent *, const unsigned char *, int, int, int, int, int, int, int, double, const uint64_t *,
                                     double *);
__global__ void selftest_detmath_kernel(const double *, int, double *, double *, double *, double *);
__global__ void selftest_philox_kernel(const uint32_t *, int, uint32_t *);


int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void set_device(int d) { HIP_OK(hipSetDevice(d)); }


// Lanes per chain for sampler_k2.  Measured on MI355X (profiles/r01_k2_phase_cycles.txt): the
// kernel is VALU-issue bound at two resident wavefronts per SIMD; the per-iteration scalar MH
// step costs a wavefront ~9k cycles whatever G is, so fewer lanes per chain (more chains sharing
// it) is better -- until the wavefronts no longer fit the device's resident slots and a second,
// mostly empty round starts.  Hence: the smallest supported G whose wavefront count still fills
// the slots once, i.e. the largest G with ceil(chains / (64 / G)) <= slots; G = 1 for batches that
// overflow anyway; never more lanes than a chain has pairs of draw quads to stride over.

int choose_lanes_per_chain(long chains, int max_quads, int wave_slots, int max_cpw) {
  static const int kG[] = {64, 32, 21, 16, 12, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1};
  const int cap = std::max(1, max_quads / 2);
  const bool pow2_only = max_cpw < 64;   // paired-end reduces three values per step: measured, the
  int last = 64;                         // shuffle-loop reduction of odd group sizes does not pay
  for (int G : kG) {
    const int cpw = 64 / G;
    if (cpw > max_cpw) break;            // paired-end: per-chain LDS tables bound the chains per wave
    if (pow2_only && (G & (G - 1))) continue;
    last = G;
    if (G > cap) continue;
    if ((chains + cpw - 1) / cpw <= wave_slots) return G;
  }
  return last;
}

}  // namespace miso

using namespace miso;

bool miso_batch::coop_enabled() const { return !no_coop && !knobs.no_coop; }

void miso_batch::release() {
  if (device >= 0) (void) hipSetDevice(device);
  if (d_events) (void) hipFree(d_events);
  if (d_in) (void) hipFree(d_in);
  if (d_out) (void) hipFree(d_out);
  if (d_fp) (void) hipFree(d_fp);
  if (d_slots) (void) hipFree(d_slots);
  d_slots = nullptr;
  // (the next upload may be to another device: nothing may outlive its allocation as a stale pointer or a cached plan)
  each_table([](auto &t) { t.reset(); });
  k2_pair_grid = k2_pair_wide_blocks = 0;
  k2[0].plan_key = k2[1].plan_key = -1;
  if (probe_stream) { (void) hipStreamSynchronize(probe_stream); (void) hipStreamDestroy(probe_stream); probe_stream = nullptr; }
  if (d_probe) { (void) hipFree(d_probe); d_probe = nullptr; }
  probe_armed = false;
  if (ev0) (void) hipEventDestroy(ev0);
  if (ev1) (void) hipEventDestroy(ev1);
  for (hipStream_t st : aux_streams) (void) hipStreamDestroy(st);
  for (hipEvent_t e : aux_done) (void) hipEventDestroy(e);
  aux_streams.clear(); aux_done.clear();
  if (stream) (void) hipStreamDestroy(stream);
  d_events = nullptr; d_in = d_out = nullptr; d_fp = nullptr; ev0 = ev1 = nullptr; stream = nullptr;
  uploaded = launched = downloaded = false;
}

// Row f1: the compatibility of every pending event's reads with its isoforms, in one launch.
// Inputs: the genes' exon tables and the host-parsed CIGAR blocks; outputs: u32 masks (single-end)
// or u16 fragment indices (paired-end), from which the events are packed exactly as the host path
// packs them (the same pack_event, fed with the match matrix those outputs stand for).
void miso_batch::resolve_pending() {
  if (pending.empty()) return;
  knobs = Knobs::from_env();
  const bool timing = knobs.timing;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double>(b - a).count(); };
  const auto T0 = now();
  const int n = static_cast<int>(pending.size());
  const bool pe = p.paired != 0;
  const int mates = pe ? 2 : 1;
  const int ov = p.overHang == 0 ? 1 : p.overHang;
  std::vector<MatchEvent> mev(n);
  std::vector<int2> blocks;
  std::vector<int> h_exidx, h_exstart, h_exend, h_pos, h_opidx, h_ops, h_len;
  // offsets first, then the copies in parallel
  std::vector<size_t> o_xi(n + 1, 0), o_ex(n + 1, 0), o_rd(n + 1, 0), o_op(n + 1, 0), o_out(n + 1, 0);
  std::vector<size_t> frag_off(n, 0);
  size_t out_frags = 0;
  for (int i = 0; i < n; i++) {
    const Pending &q = pending[i];
    const int N = events[q.event].N;
    const size_t K = static_cast<size_t>(q.gene.K);
    o_xi[i + 1] = o_xi[i] + q.gene.exidx.size();
    o_ex[i + 1] = o_ex[i] + q.gene.exstart.size();
    o_rd[i + 1] = o_rd[i] + static_cast<size_t>(mates) * N;
    o_op[i + 1] = o_op[i] + q.ct.ops.size();
    // frags[(out_off + r) * K + k]: out_off in units of the event's own K, so round up
    const size_t slot = pe ? (out_frags + K - 1) / K : o_out[i];
    frag_off[i] = slot * K;
    if (pe) out_frags = frag_off[i] + static_cast<size_t>(N) * K;
    o_out[i + 1] = o_out[i] + static_cast<size_t>(N) * (pe ? 1 : (K + 31) / 32);   // single-end masks: (K + 31) / 32 words per read
    MatchEvent &m = mev[i];
    m.K = q.gene.K; m.n_reads = N;
    m.exidx_off = static_cast<int32_t>(o_xi[i]); m.ex_off = static_cast<int32_t>(o_ex[i]);
    m.read_off = static_cast<int32_t>(o_rd[i]); m.out_off = static_cast<int32_t>(slot);
    for (int r0 = 0; r0 < N; r0 += 256) blocks.push_back(make_int2(i, r0));
  }
  if (o_op[n] > 0x7FFFFFF0u || o_rd[n] > 0x7FFFFFF0u || out_frags > 0x7FFFFFF0u)
    MISO_FAIL(MISO_EINVAL, "Batch too large for one match launch");
  const size_t out_slots = o_out[n];
  h_exidx.resize(o_xi[n]); h_exstart.resize(o_ex[n]); h_exend.resize(o_ex[n]);
  h_pos.resize(o_rd[n]); h_len.resize(o_rd[n]); h_opidx.resize(o_rd[n] + 1); h_ops.resize(o_op[n]);
  const int nthreads = std::max(1, std::min<int>(16, static_cast<int>(std::thread::hardware_concurrency())));
  auto parallel = [&](auto &&fn) {
    std::vector<std::thread> pool;
    for (int t = 1; t < nthreads; t++) pool.emplace_back([&fn, t] { fn(t); });
    fn(0);
    for (auto &th : pool) th.join();
  };
  parallel([&](int t) {
    for (int i = t; i < n; i += nthreads) {
      const Pending &q = pending[i];
      std::copy(q.gene.exidx.begin(), q.gene.exidx.end(), h_exidx.begin() + o_xi[i]);
      std::copy(q.gene.exstart.begin(), q.gene.exstart.end(), h_exstart.begin() + o_ex[i]);
      std::copy(q.gene.exend.begin(), q.gene.exend.end(), h_exend.begin() + o_ex[i]);
      std::copy(q.pos.begin(), q.pos.end(), h_pos.begin() + o_rd[i]);
      std::copy(q.ct.len.begin(), q.ct.len.end(), h_len.begin() + o_rd[i]);
      std::copy(q.ct.ops.begin(), q.ct.ops.end(), h_ops.begin() + o_op[i]);
      const int base = static_cast<int>(o_op[i]);
      const size_t nr = o_rd[i + 1] - o_rd[i];
      for (size_t r = 0; r < nr; r++) h_opidx[o_rd[i] + r] = base + q.ct.idx[r];
    }
  });
  h_opidx[o_rd[n]] = static_cast<int>(o_op[n]);
  const auto T1 = now();
  std::vector<uint32_t> h_masks(pe ? 0 : out_slots);
  std::vector<uint16_t> h_frags(pe ? out_frags : 0);
  if (!blocks.empty()) {
    auto up = [&](const void *src, size_t bytes) {
      void *d = nullptr;
      HIP_OK(hipMalloc(&d, std::max<size_t>(bytes, 16)));
      if (bytes) HIP_OK(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
      return d;
    };
    void *d_ev = up(mev.data(), mev.size() * sizeof(MatchEvent));
    void *d_bl = up(blocks.data(), blocks.size() * sizeof(int2));
    void *d_xi = up(h_exidx.data(), h_exidx.size() * 4), *d_xs = up(h_exstart.data(), h_exstart.size() * 4);
    void *d_xe = up(h_exend.data(), h_exend.size() * 4), *d_po = up(h_pos.data(), h_pos.size() * 4);
    void *d_oi = up(h_opidx.data(), h_opidx.size() * 4), *d_op = up(h_ops.data(), h_ops.size() * 4);
    void *d_le = up(h_len.data(), h_len.size() * 4);
    void *d_out = nullptr;
    const size_t out_bytes_m = pe ? h_frags.size() * 2 : h_masks.size() * 4;
    HIP_OK(hipMalloc(&d_out, std::max<size_t>(out_bytes_m, 16)));
    hipEvent_t t0, t1;
    HIP_OK(hipEventCreate(&t0)); HIP_OK(hipEventCreate(&t1));
    HIP_OK(hipEventRecord(t0, nullptr));
    hipLaunchKernelGGL(match_kernel, dim3(static_cast<unsigned>(blocks.size())), dim3(256), 0, nullptr,
                       static_cast<const MatchEvent *>(d_ev), static_cast<const int2 *>(d_bl),
                       static_cast<const int *>(d_xi), static_cast<const int *>(d_xs),
                       static_cast<const int *>(d_xe), static_cast<const int *>(d_po),
                       static_cast<const int *>(d_oi), static_cast<const int *>(d_op),
                       static_cast<const int *>(d_le), p.readLength, ov, pe ? 1 : 0, fd.start,
                       static_cast<int>(fd.prob.size()), static_cast<uint32_t *>(d_out),
                       static_cast<uint16_t *>(d_out));
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(t1, nullptr));
    HIP_OK(hipMemcpy(pe ? static_cast<void *>(h_frags.data()) : static_cast<void *>(h_masks.data()), d_out,
                     out_bytes_m, hipMemcpyDeviceToHost));
    HIP_OK(hipEventElapsedTime(&match_ms, t0, t1));
    (void) hipEventDestroy(t0); (void) hipEventDestroy(t1);
    for (void *d : {d_ev, d_bl, d_xi, d_xs, d_xe, d_po, d_oi, d_op, d_le, d_out}) (void) hipFree(d);
  }
  const auto T2 = now();
  if (p.want_counts_trace) { kept_masks.resize(events.size()); kept_frags.resize(events.size()); }
  // pack on the host cores (a few, the cgroup may allow far fewer than the machine has)
  std::vector<std::string> errors(nthreads);
  std::vector<int> codes(nthreads, 0);
  parallel([&](int t) {
    try {
      for (int i = t; i < n; i += nthreads) {
        const Pending &q = pending[i];
        const int K = q.gene.K, N = mev[i].n_reads;
        const uint32_t *mk32 = pe ? nullptr : h_masks.data() + mev[i].out_off;
        const uint16_t *f = pe ? h_frags.data() + frag_off[i] : nullptr;
        const int W = (K + 63) / 64, W32 = (K + 31) / 32;   // mask words per read: 64-bit on the host, 32-bit from the kernel
        std::vector<uint64_t> pm(static_cast<size_t>(std::max(N, 1)) * W, 0u);
        if (pe) {   // a pair's mask = the isoforms with a fragment length inside the distribution
          for (int r = 0; r < N; r++)
            for (int k = 0; k < K; k++) if (f[static_cast<size_t>(r) * K + k] != FRAG_NONE) pm[static_cast<size_t>(r) * W + (k >> 6)] |= 1ull << (k & 63);
        } else {
          for (int r = 0; r < N; r++)
            for (int w = 0; w < W32; w++) pm[static_cast<size_t>(r) * W + (w >> 1)] |= static_cast<uint64_t>(mk32[static_cast<size_t>(W32) * r + w]) << (32 * (w & 1));
        }
        const uint64_t *mk = pm.data();
        if (p.want_counts_trace) {
          if (pe) kept_frags[q.event].assign(f, f + static_cast<size_t>(N) * K);
          else kept_masks[q.event].assign(mk, mk + static_cast<size_t>(N) * W);
        }
        events[q.event] = pack_event_masks(p, pe ? &fd : nullptr, K, N, mk, f, nullptr, q.gene.isolen.data(),
                                           q.gene.noexons.data(), q.hyper.empty() ? nullptr : q.hyper.data(), W);
        attach_gene_classes(events[q.event], p, q.gene);   // algorithm = CLASSES only
      }
    } catch (const Error &e) { codes[t] = e.code; errors[t] = e.text;
    } catch (const std::bad_alloc &) { codes[t] = MISO_ENOMEM; errors[t] = "Error at runtime.hip:0: allocation failed, Out of memory";
    } catch (const std::exception &e) {   // nothing may leave a worker thread (std::terminate)
      codes[t] = MISO_EINTERNAL; errors[t] = std::string("Error at runtime.hip:0: ") + e.what() + ", Internal error";
    } catch (...) { codes[t] = MISO_EINTERNAL; errors[t] = "Error at runtime.hip:0: unknown exception, Internal error"; }
  });
  for (int t = 0; t < nthreads; t++) if (codes[t]) throw Error(codes[t], errors[t], Error::Formatted{});
  pending.clear();
  if (timing)
    std::fprintf(stderr, "[miso] resolve: flatten %.3f s, device (alloc+copies+kernel %.3f ms) %.3f s, pack (%d threads) %.3f s\n",
                 secs(T0, T1), match_ms, secs(T1, T2), nthreads, secs(T2, now()));
}


void miso_batch::upload(int dev) {
  if (uploaded && dev == device) return;
  if (uploaded) release();
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device: the sampler has no CPU path");
  device = dev;
  HIP_OK(hipSetDevice(dev));
  knobs = Knobs::from_env();
  resolve_pending();
  {   // the reference's proposal density overflows beyond about 85 isoforms (miso.c:97-122: linear domain):
      // such a chain accepts its first proposal and nothing after -- bit-equal to the reference, not a posterior
    int wide = 0, kmax = 0;
    for (const PackedEvent &e : events) if (e.K > 80) { wide++; kmax = std::max(kmax, e.K); }
    if (wide > 0 && !knobs.quiet)
      std::fprintf(stderr, "[miso] warning: %d gene(s) of more than 80 isoforms (up to %d): as in the reference, the proposal density "
                           "(miso.c:97-122, linear domain) overflows beyond about 85 isoforms and the chains stop accepting after "
                           "their first iteration; the samples equal the reference's and are not a posterior\n", wide, kmax);
  }
  const int n = static_cast<int>(events.size());
  const int C = p.noChains, M = p.noIterations, Sn = S();
  h_events.assign(n, DevEvent{});
  uint64_t in_off = 0, out_off = 0;
  for (int i = 0; i < n; i++) {
    const PackedEvent &e = events[i];
    DevEvent &d = h_events[i];
    d.K = e.K; d.n_draw = e.n_draw; d.n_reads = e.N; d.base_bad = e.base_bad;
    d.base_sfix = e.base_sfix;
    if (i < static_cast<int>(event_ids.size()) && event_ids[i] >= 0) {
      d.has_id = 1; d.explicit_id = static_cast<uint32_t>(event_ids[i]);
    }
    d.off_consts = in_off; in_off = align_up(in_off + e.consts.size() * 8, 16);
    d.off_base = in_off; in_off = align_up(in_off + e.base_count.size() * 4, 16);
    d.off_draw = in_off;   // (single-end: the masks' low words, whole quads; from 33 isoforms on the high words behind them)
    in_off = align_up(in_off + (e.paired ? e.draw_frag.size() * 2
                                         : align_up(e.draw_mask.size(), 4) * 4 * ((e.K + 31) / 32)), 16);   // one plane of whole quads per 32 isoforms
    d.n_dcls = static_cast<int32_t>(e.dcls_mask.size());
    d.n_units = e.n_units;
    d.max_cls = e.max_cls_size;
    d.n_pairs = static_cast<int32_t>(e.dcls_pairs.size());
    d.off_cls = in_off; in_off = align_up(in_off + e.dcls_tab.size() * 4, 16);
    d.off_clsmask = in_off; in_off = align_up(in_off + e.dcls_pairs.size() * 2, 16);
    d.off_units = in_off; in_off = align_up(in_off + e.unit_desc.size() * 4, 16);
    d.off_sfix = in_off; in_off = align_up(in_off + e.sfix_table.size() * 4, 16);
    d.pe_delta = e.pe_delta ? 1 : 0;
    d.dense_nobad = e.dense_nobad ? 1 : 0;
    d.off_dense = d.off_sfixd = NO_DENSE;
    if (!e.draw_dense.empty()) {
      d.off_dense = in_off; in_off = align_up(in_off + e.draw_dense.size() * 2, 16);
      d.off_sfixd = in_off; in_off = align_up(in_off + e.sfix_dense.size() * 4, 16);
    }
    d.n_mcls = static_cast<int32_t>(e.mcls_tab.size() / (e.K + 1));
    d.off_mcls = in_off; in_off = align_up(in_off + e.mcls_tab.size() * 8, 16);
    d.off_samples = out_off; out_off = align_up(out_off + static_cast<uint64_t>(Sn) * e.K * 8, 16);
    d.off_loglik = out_off; out_off = align_up(out_off + static_cast<uint64_t>(Sn) * 8, 16);
    d.off_drawass = out_off; out_off = align_up(out_off + static_cast<uint64_t>(e.n_draw), 16);
    d.off_stats = out_off; out_off = align_up(out_off + sizeof(ChainStats) * C, 16);
    if (p.want_counts_trace) {
      d.off_trace = out_off;
      out_off = align_up(out_off + static_cast<uint64_t>(M + 1) * C * e.K * 4, 16);
    } else {
      d.off_trace = NO_TRACE;
    }
  }
  in_bytes = std::max<uint64_t>(in_off, 16);
  out_bytes = std::max<uint64_t>(out_off, 16);
  std::vector<unsigned char> h_in(in_bytes, 0);
  for (int i = 0; i < n; i++) {
    const PackedEvent &e = events[i];
    const DevEvent &d = h_events[i];
    std::memcpy(h_in.data() + d.off_consts, e.consts.data(), e.consts.size() * 8);
    std::memcpy(h_in.data() + d.off_base, e.base_count.data(), e.base_count.size() * 4);
    if (e.paired) std::memcpy(h_in.data() + d.off_draw, e.draw_frag.data(), e.draw_frag.size() * 2);
    else {
      // plane w = bits 32 w .. 32 w + 31 of every draw's mask, each plane whole quads long
      uint32_t *pl = reinterpret_cast<uint32_t *>(h_in.data() + d.off_draw);
      const size_t npad = align_up(e.draw_mask.size(), 4), nd = e.draw_mask.size();
      const int W32 = (e.K + 31) / 32, Wx = (e.K + 63) / 64 - 1;
      for (size_t r = 0; r < nd; r++)
        for (int w = 0; w < W32; w++) {
          const uint64_t word = (w < 2) ? e.draw_mask[r] : e.draw_mask_x[r * Wx + (w >> 1) - 1];
          pl[npad * w + r] = static_cast<uint32_t>(word >> (32 * (w & 1)));
        }
    }
    if (!e.unit_desc.empty()) std::memcpy(h_in.data() + d.off_units, e.unit_desc.data(), e.unit_desc.size() * 4);
    if (!e.dcls_tab.empty()) {
      std::memcpy(h_in.data() + d.off_cls, e.dcls_tab.data(), e.dcls_tab.size() * 4);
      if (!e.dcls_pairs.empty())
        std::memcpy(h_in.data() + d.off_clsmask, e.dcls_pairs.data(), e.dcls_pairs.size() * 2);
    }
    if (!e.mcls_tab.empty()) std::memcpy(h_in.data() + d.off_mcls, e.mcls_tab.data(), e.mcls_tab.size() * 8);
    if (!e.sfix_table.empty())
      std::memcpy(h_in.data() + d.off_sfix, e.sfix_table.data(), e.sfix_table.size() * 4);
    if (!e.draw_dense.empty()) {
      std::memcpy(h_in.data() + d.off_dense, e.draw_dense.data(), e.draw_dense.size() * 2);
      std::memcpy(h_in.data() + d.off_sfixd, e.sfix_dense.data(), e.sfix_dense.size() * 4);
    }
  }
  {
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, dev));
    wave_slots = prop.multiProcessorCount * 4 * 2;  // CUs x SIMDs x resident sampler_k2 waves
    if (knobs.wave_slots.set) wave_slots = knobs.wave_slots.v;
  }
  {
    // The batch's own stream carries its FIRST kernel -- the longest-running class of a whole-gene batch (runs are
    // launched heaviest class first) -- at the highest queue priority; the kernels beside it go to streams of falling
    // priority (launch: stream_for_next), so that whenever a slot frees up the dispatcher takes a workgroup of the longest
    // class still waiting: longest first ACROSS the classes without one kernel holding all their bodies (that kernel was
    // built: 28 minutes of compilation, 800 spilled registers -- tools/experiments/grp_all/).  MEASURED, round 5, and OFF
    // unless knobs.stream_prio: 16 384 genes of 3 - 20 isoforms x 1000 pairs 922 ms with against 917 ms without, hg19-like
    // pair counts 958 against 865 ms (the chains on several workgroups sit in the high-priority kernel and everything else
    // waits behind them) -- profiles/r05_stream_priorities.txt.
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { lo = hi = 0; (void) hipGetLastError(); }
    prio_lo = lo; prio_hi = knobs.stream_prio.on() ? hi : lo;
    if (prio_hi != prio_lo) HIP_OK(hipStreamCreateWithPriority(&stream, hipStreamDefault, prio_hi));
    else HIP_OK(hipStreamCreate(&stream));
  }
  HIP_OK(hipEventCreate(&ev0));
  HIP_OK(hipEventCreate(&ev1));
  HIP_OK(hipMalloc(reinterpret_cast<void **>(&d_events), std::max<size_t>(n, 1) * sizeof(DevEvent)));
  HIP_OK(hipMalloc(reinterpret_cast<void **>(&d_in), in_bytes));
  HIP_OK(hipMalloc(reinterpret_cast<void **>(&d_out), out_bytes));
  if (n) HIP_OK(hipMemcpy(d_events, h_events.data(), n * sizeof(DevEvent), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_in, h_in.data(), in_bytes, hipMemcpyHostToDevice));
  build_slots();
  if (p.paired) {
    HIP_OK(hipMalloc(reinterpret_cast<void **>(&d_fp), fd.prob.size() * 8));
    HIP_OK(hipMemcpy(d_fp, fd.prob.data(), fd.prob.size() * 8, hipMemcpyHostToDevice));
  }
  uploaded = true;
  pool_cleared = false; launched_once = false;
}

// The launch lists of the uploaded events: [two-isoform events | the other events by class | the exact mode's events].
// Made by upload(), and again by launch() when miso_batch_set_exact was called in between.
void miso_batch::build_slots() {
  const int n = static_cast<int>(events.size());
  // launch lists: two-isoform events (single- or paired-end) go to sampler_k2, ordered by their
  // number of drawing reads so the chains sharing a wavefront loop equally long
  // (paired-end with a fragment-length distribution so wide that one chain's tables do not fit a CU's LDS -- sd beyond
  // ~400 -- : the two-isoform events take the general kernel, whose tables may stay in global memory, like the
  // reference, which takes any sd, miso_paired.c:299-308; or knobs.k2_general)
  k2_general = p.paired && (48 * fd.prob.size() + 64 > 150 * 1024 || knobs.k2_general);
  // (the exact-posterior mode, miso_batch_set_exact: its eligible events leave both lists for one of their own)
  std::vector<int32_t> two, gen, ex;
  is_exact.assign(n, 0);
  if (exact && !p.paired && p.algorithm == MISO_ALGO_REASSIGN)
    for (int i = 0; i < n; i++) {
      if (events[i].K != 2) continue;
      // (every single-end event is packed with its effective lengths, host.cpp pack_event_masks: one without them came
      // by a route that forgot them, and must not fall back to the sampler in silence)
      if (events[i].eff.size() != 2 || events[i].hyper.size() != 2)
        MISO_FAIL(MISO_EINTERNAL, "exact-posterior mode: a two-isoform event was packed without its effective lengths");
      is_exact[i] = exact_eligible(false, 2, events[i].eff.data(), events[i].hyper.data());
    }
  // (the paired-end mode, miso_batch_set_exact_paired: A0, A1 in the place of the effective lengths; no pair of the event
  // on a non-finite score entry -- base_bad the fixed pairs, pe_delta the drawing ones; the batch's smallest
  // fragment-length probability at least 2^-63, so that sixteen factors multiply to a normal number; indices in 16 bits)
  if (exact_paired && p.paired && p.algorithm == MISO_ALGO_REASSIGN) {
    double fp_min = 1.0;
    for (double v : fd.prob) fp_min = std::min(fp_min, v);
    const bool batch_ok = !fd.prob.empty() && fp_min >= EXACT_PAIRED_MIN_PROB && fd.prob.size() <= 0xFFFFu;
    for (int i = 0; i < n && batch_ok; i++) {
      if (events[i].K != 2) continue;
      if (events[i].eff.size() != 2 || events[i].hyper.size() != 2)
        MISO_FAIL(MISO_EINTERNAL, "paired exact-posterior mode: a two-isoform event was packed without its A0, A1");
      is_exact[i] = exact_paired_eligible(2, events[i].eff.data(), events[i].hyper.data(), events[i].base_bad != 0 || !events[i].pe_delta);
    }
  }
  for (int i = 0; i < n; i++) (is_exact[i] ? ex : (events[i].K == 2 && !k2_general) ? two : gen).push_back(i);
  // (paired-end: the events sampler_k2's MODE 2 can take come first)
  use_delta = !knobs.no_pe_delta;   // fixed here: the slot order depends on it
  // (Round 5 tried ordering a collapsed batch's list by the binomial's likely regime -- inversion below n min(p, q) = 10, BTRS
  // above: a wavefront that holds chains of both runs both -- and measured nothing once the inversion had lost its division:
  // 50.3 - 50.8 ms against 50.1 - 50.6 ms, profiles/r05_sampler_lane_ilp.txt.)
  std::stable_sort(two.begin(), two.end(), [&](int x, int y) {
    const bool dx = k2_mode2(events[x]), dy = k2_mode2(events[y]);
    return dx != dy ? dx : events[x].n_draw > events[y].n_draw; });
  n_k2w = 0;
  for (int i : two) n_k2w += k2_mode2(events[i]) ? 1 : 0;
  // the general kernel's wavefronts loop to their largest K and longest draw list: group alike.
  // Paired-end (sampler_grp gives every chain of a launch the same lanes): genes of very different sizes -- real
  // read counts, 20 ... 10^5 pairs per gene; the reference costs O(reads) per gene, miso_paired.c:393-552 -- are
  // split into size buckets per isoform-count class, each its own launch beside the others.  How many lanes a gene
  // needs follows from its SHARE of the batch's work (drawing quads x isoforms): the batch takes W / (lanes of the
  // device) at best, a chain on L lanes w / L, and a chain should be done in half of that -- L >= 2 x device lanes x
  // w / W.  Up to 1.5 x the rule's 16 lanes: the class's normal launch; up to 64: at least 32 lanes; up to 256: a
  // wavefront of its own (sampler_grp<64, true, KC>); beyond: one chain per workgroup (256 lanes, kernels_grp.inl WIDE
  // -- its four wavefronts each repeat the chain's Metropolis-Hastings step, so only where the read loop dominates);
  // beyond 384: several workgroups (coop.hpp), one per 256 lanes needed.  Never more lanes than the gene has pairs of
  // quads.  Thresholds measured: profiles/r03_pe_buckets.txt (knobs.no_pe_buckets, pe_t_wave, pe_t_wide).
  // (64: 33 ... MISO_MAX_ISOFORMS isoforms -- sampler_wave only, lane k = isoform k; the reference has no limit, miso.c:696)
  // (256: 65 ... MISO_MAX_ISOFORMS isoforms -- sampler_big, the chain's vectors in LDS, kernels_big.hip)
  auto kc_of = [](int K) { return K <= 4 ? 4 : (K <= 8 ? 8 : (K <= 12 ? 12 : (K <= 16 ? 16 : (K <= 32 ? 32 : (K <= 64 ? 64 : 256))))); };
  std::vector<Bucket> bucket(n, Bucket::Normal);   // (Workgroup: on coop_n[event] workgroups)
  coop_n.assign(n, 1);
  if (p.paired && !knobs.no_pe_buckets) {
    double W = 0;
    for (int i : gen) W += static_cast<double>((events[i].n_draw + 3) / 4) * events[i].K;
    const double device_lanes = 2048.0 * 64.0;
    const double share_factor = knobs.pe_share.v, t_wave = knobs.pe_t_wave.v, t_wide = knobs.pe_t_wide.v;
    const bool dense_ok = !knobs.no_pe_dense;
    const bool coop_on = coop_enabled();
    // "at least 32 lanes" from a need of 24 lanes in a batch with a heavy tail (some gene needs a wavefront or more), from 32
    // in a batch of like-sized genes, where a 20-isoform gene of 1000 pairs needs 28 by the share rule and runs better on
    // 16 (round 5, 16 384 genes of 3 - 20 isoforms: 1000 pairs each 920 -> 863 ms with 32, hg19-like pair counts 830 -> 927 ms;
    // profiles/r05_pe_mix_lanes.txt)
    double max_need = 0.0;
    for (int i : gen) max_need = std::max(max_need, W > 0 ? share_factor * device_lanes * (static_cast<double>((events[i].n_draw + 3) / 4) * events[i].K) / W : 0.0);
    const double t_32 = knobs.pe_t_32.set ? knobs.pe_t_32.v : (max_need > t_wave ? 24.0 : 32.0);
    for (int i : gen) {
      const PackedEvent &e = events[i];
      const int nq = (e.n_draw + 3) / 4;
      const double need = W > 0 ? share_factor * device_lanes * (static_cast<double>(nq) * e.K) / W : 0.0;
      const bool can_wide = dense_ok && !e.draw_dense.empty() && e.K >= 3 && e.K <= PE_DENSE_KMAX;
      if (can_wide && need > t_wide && nq >= 512) {
        bucket[i] = Bucket::Workgroup;
        if (coop_on && need > 384.0)
          coop_n[i] = std::max(1, std::min({COOP_MAX_N, static_cast<int>(std::ceil(need / 256.0)), nq / 512}));
      } else if (can_wide && need > t_wave && nq >= 128) bucket[i] = Bucket::Wavefront;
      else if (need > t_32 && nq >= 64) bucket[i] = Bucket::Lanes32;
    }
    // (round 6) ... and the SMALL genes of a batch of several classes: eight lanes per chain -- a gene of a hundred pairs is all
    // scalar step, which eight chains of a wavefront share instead of four (16 384 genes of 3 - 8 isoforms x 100 / 250 / 500 pairs:
    // 198.5 -> 147.4, 237.3 -> 190.3, 306.2 -> 291.8 ms; profiles/r06_small_genes.txt).
    const int t_small = knobs.pe_t_small.v;
    bool classes2 = false;
    for (int i : gen) classes2 |= kc_of(events[i].K) != kc_of(events[gen[0]].K);
    if (classes2 && t_small > 0 && dense_ok)
      for (int i : gen) {
        const PackedEvent &e = events[i];
        if (bucket[i] == Bucket::Normal && !e.draw_dense.empty() && e.K >= 3 && e.K <= PE_DENSE_KMAX && (e.n_draw + 3) / 4 <= t_small) bucket[i] = Bucket::Small;
      }
  }
  std::stable_sort(gen.begin(), gen.end(), [&](int x, int y) {
    const int kx = kc_of(events[x].K), ky = kc_of(events[y].K);
    if (kx != ky) return kx > ky;
    if (bucket[x] != bucket[y]) return bucket[x] > bucket[y];
    return events[x].K != events[y].K ? events[x].K > events[y].K : events[x].n_draw > events[y].n_draw; });
  gen_runs.clear(); tuned_k2_G = 0; k2[0].plan_key = k2[1].plan_key = -1;
  for (size_t j = 0; j < gen.size(); j++) {
    const PackedEvent &e = events[gen[j]];
    const int kc = kc_of(e.K);
    if (gen_runs.empty() || gen_runs.back().kc != kc || gen_runs.back().bucket != bucket[gen[j]]) {
      GenRun r; r.first = static_cast<int>(j); r.kc = kc; r.bucket = bucket[gen[j]];
      gen_runs.push_back(std::move(r));
    }
    GenRun &r = gen_runs.back();
    r.count++;
    r.kmax = std::max(r.kmax, e.K);
    r.kmin = std::min(r.kmin, e.K);
    r.maxq = std::max(r.maxq, (e.n_draw + 3) / 4);
    r.sum_q += (e.n_draw + 3) / 4;
    r.maxcls = std::max(r.maxcls, static_cast<int>(e.dcls_mask.size()));
    if (!e.paired && e.n_draw > 0 && e.dcls_mask.empty()) r.nocls = true;
    if (!e.paired || e.draw_dense.empty() || e.K == 2) r.dense = false;   // (K = 2: draw_dense holds sampler_k2's records)
  }
  n_k2 = static_cast<int>(two.size()); n_gen = static_cast<int>(gen.size());
  n_exact = static_cast<int>(ex.size());
  k2[0].mode = 2; k2[0].first = 0; k2[0].count = n_k2w;
  k2[1].mode = p.paired ? 1 : 0; k2[1].first = n_k2w; k2[1].count = n_k2 - n_k2w;
  h_slots = two;
  h_slots.insert(h_slots.end(), gen.begin(), gen.end());
  h_slots.insert(h_slots.end(), ex.begin(), ex.end());
  std::vector<double> eff2;
  for (int i : ex) { eff2.push_back(events[i].eff[0]); eff2.push_back(events[i].eff[1]); }
  put(exact_eff, eff2);
  slots_exact = exact_any(); exact_sums.clear(); exact_sums_level = -1.0;
  if (!d_slots) HIP_OK(hipMalloc(reinterpret_cast<void **>(&d_slots), std::max<size_t>(n, 1) * sizeof(int32_t)));
  if (n) HIP_OK(hipMemcpy(d_slots, h_slots.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
}


// ---- launch(): plan the two-isoform part, plan the general runs, group them into launches, launch ----
void miso_batch::launch(uint64_t seed, uint32_t first_event_id) {
  if (!uploaded) MISO_FAIL(MISO_EINVAL, "batch not uploaded");
  HIP_OK(hipSetDevice(device));
  knobs = Knobs::from_env();
  if (slots_exact != exact_any()) {   // miso_batch_set_exact / _paired after the upload: the launch lists anew
    HIP_OK(hipStreamSynchronize(stream));
    for (GenRun &r : gen_runs) { r.wave_tab.reset(); r.coop.reset(); }
    build_slots();
  }
  const int n = static_cast<int>(events.size());
  KernelArgs a{};
  a.events = d_events; a.in_pool = d_in; a.out_pool = d_out; a.frag_prob = d_fp;
  a.il = static_cast<int>(fd.prob.size()); a.n_events = n;
  a.C = p.noChains; a.M = p.noIterations; a.B = p.noBurnIn; a.lag = p.noLag;
  a.start = p.start; a.first_event_id = first_event_id; a.seed = seed;
  a.balance = knobs.prio_quartiles.on() ? 2 : 0;   // device.hpp prio_by_progress
  a.wide_dedup = knobs.k2_wide_dedup.off() ? 0 : 1;
  a.round_tab = nullptr;
  if (!round_starts.empty()) {   // a later round of stop = CONVERGENT_MEAN (converge_rounds): where the rounds after the first open
    std::vector<int32_t> tab(MISO_MAX_ROUNDS);
    for (int i = 0; i < MISO_MAX_ROUNDS; i++) tab[i] = i < static_cast<int>(round_starts.size()) ? round_starts[i] : -1;
    put(round_tab, tab);
    a.round_tab = round_tab.d;
  }
  last_seed = seed; last_first_event_id = first_event_id;
  converged_done = false;
  if (probe_armed) { HIP_OK(hipStreamSynchronize(probe_stream)); probe_armed = false; }   // (a launch nobody waited for)
  a.k2_full_math = knobs.k2_full_math;
  if (knobs.coop_max_polls.set) a.coop_max_polls = static_cast<uint32_t>(knobs.coop_max_polls.v);
  // (one word, two readers: the general paired-end kernels' exact scan, the two-isoform kernels' rescan -- device.hpp)
  a.pe_force_exact = knobs.pe_force_exact;
  KernelArgs k2a = a;                    // what the two-isoform part is planned and launched with
  k2a.pe_force_exact = knobs.k2_settle_all;
  // Trailing sample columns stay 0 (miso.c:661, quirk C8) -- they exist only when the lag does not divide the kept
  // iterations; otherwise the kernels overwrite every sample, log score, pick and statistic of the pool, and clearing
  // 4.8 GB per launch (0.75 ms of the headline's 102 ms step) is for the first launch only.
  if (!pool_cleared || (p.noIterations - p.noBurnIn) % p.noLag != 0 || p.want_counts_trace) {
    HIP_OK(hipMemsetAsync(d_out, 0, out_bytes, stream));
    pool_cleared = true;
  }
  lanes_per_chain = 0;
  last_kernels.clear(); trial_launch = false;
  if (!launched_once) coop_wgs_used = 0;
  plan = LaunchPlan{};
  kernel_no = 0;
  // algorithm = MARGINAL / CLASSES (miso.c:272-295, 788-808): Metropolis-Hastings on psi alone, no reads to reassign
  const bool marginal = !p.paired && (p.algorithm == MISO_ALGO_MARGINAL || p.algorithm == MISO_ALGO_CLASSES);
  if (!marginal) {
    plan_sizes();
    plan_k2(k2a);
    plan_runs(a);
    group_runs();
    plan.sampled = true;
  }
  HIP_OK(hipEventRecord(ev0, stream));                  // events bracket the sampler kernels only
  if (marginal) {
    launch_marginal(a);
  } else {
    launch_planned(a, k2a);
    if (n_exact > 0) launch_exact(a);
  }
  // kernel i > 0 went to its own stream, forked from the batch's stream: joined back into it
  for (size_t i = 1; i < kernel_no && i <= aux_streams.size() && !knobs.serial_kernels; i++) {
    HIP_OK(hipEventRecord(aux_done[i - 1], aux_streams[i - 1]));
    HIP_OK(hipStreamWaitEvent(stream, aux_done[i - 1], 0));
  }
  HIP_OK(hipEventRecord(ev1, stream));
  start_clock_probe();
  launched = true; launched_once = true; downloaded = false; summarized = false; compared = false; exact_compared = false; pairs_compared = false; diagnosed = false; rank_diagnosed = false;
}

// The launch's sizes and switches, read once per launch.
void miso_batch::plan_sizes() {
  LaunchPlan &q = plan;
  // a workgroup may use half of the CU's 160 KB of LDS (two workgroups per CU)
  // (knobs.lds_max_kb: a larger cap lets one workgroup per CU hold more chains per wavefront)
  q.lds_max = knobs.lds_max_kb.v * 1024;
  const int il = static_cast<int>(fd.prob.size());
  K2Half &w = k2[0], &r = k2[1];
  for (K2Half *h : {&w, &r}) { h->kind = K2Kernel::None; h->G = 0; }
  r.fp = p.paired ? align_up(fd.prob.size() * 8, 16) : 0;
  r.tab = p.paired ? 2 * fd.prob.size() * 4 : 0;   // per chain: int32[2 x il]
  // paired-end: the first n_k2w slots go to MODE 2 (no drawing read with a non-finite score), the rest to
  // MODE 1; single-end: everything is "the rest".  Both keep the event's score table (2 il int32) per chain in LDS.
  // MODE 2 reads the dense records (device.hpp pe_k2_entries): both tables with 2 il + 2 entries
  w.fp = p.paired ? align_up(static_cast<size_t>(pe_k2_entries(il)) * 8, 16) : 0;
  w.tab = p.paired ? static_cast<size_t>(pe_k2_entries(il)) * 4 : 0;
  q.fp_plain = p.paired ? align_up(fd.prob.size() * 8, 16) : 0;
  // paired-end dense path (pe_dense): byte records, the probability table with its two extra entries, the
  // score table with rows of il + 2
  q.dense_env = !knobs.no_pe_dense;
  q.il2 = pe_dense_il2(il);
  // A batch with several kernels (two-isoform events + one general kernel per isoform-count class)
  // runs them CONCURRENTLY, one stream each: every kernel then only has its share of the device to
  // fill, so the lanes-per-chain rule sees `wave_slots x share` (one after the other, each class of
  // a whole-gene batch -- a few thousand chains -- would be spread thin over 32 lanes per chain and
  // still leave the GPU half empty).
  q.total_chains = static_cast<long>(n_k2 + n_gen) * p.noChains;   // (the exact mode's events are not the samplers')
  q.n_kernels = (r.count > 0 ? 1 : 0) + (w.count > 0 ? 1 : 0) + gen_runs.size();
  // Lanes per chain, measured: the best split depends on how the batch's wavefronts fill the SIMDs
  // (chains, isoforms, reads, LDS per workgroup), so the first launch of a large single-end batch
  // with more than two isoforms times a few iterations of the rule of thumb's choice and of the next
  // larger ones on the batch itself and keeps the fastest (K=5: 58k -> 81k events/s) (the trial launches record nothing: burn-in = their length; what they leave in the
  // output pool is rewritten by the real launch).
  const bool tune = !knobs.no_autotune && p.noIterations >= 2000;   // ~400 trial iterations: <= 20 % of a one-shot run
  q.tune_runs = tune && q.n_kernels <= 1;   // trial launches would time a kernel alone
  // (workgroup-wide chains may use several workgroups, coop.hpp)
  q.coop_max = coop_enabled() ? COOP_MAX_N : 1;
}

int miso_batch::slots_for(long chains) const {
  if (plan.n_kernels <= 1 || plan.total_chains <= 0) return wave_slots;
  return std::max(1, static_cast<int>(static_cast<double>(wave_slots) * chains / plan.total_chains));
}

// Trial launches: the candidate whose per-iteration cost is lowest -- the slope between a short and a longer trial
// (set-up, launch and code-object load cancel); ~200 iterations per candidate
template <class F> int miso_batch::fastest(const KernelArgs &a, const std::vector<int> &cand, F &&trial) {
  auto timed = [&](int iters, int g) {
    KernelArgs t = a;
    t.M = iters; t.B = iters;
    float ms = 0;
    HIP_OK(hipEventRecord(ev0, stream));
    trial_launch = true;   // (launch_kernel: not into last_kernels)
    trial(t, g);
    trial_launch = false;
    HIP_OK(hipEventRecord(ev1, stream));
    HIP_OK(hipEventSynchronize(ev1));
    HIP_OK(hipEventElapsedTime(&ms, ev0, ev1));
    return ms;
  };
  int best = cand[0]; float best_slope = 0;
  for (size_t i = 0; i < cand.size(); i++) {
    timed(4, cand[i]);
    const float t0 = timed(32, cand[i]), t1 = timed(160, cand[i]);
    const float slope = t1 - t0;
    if (i == 0 || slope < best_slope) { best = cand[i]; best_slope = slope; }
  }
  return best;
}

// ---- the two-isoform part: sampler_k2<G> and its relatives ----
// lanes per chain a run of sampler_k2_multi may have: single-end, paired-end
static constexpr int K2_WIDTHS_SE[] = {1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 32, 64}, K2_WIDTHS_PE[] = {4, 8, 16, 32, 64};

// plan_lanes for a part of the two-isoform list (batch.hpp K2Part) under this launch's knobs: knobs.k2_target forces the
// bound on a wavefront's step
LanePlan miso_batch::k2_lanes(const K2Part &pt, const std::vector<int> &nd, const LaneCost &cost) const {
  return plan_lanes(nd.data(), pt.count, p.noChains, pt.widths, pt.n_widths, pt.wide_wpb, pt.wpb, pt.resident, pt.max_cpw, cost,
                    knobs.k2_target.v, plan.coop_max, pt.coop_budget);
}

// The lane plan of one half into `h.plan`, unless it still holds the one made for the same key: the resident workgroups, the
// chains and the cooperative budget.  A knob the key does not carry (knobs.replan_k2(), the caller's `forced`) plans anew
// at every launch.  `cost`: the part's cost model, here overridden by knobs.k2_cost and knobs.coop_min_quads.  True when
// it planned: `nd` then holds the slots' drawing reads, for what the caller plans further.
bool miso_batch::plan_k2_lanes(const K2Part &pt, bool forced, LaneCost &cost, std::vector<int> &nd, K2Half &h) {
  const long key = (static_cast<long>(pt.resident) * 64 + p.noChains) * 256 + pt.coop_budget + (plan.coop_max > 1 ? 0 : 200);
  if (h.plan_key == key && !forced && !knobs.replan_k2()) return false;
  double *const c[5] = {&cost.block, &cost.step[1], &cost.step[2], &cost.step[3], &cost.step[4]};
  for (size_t i = 0; i < knobs.k2_cost.size(); i++) *c[i] = knobs.k2_cost[i];
  if (knobs.coop_min_quads.set) cost.coop_min_quads = knobs.coop_min_quads.v;
  nd.resize(pt.count);
  for (int i = 0; i < pt.count; i++) nd[i] = events[h_slots[pt.first + i]].n_draw;
  h.plan = k2_lanes(pt, nd, cost);
  h.plan_key = key;
  return true;
}

void miso_batch::plan_k2(const KernelArgs &a) {
  LaunchPlan &q = plan;
  K2Half &w = k2[0], &r = k2[1];   // MODE 2; the others
  const size_t LDS_MAX = q.lds_max;
  // (only when the batch's wavefronts fit the resident slots once: with several rounds the hardware hands
  // out workgroups as slots free up, heaviest first, and the 4-wavefront workgroups balance better --
  // MISO defaults, 6 chains x 40 000 events at one lane per chain: 374 ms paired, 351 ms unpaired)
  q.k2_pair = !p.paired && !knobs.k2_pair.off();
  if (r.count > 0) {
    const long chains = static_cast<long>(r.count) * p.noChains;
    const int maxq = p.paired ? (events[k2_first_event()].n_draw + 3) / 4 : (events[k2_first_event()].n_draw + 7) / 8;   // Philox blocks
    const int max_cpw = p.paired ? std::max<int>(1, static_cast<int>((60 * 1024 - r.fp) / (4 * r.tab))) : 64;
    if (knobs.lanes_per_chain.set) r.G = knobs.lanes_per_chain.v;
    else if (tuned_k2_G) r.G = tuned_k2_G;
    else {
      r.G = choose_lanes_per_chain(chains, maxq, slots_for(chains), max_cpw);
      if (q.tune_runs && chains >= 4096 && knobs.autotune_k2) {   // the rule is the measured optimum
        static const int kG[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 21, 32, 64};
        std::vector<int> cand{r.G};
        for (int i = 0; i < 15; i++)
          if (kG[i] == r.G) {
            for (int j : {i - 1, i + 1, i + 2})
              if (j >= 0 && j < 15 && 64 / kG[j] <= max_cpw && !(p.paired && (kG[j] & (kG[j] - 1))) &&
                  kG[j] <= std::max(1, maxq))
                cand.push_back(kG[j]);
          }
        if (cand.size() > 1) r.G = fastest(a, cand, [&](const KernelArgs &t, int g) { launch_k2(t, r, g, stream); });
        tuned_k2_G = r.G;
      }
    }
  }
  if (w.count > 0) {   // MODE 2: two workgroups per CU may share the LDS (80 KB each)
    const long chains = static_cast<long>(w.count) * p.noChains;
    const int maxq = (events[k2_first_event()].n_draw + 3) / 4;
    const long lds_left = static_cast<long>(LDS_MAX) - static_cast<long>(w.fp);
    const int max_cpw = static_cast<int>(std::max<long>(1, lds_left / static_cast<long>(4 * w.tab)));
    if (knobs.lanes_per_chain.set) {
      w.G = knobs.lanes_per_chain.v;
      if (w.G < 1 || w.G > 64) MISO_FAIL(MISO_EINVAL, "MISO_LANES_PER_CHAIN must be one of 1-10,12,16,21,32,64");
    } else w.G = choose_lanes_per_chain(chains, maxq, slots_for(chains), max_cpw);
    while (w.G < 64 && static_cast<size_t>(64 / w.G) > static_cast<size_t>(max_cpw)) w.G *= 2;   // a forced choice never exceeds the LDS
  }
  if (q.k2_pair && r.G > 0) {
    const long waves = (static_cast<long>(r.count) * p.noChains + 64 / r.G - 1) / (64 / r.G);
    q.k2_pair = waves <= wave_slots || knobs.k2_pair.set;
  }
  // ---- single-end two-isoform events in one launch with two lane widths (sampler_k2_mix, kernels_k2.hip) ----
  // Only when the batch runs as ONE round of paired 8-wavefront workgroups (k2_pair) that does not fill the CUs:
  // the heaviest events get G + 1 lanes per chain, as many of them as still leave one CU per workgroup.
  // (knobs.k2_mix switches it off, knobs.k2_split forces the number of events of the wide part.)
  {
    const int count = r.count, C = p.noChains, G = r.G;
    if (!p.paired && q.k2_pair && count > 0 && G >= 1 && G <= 7 && q.n_kernels <= 1 && !knobs.k2_mix.off()) {
      const int cus = wave_slots / 8, cpwA = 64 / (G + 1), cpwB = 64 / G;
      auto blocks = [&](long chains, int cpw) { return static_cast<int>(((chains + cpw - 1) / cpw + 7) / 8); };
      auto total = [&](int y) { return blocks(static_cast<long>(y) * C, cpwA) + blocks(static_cast<long>(count - y) * C, cpwB); };
      if (total(0) < cus && blocks(static_cast<long>(count) * C, cpwB) * 8 >= wave_slots / 2) {
        int y = 0;
        if (knobs.k2_split.set) y = std::max(0, std::min(count - 1, knobs.k2_split.v));
        else {
          int lo = 0, hi = count - 1;          // total(y) grows with y: the largest y that still fits
          while (lo < hi) { const int mid = (lo + hi + 1) / 2; if (total(mid) <= cus) lo = mid; else hi = mid - 1; }
          y = lo;
        }
        if (y > 0 && total(y) <= cus) { q.k2_mix = y; q.k2_mix_blocks = blocks(static_cast<long>(y) * C, cpwA); }
      }
    }
  }

  // ---- single-end two-isoform events: a lane width per event (sampler_k2_multi, kernels_k2m.hip) ----
  // Default for single-end batches; knobs.k2_multi off or a forced knobs.lanes_per_chain: the single-width / two-width
  // launches above.  The plan depends on the list, the chains and this kernel's share of the device only: made once per
  // upload (plan_k2_lanes).
  const int coop_max = q.coop_max;
  // All cooperative workgroups of ONE launch() -- the gene runs' (wide_setup) and the two-isoform plans' -- come out of one
  // budget of COOP_MAX_WGS (coop.hpp): the gene runs take what upload() asked for, at most 5/8 when two-isoform events are
  // in the batch too; the MODE 2 plan gets two thirds of the rest when both two-isoform kernels run, the other plan the
  // remainder.  (Single-end batches have one cooperative user, the two-isoform plan: all of it.)
  int coop_k2_budget = COOP_MAX_WGS, coop_k2w_budget = COOP_MAX_WGS;
  {
    long want = 0;
    for (int i = 0; i < n_gen; i++) { const int ev_i = h_slots[n_k2 + i]; if (coop_n[ev_i] > 1) want += static_cast<long>(coop_n[ev_i]) * p.noChains; }
    if (knobs.coop_draws.set && p.paired && n_gen > 0) want = COOP_MAX_WGS;   // (the table decides chain by chain)
    const long cap = n_k2 > 0 ? COOP_MAX_WGS * 5 / 8 : COOP_MAX_WGS;
    coop_gen_budget = coop_max > 1 ? static_cast<int>(std::min(want, cap)) : 0;
    const int left = COOP_MAX_WGS - coop_gen_budget;
    coop_k2w_budget = (w.count > 0 && r.count > 0) ? left * 2 / 3 : left;
    coop_k2_budget = w.count > 0 ? left - coop_k2w_budget : left;
    if (!p.paired) coop_k2_budget = left;
  }
  q.lane_route = collapsed && !p.paired && n_k2 > 0;   // miso_batch_set_collapsed
  // lanes per chain of the collapsed step: one (sampler_lane).  Sharing a chain between 2, 4 or 8 lanes (sampler_k2c:
  // the Metropolis-Hastings step's transcendentals one per lane, the binomial's rejection trials G at a time) brings more
  // wavefronts but the same instructions per wavefront -- 40 000 chains: 56.4 ms on one lane, 58.5 / 59.1 / 86.3 ms on
  // 2 / 4 / 8 (profiles/r03_collapsed.txt); knobs.collapsed_lanes forces
  if (q.lane_route && knobs.collapsed_lanes.set) {
    const int g = knobs.collapsed_lanes.v;
    if (g == 1 || g == 2 || g == 4 || g == 8) q.lane_G = g;
  }
  // one chain per lane, up to two wavefronts per SIMD: the form that overlaps a chain's own work (kernels_lane.hip
  // sampler_lane_ilp); beyond, the lean one (six wavefronts per SIMD hide each other's latencies); knobs.lane_ilp forces.
  if (q.lane_route && q.lane_G == 1) {
    q.lane_ilp = ((static_cast<long>(n_k2) * p.noChains + 255) / 256) * 4 <= wave_slots;
    if (knobs.lane_ilp.set) q.lane_ilp = knobs.lane_ilp.v != 0;
  }
  const bool multi = !knobs.lanes_per_chain.set && !knobs.k2_multi.off();
  bool r_multi = false, w_multi = false;   // sampler_k2_multi for the half
  std::vector<int> nd;
  // ---- paired-end: both halves likewise (sampler_k2_multi<1, 4>, <2, 4>), 4-wavefront workgroups, 4 ... 64 lanes per chain
  // as far as the chains' score tables fit the workgroup's LDS, 256 lanes (the workgroup) for the largest events ----
  for (K2Half *h : {&r, &w}) {
    if (!p.paired || h->count <= 0 || !multi) continue;
    const bool mode2 = h == &w;
    const long lds_left = static_cast<long>(LDS_MAX) - static_cast<long>(h->fp) - K2_RED_BYTES;
    const int max_cpw = static_cast<int>(std::max<long>(0, lds_left / static_cast<long>(4 * h->tab)));
    if (max_cpw < 1) continue;
    K2Part pt{h->first, h->count, K2_WIDTHS_PE, 5};
    pt.wide_wpb = pt.wpb = 4; pt.max_cpw = max_cpw; pt.coop_budget = mode2 ? coop_k2w_budget : coop_k2_budget;
    pt.resident = std::max(1, slots_for(static_cast<long>(h->count) * p.noChains) / 4);
    LaneCost cost = k2_cost_paired();
    if (plan_k2_lanes(pt, mode2 && knobs.k2w_wpb.set, cost, nd, *h) && mode2) {
      // The widest a chain can be is its workgroup: 256 lanes with 4 wavefronts, 512 with 8 (one workgroup per CU,
      // twice the LDS each: the same chains per CU).  8-wavefront workgroups lose ~19 % when the launch runs in
      // several rounds (a workgroup starts when ALL its slots are free), so they are taken only when the largest
      // events would otherwise outlast the launch (hg19-like read counts: 218 ms -> 175 ms; uniform: 217 ms -> 259 ms, not taken; profiles/r03_pe_k2_wpb.txt).
      pt.wide_wpb = pt.wpb = 8; pt.resident = std::max(1, pt.resident / 2);
      const LanePlan p8 = k2_lanes(pt, nd, cost);
      if (knobs.k2w_wpb.set ? knobs.k2w_wpb.v == 8 : 1.2 * p8.est < w.plan.est) w.plan = p8;
    }
    (mode2 ? w_multi : r_multi) = h->plan.n_segs > 0;
  }
  if (!p.paired && r.count > 0 && multi) {
    K2Part pt{r.first, r.count, K2_WIDTHS_SE, 12};
    pt.wide_wpb = pt.wpb = 8; pt.max_cpw = 64; pt.coop_budget = coop_k2_budget;
    pt.resident = std::max(1, slots_for(static_cast<long>(r.count) * p.noChains) / 8);
    LaneCost cost = k2_cost_single();
    if (knobs.k2_wpb.set && knobs.k2_wpb.v != 8 && knobs.k2_wpb.v != 4 && knobs.k2_wpb.v != 1) MISO_FAIL(MISO_EINVAL, "MISO_K2_WPB must be 8, 4 or 1");
    if (plan_k2_lanes(pt, knobs.k2_wpb.set, cost, nd, r)) {
      // several rounds: smaller workgroups (a workgroup starts when ALL its wavefronts' slots are free; with 8 the
      // slots of early finishers idle: MISO defaults on 40 000 events 425 ms, with 4: see profiles/r03_k2_multi_ab.txt)
      const int wpb = knobs.k2_wpb.set ? knobs.k2_wpb.v : (r.plan.rounds == 1 ? 8 : 4);
      if (wpb != 8) {
        pt.wide_wpb = wpb >= 4 ? wpb : 0; pt.wpb = wpb; pt.resident = pt.resident * 8 / wpb;
        r.plan = k2_lanes(pt, nd, cost);
      }
      k2_pair_grid = 0; k2_pair_wide_blocks = 0;
      if (wpb == 8) k2_pair_table(nd, cost);
    }
    r_multi = r.plan.n_segs > 0;
  }
  // the several-rounds single-end plan has runs of one and two lanes per chain only: the kernel of three wavefronts per SIMD (kernels_k2m.inl)
  q.k2_narrow = r_multi && !p.paired && r.plan.wpb == 4 && r.plan.n_segs > 0 && !knobs.k2_no_narrow;
  for (int i = 0; i < r.plan.n_segs && q.k2_narrow; i++) q.k2_narrow = r.plan.seg_lanes[i] <= 2;
  // the halves' kernels: decided here, read by the launch, the names and the statistics (launch.hip)
  if (w.count > 0) w.kind = w_multi ? K2Kernel::Multi : K2Kernel::Single;
  if (r.count > 0) r.kind = q.lane_route ? K2Kernel::Lane : r_multi ? K2Kernel::Multi : q.k2_mix > 0 ? K2Kernel::Mix : K2Kernel::Single;
}

// One round, 8 wavefronts per workgroup: wavefronts w and w + 4 of a workgroup share a SIMD.  Pair the launch's
// wavefronts (all runs but the workgroup-wide chains') by estimated duration, the i-th heaviest with the i-th
// lightest ACROSS the runs: within a run the p-th heaviest + p-th lightest (a.pair_waves) give every SIMD of the
// run the same work, but the runs' sums differ (a run's first wavefront sits at the planner's bound, its last
// wherever the next width takes over) and the SIMDs of the lighter runs idle at the end (wave-slot occupancy
// 0.78, profiles/r03_wave_time.txt).  Measured, 40 000 events: hg19-like read counts (13 runs) 73.9 -> 71.4 ms;
// 1000 reads each (4 runs) 99.7 -> 100.8 ms, 3000 reads 244.6 -> 250.0 ms (few runs: their sums are close already,
// and the kernel with a body per run AND per wavefront is larger): used from seven runs on (knobs.k2_global_pair).
void miso_batch::k2_pair_table(const std::vector<int> &nd, const LaneCost &cost) {
  const LanePlan &pl = k2[1].plan;
  const Opt<int> &gp = knobs.k2_global_pair;
  if (!(pl.n_segs > 0 && pl.rounds == 1 && (gp.set ? gp.v != 0 : pl.n_segs >= 7))) return;
  struct W { double cost; int32_t code; };
  std::vector<W> ws;
  bool ok = true, seen_narrow = false;
  for (int sg = 0; sg < pl.n_segs && ok; sg++) {
    const int G = pl.seg_lanes[sg];
    if (G == K2_WIDE) { ok = !seen_narrow; k2_pair_wide_blocks = pl.seg_block[sg + 1]; continue; }   // (wide runs come first)
    seen_narrow = true;
    const int cpw = 64 / G;
    const long chains = static_cast<long>(pl.seg_slot[sg + 1] - pl.seg_slot[sg]) * p.noChains;
    const long waves = (chains + cpw - 1) / cpw;
    ok = waves < (1L << 20) && sg < 2048;
    for (long w = 0; w < waves && ok; w++) {
      const int first = nd[pl.seg_slot[sg] + static_cast<int>((w * cpw) / p.noChains)];   // the wavefront's longest chain
      ws.push_back(W{cost.wave_step(G, first), static_cast<int32_t>(sg << 20 | static_cast<int32_t>(w))});
    }
  }
  if (!ok || ws.empty()) return;
  std::stable_sort(ws.begin(), ws.end(), [](const W &x, const W &y) { return x.cost > y.cost; });
  const size_t N = ws.size(), Q = (N + 1) / 2, blocks = (Q + 3) / 4;
  std::vector<int32_t> tab(blocks * 8, -1);
  for (size_t q = 0; q < Q; q++) {
    tab[(q / 4) * 8 + q % 4] = ws[q].code;
    if (N - 1 - q > q) tab[(q / 4) * 8 + q % 4 + 4] = ws[N - 1 - q].code;
  }
  k2_pair_grid = k2_pair_wide_blocks + static_cast<int>(blocks);
  put(k2_pair_tab, tab);
}


// ---- more than two isoforms: sampler_grp<G, PE, KC> per isoform-count class ----
int miso_batch::fp_rows(const GenRun &run) const { return (p.paired && plan.dense_env && run.dense) ? 1 : 0; }
size_t miso_batch::fp_bytes_of(const GenRun &run) const {
  return fp_rows(run) ? align_up(static_cast<size_t>(plan.il2) * 8, 16) : plan.fp_plain;
}
GrpShape miso_batch::grp_shape(const GenRun &run) const {
  const size_t fp_bytes = fp_bytes_of(run);
  // single-end: per-class thresholds join the slice (class path) when every event has a class table
  int qs = (!p.paired && !knobs.no_class_path && !run.nocls && run.maxcls > 0) ? run.maxcls : 0;
  if (qs && 4 * 2 * static_cast<size_t>(grp_slice_bytes(run.kmax, qs, 0)) > plan.lds_max) qs = 0;
  // paired-end: the per-event score table (K x il int32) joins the slice when >= 4 chains still fit
  int ts = p.paired ? run.kmax * (fp_rows(run) ? plan.il2 : static_cast<int>(fd.prob.size())) : 0;
  if (ts && fp_bytes + 4 * 4 * static_cast<size_t>(grp_slice_bytes(run.kmax, 0, ts)) > plan.lds_max) ts = 0;
  return GrpShape{qs, ts};
}
bool miso_batch::grp_fits(const GenRun &run, const GrpShape &sh, int G) const {
  const size_t fp_bytes = fp_bytes_of(run);
  return G >= 2 && G <= 32 && !(G & (G - 1)) &&
         fp_bytes + 4 * static_cast<size_t>(64 / G) * grp_slice_bytes(run.kmax, sh.qs, sh.ts) <= plan.lds_max;
}
// runs [r0, r1) (consecutive in the list) as one
miso_batch::GenRun miso_batch::joined_run(size_t r0, size_t r1) const {
  GenRun m;
  m.first = gen_runs[r0].first; m.count = 0; m.kc = gen_runs[r0].kc;
  for (size_t ri = r0; ri < r1; ri++) {
    const GenRun &run = gen_runs[ri];
    m.count += run.count; m.kmax = std::max(m.kmax, run.kmax); m.kmin = std::min(m.kmin, run.kmin); m.maxq = std::max(m.maxq, run.maxq);
    m.maxcls = std::max(m.maxcls, run.maxcls); m.nocls = m.nocls || run.nocls; m.dense = m.dense && run.dense;
  }
  return m;
}


// ---- the general runs: sampler_lane_k, sampler_flat or sampler_grp, and the lanes per chain ----
void miso_batch::plan_runs(const KernelArgs &a) {
  LaunchPlan &q = plan;
  q.runs.assign(gen_runs.size(), LaunchPlan::Run{});
  // collapsed single-end batches (miso_batch_set_collapsed): the events with three and more isoforms in ONE launch of
  // sampler_lane_k (kernels_lane.hip), provided every one of them has its class table
  // (level 2 only: with the classes of a five- or ten-isoform event sharing ~1000 reads the chains of small binomials
  // cost more than the read sweep they replace -- profiles/r03_collapsed.txt; it pays from ~10^4 reads per event)
  // The route is decided per run: a class whose events all have their class tables takes sampler_lane_k, a
  // run without them -- or of 33 isoforms and more: several mask words, sampler_wave / sampler_big only -- keeps the
  // per-read kernels: its events are sampled per read, i.e. equal the CPU checker's COUNTER mode
  // (tests/test_gpu_collapsed.py).
  if (collapsed && collapsed_level >= 2 && !p.paired && n_gen > 0)
    for (size_t ri = 0; ri < gen_runs.size(); ri++) {
      if (gen_runs[ri].nocls || gen_runs[ri].kc >= 64) continue;
      q.runs[ri].kind = q.runs[ri].layout = RunKernel::LaneK;
      q.lane_gen = true;
    }
  for (size_t ri = 0; ri < gen_runs.size(); ri++) plan_flat(ri);
  for (size_t ri = 0; ri < gen_runs.size(); ri++) plan_grp(ri, a);
  // the runs' own kernels: decided here, read by the launch, the names and the statistics (launch.hip); group_runs may
  // still put a run into a launch of several
  for (size_t ri = 0; ri < gen_runs.size(); ri++) {
    LaunchPlan::Run &r = q.runs[ri];
    if (!r.lane()) r.kind = r.layout = run_kernel(gen_runs[ri], r.G, r.flat_nc > 0, q.dense_env, p.paired != 0);
  }
}

// single-end runs whose events all have a class table go to sampler_flat (kernels_flat.inl): NC chains
// per wavefront, as many as fit the wavefront's share of the LDS (two workgroups of four wavefronts
// per CU: 20 KB each), fewer when the batch would not fill the device otherwise.
// (knobs.no_flat: sampler_grp as in round 1; knobs.flat_nc forces the chains per wavefront.)
void miso_batch::plan_flat(size_t ri) {
  const GenRun &run = gen_runs[ri];
  LaunchPlan::Run &r = plan.runs[ri];
  // up to twenty isoforms the kernel of the launch's largest isoform count (its slice layout at compile time,
  // kernels_flat.inl)
  const int lo = run.kc == 4 ? 3 : (run.kc == 8 ? 5 : (run.kc == 12 ? 9 : (run.kc == 16 ? 13 : 17)));
  r.flat_ks = (run.kc <= 32 && run.kmax >= lo && run.kmax <= std::min(run.kc, 20) && !knobs.flat_no_ks) ? run.kmax : 0;
  // ... and, when every event of the launch has that count, the kernel that knows it (UNI: no per-chain `k < K` masks)
  r.flat_uni = r.flat_ks > 0 && run.kmin == run.kmax && !knobs.flat_no_uni;
  if (r.lane()) return;
  if (p.paired || run.nocls || run.kc >= 64 || knobs.no_flat) return;
  const int slice = flat_layout(run.kmax, std::max(run.maxcls, 1)).bytes;
  const int wgs = flat_wgs(run.kc);
  const size_t lds_wave = knobs.lds_max_kb.set ? plan.lds_max / 4 : static_cast<size_t>(160 * 1024 / (4 * wgs)) - 64;
  const int nc_max = std::min<int>(64, static_cast<int>(lds_wave) / slice);
  if (nc_max < 1) return;
  const long chains = static_cast<long>(run.count) * p.noChains;
  // the fewest rounds of resident wavefronts that nc_max allows, then the fewest chains per wavefront
  // that still makes that many rounds (a 40 000-chain batch at nc_max = 17 would run 1.15 rounds = 2)
  const long slots = std::max<long>(1, static_cast<long>(slots_for(chains)) * wgs / 2);
  const long rounds = std::max<long>(1, (chains + slots * nc_max - 1) / (slots * nc_max));
  int nc = static_cast<int>(std::min<long>(nc_max, std::max<long>(1, (chains + slots * rounds - 1) / (slots * rounds))));
  // five to eight isoforms: how the 64 lanes divide over a wavefront's chains and items matters more than the
  // rounds -- measured on one device, 40 000 events (events/s at 5 / 6 / 7 / 8 / 10 chains per wavefront):
  // K=6 69.4k / 67.5k / 72.2k / 77.2k / 68.6k, K=7 64.1k / 61.4k / 68.8k / 73.5k / 64.3k, K=8 55.8k / 57.1k /
  // 52.6k / 55.1k / 54.4k; K=5: 8 -> 93.4k, 7 -> 90.3k, 10 -> 86.8k.  (Timing the candidates on the first launch
  // was tried: a 7 % difference is inside the noise of a 200-iteration trial, the choice flipped between runs.)
  if (run.kc == 8) nc = std::min(nc, run.kmin >= 8 ? 6 : 8);
  if (run.kc == 4 && run.kmin >= 4) nc = std::min(nc, 8);   // four isoforms, descriptor loop: 8 -> 119.8k, 16 -> 116.1k, 13 -> 85.5k
  if (knobs.flat_nc.set) nc = std::max(1, std::min(nc_max, knobs.flat_nc.v));
  r.flat_nc = nc; r.flat_nc_max = nc_max;
}

void miso_batch::plan_grp(size_t ri, const KernelArgs &a) {
  GenRun &run = gen_runs[ri];
  LaunchPlan::Run &r = plan.runs[ri];
  if (r.lane()) return;
  if (run.kc >= 64) { r.flat_nc = 0; r.G = 64; r.sh = GrpShape{0, 0}; return; }   // more than 32 isoforms: one wavefront per chain
  // sampler_flat or sampler_grp?  Measured on the batch's first launch like the lanes per chain below
  // (flat wins at every isoform count of profiles/r02_flat_vs_grp_sweep.txt but 5); a small or untuned
  // batch takes sampler_flat.
  const bool contest = r.flat_nc > 0 && plan.tune_runs && static_cast<long>(run.count) * p.noChains >= 2048 &&
                       run.tuned_flat < 0 && !knobs.flat_nc.set;
  if (r.flat_nc > 0 && run.tuned_flat == 0) r.flat_nc = 0;
  if (r.flat_nc > 0 && !contest) return;
  GrpShape &sh = r.sh = grp_shape(run);
  const long chains = static_cast<long>(run.count) * p.noChains;
  int G = 64;
  if (run.wide()) {   // one chain per workgroup (launch_grp): the score table joins the slice when four of them fit
    GrpShape w{0, 0};
    w.ts = run.kmax * plan.il2;
    if (fp_bytes_of(run) + 4 * static_cast<size_t>(grp_slice_bytes(run.kmax, 0, w.ts)) + 64 > plan.lds_max) w.ts = 0;
    r.sh = w;
    r.G = 64;
    return;
  }
  if (knobs.general_lanes.set) {
    G = knobs.general_lanes.v;
  } else if (knobs.general_lanes_by_class_set) {
    G = 16;
    for (const auto &c : knobs.general_lanes_by_class) if (c.first == run.kc) G = c.second;
  } else if (run.tuned_G) {
    G = run.tuned_G;
    if (p.paired && sh.ts && !grp_fits(run, sh, G)) {   // chosen with the score tables in global memory (the eight-lane rule below)
      GrpShape s0 = sh;
      s0.ts = 0;
      if (grp_fits(run, s0, G)) sh = s0;
    }
  } else {
    // rule of thumb.  single-end: the per-iteration scalar step costs the same per wavefront
    // whatever G is, so pack as many chains per wavefront as still fills the device: the smallest
    // G whose wavefronts occupy every resident slot; a batch too small for that takes the largest.
    // paired-end: the read loop waits on memory and more wavefronts hide it: largest G up to 16; 32 from
    // nine isoforms on (measured, pe_dense: K=10 19.5k -> 19.9k, K=20 7.35k -> 7.57k events/s; K=5 29.9k ->
    // 28.9k, K=3 53k -> 46k) and whenever 16 would leave the kernel's share of the device unfilled.
    bool found = false;
    // (a whole-gene mix -- several classes side by side -- runs 9 % faster with 32 everywhere: 14.4k -> 15.7k genes/s)
    // (round 3, 20 000 events of one isoform count: 16 lanes beat 32 from nine isoforms on as well once the launch
    // is more than a round and a half of wavefronts -- K = 9 21.3k -> 26.8k, K = 10 20.8k -> 26.9k, K = 12 19.1k ->
    // 22.5k, K = 16 14.4k -> 16.6k, K = 20 10.7k -> 10.9k events/s; the mix keeps 32: 16.8k vs 14.2k genes/s;
    // profiles/r03_pe_lanes_sweep.txt)
    int n_classes = 0;
    for (size_t rj = 0; rj < gen_runs.size(); rj++) if (rj == 0 || gen_runs[rj].kc != gen_runs[rj - 1].kc) n_classes++;
    // (round 3, 8 hardware queues, 16 384 genes of 3-20 isoforms per 1500 iterations: 16 lanes up to 16 isoforms against 32
    // everywhere -- 400 pairs per gene 120 vs 150 ms, 1000 pairs 194 vs 206 ms, hg19-like counts 176 vs 175 ms, 2500 pairs
    // 436 vs 367 ms: small genes share the scalar step four to a wavefront, large ones want the lanes; the switch sits at a
    // mean of 400 drawing quads per gene of the class; knobs.pe_mix_lanes forces)
    const double mean_q = run.sum_q / std::max(1, run.count);
    // (round 5, same batch on one box, 7500 iterations: the 17 - 20 isoform class on 16 lanes as well -- 1000 pairs per gene
    // 930 -> 852 ms, hg19-like pair counts 865 -> 820 ms: four chains of a wavefront share the scalar step, and the class
    // no longer fills the device with half-efficient wavefronts for the launch's first third while the other classes
    // wait; the bucket of "at least 32 lanes" from a need of 32 lanes instead of 24: a 20-isoform gene of 1000 pairs
    // needs 28 by the share rule; profiles/r05_pe_mix_lanes.txt)
    const bool mix16 = run.kc <= 32 && !run.force_G() && (knobs.pe_mix_lanes.set ? knobs.pe_mix_lanes.v == 16 : mean_q < 400.0);
    const bool pe32 = p.paired && ((n_classes + (n_k2 > 0 ? 1 : 0) > 1 && !mix16) || (run.kc >= 12 && 2 * ((chains + 3) / 4) < 3 * static_cast<long>(slots_for(chains))) ||
                                   (chains + 3) / 4 < slots_for(chains));
    for (int g : {2, 4, 8, 16, 32}) {
      if (p.paired && g > 16 && found && !pe32) break;
      if (!grp_fits(run, sh, g)) continue;
      const int cpw = 64 / g;
      if (!found || g <= std::max(2, run.maxq)) G = g;
      found = true;
      if (!p.paired && (chains + cpw - 1) / cpw >= slots_for(chains)) break;
    }
    // Round 5, paired-end, ONE isoform-count class in the batch, five to nine isoforms, two rounds of wavefronts and more at
    // eight lanes: EIGHT lanes per chain -- eight chains of a wavefront share the scalar step instead of four.  Rounds 2 - 4
    // measured that slower (the read loop waited on memory and more wavefronts hid it); since the draws are ordered by
    // fragment rows and the loop's header no longer waits for fresh gathers it wins: 40 000 events x 1000 pairs, K = 5 / 6 / 7 /
    // 8 / 9: 45.3 -> 54.2, 41.5 -> 48.7, 40.5 -> 45.5, 38.0 -> 40.5, 30.2 -> 31.5 k events/s; K = 12: 25.7 -> 21.2 k, four lanes
    // 33.7 k at K = 5; in a whole-gene mix, where a class is a few thousand genes, 19.2 -> 18.2 k genes/s: not there
    // (profiles/r05_lanes_sweep.txt).  knobs.pe_lanes8 = 0 / 1: never / also in a mix and for the size buckets' normal run.
    {
      const Opt<int> &l8 = knobs.pe_lanes8;
      const bool single = n_classes + (n_k2 > 0 ? 1 : 0) == 1;
      const bool want8 = l8.set && l8.v != 2 ? l8.v != 0 : ((single || l8.set) && chains >= 8L * 2 * slots_for(chains));   // (2: the rule in a mix of classes too)
      if (p.paired && want8 && G == 16 && !run.force_G() && run.kmin >= 5 && run.kmax <= 9 && grp_fits(run, sh, 8)) G = 8;
      // Three and four isoforms the same -- there the class keeps its score tables in LDS (grp_shape), which holds four
      // chains per wavefront and no more: eight chains with the tables in global memory (an L2 line per pick) instead,
      // K = 3 66.6 -> 78.9 k, K = 4 58.1 -> 68.0 k events/s; the tables alone are worth 2 % (16 lanes without them 65.3 /
      // 57.0 k), four lanes lose (55.9 / 37.6 k) (profiles/r05_lanes_sweep.txt).
      if (p.paired && want8 && G == 16 && !run.force_G() && run.kmax <= 4) {
        GrpShape sh8 = sh;
        if (!grp_fits(run, sh8, 8)) sh8.ts = 0;
        if (grp_fits(run, sh8, 8)) { sh = sh8; G = 8; }
      }
    }
    if (plan.tune_runs && chains >= 2048 && G != 64) {
      std::vector<int> cand{G};
      // the rule errs on the small side (tail effect when the wavefronts do not fit one round)
      for (int g : {G * 2, G * 4})
        if (!p.paired && grp_fits(run, sh, g) && g <= std::max(2, 2 * run.maxq)) cand.push_back(g);
      if (cand.size() > 1)
        G = fastest(a, cand, [&](const KernelArgs &t, int g) { launch_grp(t, run, sh, g, stream); });
      run.tuned_G = G;
    }
  }
  if (run.force_G() && G < run.force_G() && !knobs.general_lanes.set) G = run.force_G();   // size bucket (upload)
  if (run.small() && p.paired && !knobs.general_lanes.set && !knobs.general_lanes_by_class_set) {   // the small genes' bucket: eight chains per wavefront, score tables in global memory
    GrpShape sh8 = sh;
    sh8.ts = 0;
    if (grp_fits(run, sh8, 8)) { sh = sh8; G = 8; }
  }
  // a forced (or odd) choice never exceeds the LDS budget: fewer chains per wavefront instead
  while (G < 64 && !grp_fits(run, sh, G)) G = (G < 2) ? 2 : ((G & (G - 1)) ? 64 : G * 2);
  r.G = G;
  if (contest) {
    const int win = (G == 64) ? 0 : fastest(a, {0, G}, [&](const KernelArgs &t, int g) {
      if (g == 0) launch_flat(t, ri, stream); else launch_grp(t, run, sh, g, stream); });
    run.tuned_flat = win == 0 ? 1 : 0;
    if (win != 0) r.flat_nc = 0;
  }
}

// ---- the general runs into launches: all in one sampler_grp_all, a class's in one sampler_grp_multi, a size bucket with
// the run after it ----
void miso_batch::group_runs() {
  LaunchPlan &q = plan;
  // Paired-end, two classes or more, every run on dense records with sixteen lanes per chain (a whole-gene batch of like-sized
  // genes): ALL of them in one launch (sampler_grp_all, kernels_grp.inl), the segments ordered by what a workgroup costs --
  // (quads per lane + the scalar step) x isoforms, descending: longest first across the classes.  Every segment keeps the run's
  // own slice layout (launch_grp's).  Batches with size buckets (real pair counts) keep a launch per class
  // (sampler_grp_multi): twenty bodies in one kernel do not compile in reasonable time (round 5: 28 minutes, 802 spilled registers).
  {
    bool all_ok = p.paired && !q.lane_gen && gen_runs.size() >= 2 && gen_runs.size() < 127 && !knobs.no_pe_all &&
                  !knobs.no_pe_multi && !knobs.serial_kernels && (!knobs.general_lanes.set || knobs.pe_all);
    bool two_classes = false;
    for (size_t ri = 0; ri < gen_runs.size() && all_ok; ri++) {
      const GenRun &run = gen_runs[ri];
      all_ok = !q.runs[ri].lane() && q.runs[ri].flat_nc == 0 && fp_rows(run) && run.kc <= 32 && !run.wide() && q.runs[ri].G == 16;
      two_classes |= run.kc != gen_runs[0].kc;
    }
    q.grp_all = all_ok && two_classes;
    if (q.grp_all)
      for (LaunchPlan::Run &r : q.runs) r.kind = RunKernel::GrpAll;
  }
  // Paired-end: the size buckets of one isoform-count class in ONE launch (sampler_grp_multi<KC>, kernels_grp.inl):
  // segments = the class's runs in list order -- workgroup-wide chains (those on several workgroups in front), a
  // wavefront per chain, 32 lanes, 16 lanes.
  // When: the batch's launches outnumber the hardware queues (a whole-gene mix with real read counts: ~20 launches, 243 ->
  // 180 ms per 1500 iterations; a single class's three or four buckets run 3 % faster side by side: 149 vs 155 ms at K = 5;
  // profiles/r03_pe_buckets.txt); knobs.pe_multi forces.
  // ... or some run on 16 / 32 lanes holds several isoform counts: the multi kernel's segments keep them in wavefronts of their own
  bool any_mixed = false;
  for (size_t ri = 0; ri < gen_runs.size(); ri++) {
    const int G = q.runs[ri].G;
    any_mixed |= p.paired && !gen_runs[ri].wide() && (G == 16 || G == 32 || (G == 8 && gen_runs[ri].small())) && fp_rows(gen_runs[ri]) && q.runs[ri].flat_nc == 0 && gen_runs[ri].kmin != gen_runs[ri].kmax;
  }
  const bool multi_on = p.paired && !q.lane_gen && !knobs.no_pe_multi && !knobs.general_lanes.set &&
                        (knobs.pe_multi || gen_runs.size() + (n_k2 > 0 ? 1 : 0) > 8 || any_mixed);
  for (size_t r0 = 0; multi_on && !q.grp_all && r0 < gen_runs.size();) {
    size_t r1 = r0 + 1;
    while (r1 < gen_runs.size() && gen_runs[r1].kc == gen_runs[r0].kc) r1++;
    const int G0 = q.runs[r0].G;
    bool ok = (r1 - r0 >= 2 || (r1 - r0 == 1 && gen_runs[r0].kmin != gen_runs[r0].kmax && (G0 == 16 || G0 == 32 || (G0 == 8 && gen_runs[r0].small())))) &&
              r1 - r0 <= static_cast<size_t>(K2_MAX_SEGS);
    for (size_t ri = r0; ri < r1 && ok; ri++) {
      const GenRun &run = gen_runs[ri];
      const int G = q.runs[ri].G;
      ok = q.runs[ri].flat_nc == 0 && fp_rows(run) && (ri == r0 || run.first == gen_runs[ri - 1].first + gen_runs[ri - 1].count) &&
           (run.wide() || G == 16 || G == 32 || (G == 64 && run.wave64()) || (G == 8 && run.small()));
    }
    if (ok) {   // every segment's slices fit the workgroup's LDS
      const GenRun m = joined_run(r0, r1);
      const size_t fp_bytes = fp_bytes_of(m), slice = grp_slice_bytes(m.kmax, 0, grp_shape(m).ts), slice8 = grp_slice_bytes(m.kmax, 0, 0);
      for (size_t ri = r0; ri < r1 && ok; ri++)
        if (!gen_runs[ri].wide()) ok = fp_bytes + 4 * static_cast<size_t>(64 / q.runs[ri].G) * (q.runs[ri].G == 8 ? slice8 : slice) <= q.lds_max;
    }
    if (ok) {
      q.multi.emplace_back(r0, r1);
      for (size_t ri = r0; ri < r1; ri++) q.runs[ri].kind = RunKernel::GrpMulti;
    }
    r0 = r1;
  }
  // A size bucket whose lanes came out the same as the class's normal launch joins it: one launch (its chains stay
  // in front: longest first), one hardware queue less to wait in (kernels of different streams share the process's
  // hardware queues, and a kernel waits for the one before it in its queue).
  // (measured, 16 384 genes of 3-20 isoforms: 4 queues 290 -> 254 ms merged; 8 queues 195 ms apart, 241 ms merged --
  // the separate launches stagger the classes' starts; the queue count is the host's, capi.hip only records it)
  // (what is IN EFFECT, not what the environment says now: capi.hip's constructor records it; 0 = unknown -- not set, or the
  // runtime was up before this library was loaded -- counts as the runtime's default of 4)
  const int hwq = g_hw_queues_in_effect > 0 ? g_hw_queues_in_effect : 4;
  const bool merge_on = !knobs.no_pe_merge && (knobs.pe_merge || hwq < 8);
  for (size_t ri = 0; merge_on && ri + 1 < gen_runs.size(); ri++) {
    const GenRun &run = gen_runs[ri], &nx = gen_runs[ri + 1];
    const LaunchPlan::Run &r = q.runs[ri], &rx = q.runs[ri + 1];
    if (r.lane() || r.grouped() || (ri > 0 && q.runs[ri - 1].merge_next)) continue;
    if (!run.wide() && run.force_G() && r.G != 64 && r.flat_nc == 0 && !nx.wide() && !nx.force_G() && nx.kc == run.kc && rx.G == r.G &&
        rx.flat_nc == 0 && nx.first == run.first + run.count) {
      const GenRun m = joined_run(ri, ri + 2);
      q.runs[ri].merge_next = grp_fits(m, grp_shape(m), r.G);
    }
  }
}


// the statistics of an event of the exact list as exact_probe and exact_compare take them
void miso_batch::exact_stats7(int event, double *r) const {
  const PackedEvent &e = events[event];
  r[0] = e.base_count[0]; r[1] = e.base_count[1]; r[2] = e.base_count[0] + e.base_count[1] + e.n_draw;
  r[3] = e.eff[0]; r[4] = e.eff[1]; r[5] = e.hyper[0]; r[6] = e.hyper[1];
}

// Posterior mean and the two quantiles of every event the exact mode took, from the grid itself (exact_probe): made once
// per confidence level, for all of them.
void miso_batch::exact_summaries(double confidence_level) {
  if (!launched) MISO_FAIL(MISO_EINVAL, "batch not launched");
  if (!(confidence_level > 0 && confidence_level < 1)) MISO_FAIL(MISO_EINVAL, "Invalid confidence level");
  if (exact_sums_level == confidence_level && exact_sums.size() == static_cast<size_t>(n_exact) * 6) return;
  HIP_OK(hipSetDevice(device));
  const double alpha = 1 - confidence_level;
  const double prob[2] = {alpha / 2, 1 - alpha / 2};
  std::vector<double> st(static_cast<size_t>(n_exact) * 7), out8(static_cast<size_t>(n_exact) * 8), q(static_cast<size_t>(n_exact) * 4);
  if (p.paired) {   // the pairs' records are on the device: the events of the exact list themselves
    KernelArgs ka{};
    ka.events = d_events; ka.in_pool = d_in; ka.out_pool = d_out; ka.frag_prob = d_fp;
    ka.il = static_cast<int32_t>(fd.prob.size());
    ka.slot_event = d_slots + n_k2 + n_gen; ka.n_slots = n_exact;
    exact_paired_probe_run(&ka, exact_eff.d, nullptr, nullptr, nullptr, n_exact, prob, 2, out8.data(), q.data(), stream);
  } else {
    for (int j = 0; j < n_exact; j++) exact_stats7(h_slots[n_k2 + n_gen + j], &st[static_cast<size_t>(j) * 7]);
    exact_probe_run(st.data(), n_exact, prob, 2, out8.data(), q.data(), stream);
  }
  exact_sums.assign(static_cast<size_t>(n_exact) * 6, 0.0);
  for (int j = 0; j < n_exact; j++) {
    double *r = &exact_sums[static_cast<size_t>(j) * 6];
    const double *lo = &q[static_cast<size_t>(j) * 4], *hi = lo + 2;   // {x, 1 - x} at the low and at the high quantile
    r[0] = out8[static_cast<size_t>(j) * 8]; r[1] = out8[static_cast<size_t>(j) * 8 + 1];
    r[2] = lo[0]; r[3] = hi[1];
    r[4] = hi[0]; r[5] = lo[1];
  }
  exact_sums_level = confidence_level;
}


void miso_batch::sync(float *ms) {
  if (!launched) MISO_FAIL(MISO_EINVAL, "batch not launched");
  HIP_OK(hipSetDevice(device));
  HIP_OK(hipStreamSynchronize(stream));
  HIP_OK(hipEventElapsedTime(&last_ms, ev0, ev1));
  if (ms) *ms = last_ms;
  read_clock_probe();
  // chains on several workgroups: did any group give up waiting for its members (coop.hpp)?
  bool gave_up = false;
  each_coop_table([&](const CoopTable &cc) {
    if (!cc.mem.d || cc.chains == 0) return;
    std::vector<uint32_t> w(static_cast<size_t>(cc.chains) * COOP_WORDS);
    HIP_OK(hipMemcpy(w.data(), cc.mem.d, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int c = 0; c < cc.chains; c++) gave_up |= w[static_cast<size_t>(c) * COOP_WORDS + 1] != 0;
  });
  if (!gave_up) { converge_rounds(ms); return; }
  // A chain's workgroups did not all become resident in time (a busy device: other batches, other processes).  The
  // batch must not fail for it -- the reference's workers share nothing (misopy/miso.py:165-187) --, so the launch is
  // repeated here, in this process, with every chain on ONE workgroup: same results bit for bit (the contract's random
  // numbers do not depend on the layout), no exchange between workgroups left that could wait.
  if (no_coop) MISO_FAIL(MISO_EINTERNAL, "a chain timed out waiting for its workgroups although every chain has one workgroup");
  const float first_ms = last_ms;
  no_coop = true; coop_retries++;
  std::fill(coop_n.begin(), coop_n.end(), 1);
  each_coop_table([](CoopTable &c) { c.reset(); });
  k2[0].plan_key = k2[1].plan_key = -1; coop_wgs_used = 0;
  pool_cleared = false;   // (the abandoned chains left their sample columns half written)
  std::fprintf(stderr, "[miso] a chain on several workgroups gave up waiting for its workgroups after %.1f ms (busy device?): "
                       "re-running the launch with one workgroup per chain\n", first_ms);
  launch(last_seed, last_first_event_id);
  sync(ms);
}

// stop = CONVERGENT_MEAN: what the reference does after every round of its iteration loop (miso.c:903-925,
// miso_paired.c:501-523).  Events whose chains have not converged -- and whose schedule is still below maxIterations --
// run another round, noIterations' = 3 noIterations - 2 noBurnIn with noBurnIn' = noIterations, and of that round's samples
// the LAST noSamples replace the first round's (miso.c:976-983), here in the device pool, so that the summaries, the file
// writer and the getters see one finished batch.  The reference CONTINUES its chains: round r keeps the iterations
// [G_r + B_r, G_r + N_r) of one chain, G_r = the iterations of all earlier rounds.  The device keeps no chain state
// between launches, so it runs iterations [0, G_r + N_r) from the start with burn-in G_r + B_r: iteration m of a chain
// draws from the same addresses whatever the schedule, so the first G_r iterations repeat the earlier rounds bit for bit
// and the kept window is the reference's (round 6; rounds 4 - 5 ran N_r from the start and kept [B_r, N_r): the same law
// in the limit, half the burn-in).  The reference's loop counter restarts with every round and so does its rule "no
// proposal terms in a round's first ratio" (miso.c:866): the kernels are told where the later rounds open
// (KernelArgs::round_tab, device.hpp RoundOpen).  The CPU checker's counter mode continues its chains like the
// reference and addresses the draws by the chain's own iteration number: equal bit for bit (tests/test_gpu_convergent.py).
// The next round is a batch of its own (only the unconverged events; its sync() recurses).  The rounds have no limit of
// their own, as in the reference (`while (1)`): they end when the iterations from the chain's start through the next round
// no longer fit the kernels' 32-bit counter, and then the last round stands.  The kept window doubles with every round
// (N' - B' = 2 (N - B)), so that is before round MISO_MAX_ROUNDS = 32, the size of the table of round starts.
void miso_batch::converge_rounds(float *ms) {
  // once per launch: a second sync() must not test the samples the further rounds have already put in place (they might
  // pass now and reset the accept counts' bookkeeping, or fail and run the rounds -- and the paired-end sums -- twice)
  if (converged_done) { if (ms) *ms = last_ms; return; }
  converged_done = true;
  rounds = 1;
  iters_counted.clear(); went_on.clear();
  // this round's own schedule, the reference's (noIterations, noBurnIn): the batch's for the first round
  const int N = round_iters > 0 ? round_iters : p.noIterations, B = round_iters > 0 ? round_burn : p.noBurnIn;
  if (p.stop != MISO_STOP_CONVERGENT_MEAN || p.maxIterations <= N || events.empty()) return;
  const int S0 = S(), C = p.noChains;
  if (S0 < C) return;                        // fewer kept samples than chains: nothing to assess
  std::vector<unsigned char> out(out_bytes);
  HIP_OK(hipMemcpy(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost));
  std::vector<int> again;
  for (size_t i = 0; i < events.size(); i++)
    if (!event_exact(static_cast<int>(i)) &&   // (independent draws from the posterior itself: done after the first round)
        !convergent_mean(reinterpret_cast<const double *>(out.data() + h_events[i].off_samples), events[i].K, C, S0))
      again.push_back(static_cast<int>(i));
  if (again.empty()) return;
  const int64_t N2 = 3LL * N - 2LL * B, total = static_cast<int64_t>(p.noIterations) + N2;
  if (total > INT32_MAX) return;             // (the kernels count iterations in 32 bits)
  if (static_cast<int>(round_starts.size()) >= MISO_MAX_ROUNDS - 1)   // (a window of >= 1 iteration doubled 31 times is past INT32_MAX)
    MISO_FAIL(MISO_EINTERNAL, "stop = CONVERGENT_MEAN: more rounds than the table of round starts holds");
  miso_params_t p2 = p;
  p2.noIterations = static_cast<int>(total); p2.noBurnIn = p.noIterations + N;   // miso.c:921-923, behind what has been run
  p2.want_counts_trace = 0; p2.device_match = 0;
  std::unique_ptr<miso_batch> next(batch_new(p2));
  next->round_iters = static_cast<int>(N2); next->round_burn = N;
  next->round_starts = round_starts; next->round_starts.push_back(p.noIterations);
  for (int i : again) {
    next->events.push_back(events[i]);
    const bool pinned = i < static_cast<int>(event_ids.size()) && event_ids[i] >= 0;
    next->event_ids.push_back(pinned ? event_ids[i] : static_cast<int64_t>(last_first_event_id + static_cast<uint32_t>(i)));
  }
  next->collapsed = collapsed; next->collapsed_level = collapsed_level; next->no_coop = no_coop;
  float next_ms = 0.f;
  next->upload(device);
  next->launch(last_seed, 0);
  next->sync(&next_ms);
  const int Sn = next->S();
  std::vector<unsigned char> nout(next->out_bytes);
  HIP_OK(hipMemcpy(nout.data(), next->d_out, next->out_bytes, hipMemcpyDeviceToHost));
  // iterations behind an event's accept count: the single-end loop starts both counters afresh every round, the
  // paired-end one never does (miso.c:847 against miso_paired.c:345, 453)
  iters_counted.assign(events.size(), p.paired ? p.noIterations : N);
  for (size_t j = 0; j < again.size(); j++) {
    const int i = again[j];
    const DevEvent &d = h_events[i], &n = next->h_events[j];
    const PackedEvent &e = events[i];
    const size_t skip = static_cast<size_t>(Sn - S0);
    HIP_OK(hipMemcpyAsync(d_out + d.off_samples, next->d_out + n.off_samples + skip * e.K * 8, static_cast<size_t>(S0) * e.K * 8,
                          hipMemcpyDeviceToDevice, stream));
    HIP_OK(hipMemcpyAsync(d_out + d.off_loglik, next->d_out + n.off_loglik + skip * 8, static_cast<size_t>(S0) * 8,
                          hipMemcpyDeviceToDevice, stream));
    if (e.n_draw > 0)
      HIP_OK(hipMemcpyAsync(d_out + d.off_drawass, next->d_out + n.off_drawass, e.n_draw, hipMemcpyDeviceToDevice, stream));
    // accept counts.  The next launch counted from the chain's start: that IS the paired-end number; the single-end one
    // is what the last round added, i.e. minus this launch's own count (the same chain up to here).  An event that went
    // through further rounds in `next` comes back already settled.
    const bool settled = !next->iters_counted.empty() && next->event_went_on(static_cast<int>(j));
    ChainStats *mine = reinterpret_cast<ChainStats *>(out.data() + d.off_stats);
    const ChainStats *theirs = reinterpret_cast<const ChainStats *>(nout.data() + n.off_stats);
    for (int c = 0; c < C; c++) {
      const int32_t before = mine[c].accepted;
      mine[c] = theirs[c];
      if (!p.paired && !settled) mine[c].accepted -= before;
    }
    iters_counted[i] = !next->iters_counted.empty() ? next->iters_counted[j] : (p.paired ? total : N2);
    HIP_OK(hipMemcpyAsync(d_out + d.off_stats, mine, sizeof(ChainStats) * C, hipMemcpyHostToDevice, stream));
  }
  went_on.assign(events.size(), 0);
  for (int i : again) went_on[i] = 1;
  HIP_OK(hipStreamSynchronize(stream));
  rounds = 1 + next->rounds;
  last_ms += next_ms;
  if (ms) *ms = last_ms;
  coop_retries += next->coop_retries;
  last_kernels += "," + next->last_kernels;
}

// The reduction passes over the resident samples, one workgroup per (event, isoform) column (column_pass.hpp).  Each makes its
// results beside the stored ones and puts them in their place at the end, with the flag and the kernel time: a call that
// fails frees what it held on the device (HipCall) and leaves what was there.

// Posterior mean and Chen-Shao credible interval of every isoform, computed where the samples are (the interval's order
// statistics: column_pass.hpp ci_ranks).
void miso_batch::summarize(double confidence_level, bool as_text) {
  if (!launched) MISO_FAIL(MISO_EINVAL, "batch not launched");
  finish_rounds(*this);
  HIP_OK(hipSetDevice(device));
  const int n = static_cast<int>(events.size()), Sn = S();
  const CiRanks r = ci_ranks_strict(Sn, confidence_level);
  const int lo = static_cast<int>(r.lo), hi = static_cast<int>(r.hi);
  ColumnLayout l = column_layout(*this, 3);
  std::vector<double> res(l.total, 0.0);
  float ms = summarize_ms;
  if (n > 0) {
    HipCall call(stream);
    ms = column_pass(call, fn(summarize_kernel), dim3(n, l.kmax), 0, l.off, res.size(), res.data(),
                     [&](dim3 grid, const uint64_t *d_off, double *d_sum) {
                       hipLaunchKernelGGL(summarize_kernel, grid, dim3(256), 0, call.st, d_events, d_out, n, Sn, lo, hi, d_off, d_sum,
                                          as_text ? 1 : 0);
                     });
  }
  h_summary.swap(res);
  h_sum_off.swap(l.off);
  summarize_ms = ms;
  summarized = true;
}

// the guards diagnose() and diagnose_rank() share; returns the chains the samples are split by
static int diagnose_chains(const miso_batch &b, int noChains) {
  if (!b.launched) MISO_FAIL(MISO_EINVAL, "batch not launched");
  if (noChains < 0) MISO_FAIL(MISO_EINVAL, "Invalid number of chains");
  if (noChains == 0 && b.adopted) MISO_FAIL(MISO_EINVAL, "Adopted samples have no chain count of their own: give noChains");
  const int C = noChains ? noChains : b.p.noChains;
  if (b.S() / C / 2 < 4) MISO_FAIL(MISO_EINVAL, "Too few samples per chain for diagnostics");
  return C;
}

// Chain diagnostics of every (event, isoform) column, computed where the samples are (kernels_diagnose.hip):
// split R-hat, effective sample size, Monte-Carlo standard error of the mean and the lag at which Geyer's sequence was cut.
// noChains = 0: the batch's own chains; an adopted batch has none to offer.
void miso_batch::diagnose(int noChains) {
  const int C = diagnose_chains(*this, noChains);
  const int n_draws = S() / C, h = n_draws / 2;
  // (the per-sequence scratch of a workgroup: three doubles per sequence in LDS)
  if (C > DIAG_MAX_CHAINS) MISO_FAIL(MISO_EINVAL, "Too many chains for diagnostics");
  finish_rounds(*this);
  HIP_OK(hipSetDevice(device));
  const int n = static_cast<int>(events.size());
  const int M = 2 * C, N = M * h;
  ColumnLayout l = column_layout(*this, 4);
  std::vector<double> res(l.total, 0.0);
  float ms = diagnose_ms;
  if (n > 0) {
    const bool cached = N <= 256 * miso::SUMMARY_CACHE;
    const size_t dyn = (static_cast<size_t>(cached ? N : 0) + 3 * static_cast<size_t>(M)) * sizeof(double);
    HipCall call(stream);
    ms = column_pass(call, fn(diagnose_kernel), dim3(n, l.kmax), dyn, l.off, res.size(), res.data(),
                     [&](dim3 grid, const uint64_t *d_off, double *d_diag) {
                       hipLaunchKernelGGL(diagnose_kernel, grid, dim3(256), dyn, call.st, d_events, d_out, n, C, n_draws, h,
                                          std::log10(static_cast<double>(N)), cached ? 1 : 0, d_off, d_diag);
                     });
  }
  h_diag.swap(res);
  h_diag_off.swap(l.off);
  diagnose_ms = ms;
  diagnosed = true;
}

// Rank-normalised chain diagnostics of every (event, isoform) column (kernels_diagnose_rank.hip): bulk and
// folded split R-hat, bulk effective sample size, and the effective sample size of the indicators of the two bounds of
// the `confidence_level` interval, taken as summarize() takes them but over the N used draws.  Preconditions as diagnose().
void miso_batch::diagnose_rank(int noChains, double confidence_level) {
  const int C = diagnose_chains(*this, noChains);
  const int n_draws = S() / C, h = n_draws / 2;
  // (in 64 bits: C is the caller's)
  const int64_t M64 = 2 * static_cast<int64_t>(C), N64 = M64 * h;
  const CiRanks r = ci_ranks_strict(static_cast<double>(N64), confidence_level);
  if (N64 > RANK_MAX_DRAWS) MISO_FAIL(MISO_EINVAL, "Too many samples for rank diagnostics");
  if (C > RANK_MAX_CHAINS) MISO_FAIL(MISO_EINVAL, "Too many chains for rank diagnostics");
  const int M = static_cast<int>(M64), N = static_cast<int>(N64);
  const int lo = static_cast<int>(r.lo), hi = static_cast<int>(r.hi);
  finish_rounds(*this);
  HIP_OK(hipSetDevice(device));
  const int n = static_cast<int>(events.size());
  ColumnLayout l = column_layout(*this, 6);
  std::vector<double> res(l.total, 0.0);
  float ms = rank_ms;
  if (n > 0) {
    int P = 8;                                          // the sort's size: the power of two >= N
    while (P < N) P <<= 1;
    // the draws, the sort's keys, then the larger of the per-sequence scratch and the 16-bit ranks
    const size_t dyn = (static_cast<size_t>(N) + P + std::max<size_t>(3 * static_cast<size_t>(M), (static_cast<size_t>(N) + 3) / 4)) * sizeof(double);
    HipCall call(stream);
    ms = column_pass(call, fn(diagnose_rank_kernel), dim3(n, l.kmax), dyn, l.off, res.size(), res.data(),
                     [&](dim3 grid, const uint64_t *d_off, double *d_rank) {
                       hipLaunchKernelGGL(diagnose_rank_kernel, grid, dim3(256), dyn, call.st, d_events, d_out, n, C, n_draws, h, P, lo,
                                          hi, std::log10(static_cast<double>(N)), d_off, d_rank);
                     });
  }
  h_rank.swap(res);
  h_rank_off.swap(l.off);
  rank_ms = ms;
  rank_diagnosed = true;
}

// Two-sample comparison of this batch (sample 1) with `other` (sample 2), event by event and
// index-paired (hypothesis_test.py:89-179): both must hold the same events in the same order.
void miso_batch::compare(miso_batch &other, double smoothing) {
  same_events(*this, other, true);
  if (!(smoothing > 0)) MISO_FAIL(MISO_EINVAL, "Invalid smoothing parameter");
  const int n = static_cast<int>(events.size()), Sn = S();
  if (Sn < 2) MISO_FAIL(MISO_EINVAL, "Too few samples to compare");
  finish_rounds(*this);
  finish_rounds(other);
  ColumnLayout l = column_layout(*this, 4);
  std::vector<double> res(l.total, 0.0);
  float ms = compare_ms;
  if (n > 0) {
    HIP_OK(hipSetDevice(device));
    HIP_OK(hipStreamSynchronize(other.stream));
    HipCall call(stream);
    ms = column_pass(call, fn(compare_kernel), dim3(n, l.kmax), 0, l.off, res.size(), res.data(),
                     [&](dim3 grid, const uint64_t *d_off, double *d_cmp) {
                       hipLaunchKernelGGL(compare_kernel, grid, dim3(256), 0, call.st, d_events, d_out, other.d_events, other.d_out, n,
                                          Sn, smoothing, d_off, d_cmp);
                     });
  }
  h_compare.swap(res);
  h_cmp_off.swap(l.off);
  compare_ms = ms;
  compared = true;
}

// The posterior of delta psi over ALL S1 * S2 pairs of this batch's draws (sample 1) and `other`'s (sample 2), event by event
// (kernels_compare_pairs.hip): the lower median and the bounds of the `confidence_level` interval of the
// differences -- ranks as summarize() takes them but over S1 * S2, clamped --, the exact counts of the differences above and
// below 0 and, per threshold, of those at least that far from 0.  The batches hold the same events in the same order; their
// sample counts may differ.  The results stand beside compare()'s.  as_text: of the draws as the `.miso` files print them
// ("%.4f"), as summarize()'s.
void miso_batch::compare_pairs(miso_batch &other, double confidence_level, const double *tau, int n_tau, bool as_text) {
  same_events(*this, other, false);
  const int n = static_cast<int>(events.size()), S1 = S(), S2 = other.S();
  if (S1 < 1 || S2 < 1) MISO_FAIL(MISO_EINVAL, "Too few samples to compare");
  if (S1 > PAIRS_MAX_DRAWS || S2 > PAIRS_MAX_DRAWS)
    MISO_FAIL(MISO_EINVAL, "Too many samples for the all-pairs comparison: 8192 per event and sample at most");
  const int64_t M = static_cast<int64_t>(S1) * S2;
  const PairsArgs pa = pairs_args(M, confidence_level, tau, n_tau);
  finish_rounds(*this);
  finish_rounds(other);
  const size_t W = static_cast<size_t>(pairs_words(n_tau));
  ColumnLayout l = column_layout(*this, 1);
  // an event whose sample text was not decoded in either batch (adopt_text): the kernel does not touch its columns, they
  // come back not finite -- the top bit of the event's column offset says so
  std::vector<uint64_t> off_flagged(l.off);
  for (int i = 0; i < n; i++)
    if (event_unread(i) || other.event_unread(i)) off_flagged[i] |= PAIRS_SKIP_EVENT;
  std::vector<uint64_t> res(l.total * W, 0);
  float ms = 0.f;
  if (n > 0) {
    HIP_OK(hipSetDevice(device));
    HIP_OK(hipStreamSynchronize(other.stream));
    const size_t dyn = (static_cast<size_t>(S1) + S2) * sizeof(uint64_t);   // both columns: what is live, not the limit
    HipCall call(stream);
    ms = column_pass(call, fn(compare_pairs_kernel), dim3(n, l.kmax), dyn, off_flagged, res.size(), res.data(),
                     [&](dim3 grid, const uint64_t *d_off, uint64_t *d_res) {
                       hipLaunchKernelGGL(compare_pairs_kernel, grid, dim3(256), dyn, call.st, d_events, d_out, S1, other.d_events,
                                          other.d_out, S2, n, pa, as_text ? 1 : 0, d_off, d_res);
                     });
    note_pass("compare_pairs");
  }
  h_pairs.swap(res);
  h_pairs_off.swap(l.off);
  pairs_ntau = n_tau;
  pairs_M = M;
  pairs_ms = ms;
  pairs_compared = true;
}

// The two kinds of exact pair, as the comparison and the quantiles of delta psi take them: whether both batches ran the
// kind's mode, and an event's row of statistics in the kind's selftest layout.
static bool exact_single_ok(const miso_batch &a, const miso_batch &b) {
  return a.exact && b.exact && a.slots_exact == a.exact && b.slots_exact == b.exact;
}
static bool exact_paired_ok(const miso_batch &a, const miso_batch &b) {
  return a.p.paired && b.p.paired && a.exact_paired && b.exact_paired && a.slots_exact == a.exact_paired && b.slots_exact == b.exact_paired;
}
static const char *const EXACT_SINGLE_MSG = "Both batches to compare exactly must have run with the exact-posterior mode";
static const char *const EXACT_PAIRED_MSG = "Both batches to compare exactly must be paired-end and have run with the paired exact-posterior mode";
void exact_paired_stats6(const miso_batch &b, int i, double *row) {
  const PackedEvent &e = b.events[i];
  const double r[6] = {static_cast<double>(e.base_count[0]), static_cast<double>(e.base_count[1]), e.eff[0], e.eff[1], e.hyper[0], e.hyper[1]};
  std::memcpy(row, r, sizeof r);
}
ExactPairedCmpInput exact_paired_resident(const miso_batch &b, const double *stats6) {
  return ExactPairedCmpInput{stats6, nullptr, nullptr, b.d_events, b.d_in, b.d_fp, static_cast<int>(b.fd.prob.size())};
}

// the guards of every exact pass over the pairs of batch a (sample 1) and batch b (sample 2)
static void exact_pair_guards(const miso_batch &a, const miso_batch &b, bool mode_ok, const char *mode_msg) {
  same_events(a, b, true);
  if (!mode_ok) MISO_FAIL(MISO_EINVAL, mode_msg);
}

// The pairs of an exact pass: the events `take` admits, in order, and their rows of `row_w` statistics from `gather`, batch
// a's in s1 and batch b's in s2.
struct ExactPairs {
  std::vector<int32_t> list;
  std::vector<double> s1, s2;
};
template <class Take, class Gather>
static ExactPairs exact_pairs(const miso_batch &a, const miso_batch &b, int row_w, Take take, Gather gather) {
  ExactPairs x;
  for (int i = 0; i < static_cast<int>(a.events.size()); i++) {
    if (!take(i)) continue;
    x.list.push_back(i);
    x.s1.resize(x.s1.size() + row_w); x.s2.resize(x.s2.size() + row_w);
    gather(a, i, &x.s1[x.s1.size() - row_w]); gather(b, i, &x.s2[x.s2.size() - row_w]);
  }
  return x;
}

// What the two exact comparisons of batch a (sample 1) with batch b (sample 2) share: the guards, the pairs (exact_pairs) of the
// events both batches' exact mode took and that are `comparable`, the call of `run` (which
// validates z, and fails with MISO_ENODEVICE without a device, also when no event is comparable), and the scatter of its rows
// into a's h_exact_cmp / exact_cmp_ok; every other event is marked not comparable.
template <class Comparable, class Gather, class Run>
static void compare_exact_with(miso_batch &a, miso_batch &b, const double *z, int n_z, bool mode_ok, const char *mode_msg, int row_w,
                               Comparable comparable, Gather gather, Run run, const char *kernel) {
  exact_pair_guards(a, b, mode_ok, mode_msg);
  exact_check_z(z, n_z);
  const int n = static_cast<int>(a.events.size());
  a.exact_cmp_ok.assign(n, 0);
  a.exact_delta_done = false;   // (the quantiles of delta psi belong to the comparison this one replaces)
  const ExactPairs x = exact_pairs(a, b, row_w, [&](int i) { return a.event_exact(i) && b.event_exact(i) && comparable(i); }, gather);
  const std::vector<int32_t> &list = x.list;
  const size_t w = 5 + static_cast<size_t>(n_z);
  std::vector<double> got(std::max<size_t>(list.size(), 1) * w);
  HIP_OK(hipSetDevice(a.device));
  HIP_OK(hipStreamSynchronize(b.stream));
  run(x.s1.data(), x.s2.data(), list, got.data());
  a.h_exact_cmp.assign(static_cast<size_t>(n) * w, 0.0);
  for (size_t j = 0; j < list.size(); j++) {
    std::memcpy(&a.h_exact_cmp[list[j] * w], &got[j * w], w * sizeof(double));
    a.exact_cmp_ok[list[j]] = 1;
  }
  a.exact_cmp_nz = n_z;
  if (!list.empty()) a.note_kernel(kernel);
  a.exact_compared = true;
}

// The exact comparison of this batch (sample 1) with `other` (sample 2): the pairs both batches' exact mode took, with
// bit-equal effective lengths, go to exact_compare (kernels_exact_compare.hip).
void miso_batch::compare_exact(miso_batch &other, const double *z, int n_z) {
  compare_exact_with(
      *this, other, z, n_z, exact_single_ok(*this, other), EXACT_SINGLE_MSG, 7,
      [&](int i) { return std::memcmp(events[i].eff.data(), other.events[i].eff.data(), 2 * sizeof(double)) == 0; },
      [](const miso_batch &b, int i, double *row) { b.exact_stats7(i, row); },
      [&](const double *s1, const double *s2, const std::vector<int32_t> &list, double *got) {
        exact_compare_run(s1, s2, static_cast<int>(list.size()), z, n_z, got, stream, &exact_compare_ms);
      },
      "exact_compare");
}

// The exact comparison of two paired-end batches (this one is sample 1): the events both batches' paired exact mode took go
// to exact_paired_compare (kernels_exact_paired_compare.hip), which reads both batches' resident pair records.  The results
// take compare_exact's place (h_exact_cmp, read by the same getter).
void miso_batch::compare_exact_paired(miso_batch &other, const double *z, int n_z) {
  compare_exact_with(
      *this, other, z, n_z, exact_paired_ok(*this, other), EXACT_PAIRED_MSG, 6,
      [](int) { return true; },
      exact_paired_stats6,
      [&](const double *s1, const double *s2, const std::vector<int32_t> &list, double *got) {
        exact_paired_compare_run(exact_paired_resident(*this, s1), exact_paired_resident(other, s2), list.data(),
                                 static_cast<int>(list.size()), z, n_z, got, stream, &exact_compare_ms);
      },
      "exact_paired_compare");
}

// The quantiles of delta psi = psi_1 - psi_2 at prob[0 .. n_p) of exactly the pairs the stored exact comparison of this batch
// (sample 1) found comparable, `other` being sample 2 again: exact_delta_quantiles (kernels_exact_delta.hip) for single-end
// batches, exact_paired_delta_quantiles (kernels_exact_paired_delta.hip) for paired-end ones.  The results are made beside
// the stored ones and take their place at the end: a call that fails leaves what was there.
void miso_batch::exact_delta_quantiles(miso_batch &other, const double *prob, int n_p) {
  const bool paired = p.paired;
  if (paired) exact_pair_guards(*this, other, exact_paired_ok(*this, other), EXACT_PAIRED_MSG);
  else exact_pair_guards(*this, other, exact_single_ok(*this, other), EXACT_SINGLE_MSG);
  if (!exact_compared) MISO_FAIL(MISO_EINVAL, "miso_batch_compare_exact / miso_batch_compare_exact_paired has not run");
  exact_delta_check_p(prob, n_p);
  const int n = static_cast<int>(events.size());
  const ExactPairs x = exact_pairs(
      *this, other, paired ? 6 : 7,
      [&](int i) {
        if (!exact_cmp_ok[i]) return false;
        if (!other.event_exact(i)) MISO_FAIL(MISO_EINVAL, "The second batch is not the one the stored exact comparison was made with");
        return true;
      },
      [&](const miso_batch &b, int i, double *row) { if (paired) exact_paired_stats6(b, i, row); else b.exact_stats7(i, row); });
  const std::vector<int32_t> &list = x.list;
  const size_t w = static_cast<size_t>(n_p) + 1;
  const int m = static_cast<int>(list.size());
  std::vector<double> got(std::max<size_t>(list.size(), 1) * w);
  HIP_OK(hipSetDevice(device));
  HIP_OK(hipStreamSynchronize(other.stream));
  float ms = 0.f;
  if (paired)
    exact_paired_delta_run(exact_paired_resident(*this, x.s1.data()), exact_paired_resident(other, x.s2.data()), list.data(), m, prob,
                           n_p, got.data(), stream, &ms);
  else
    exact_delta_run(x.s1.data(), x.s2.data(), m, prob, n_p, got.data(), stream, &ms);
  std::vector<double> res(static_cast<size_t>(n) * w, 0.0);
  for (size_t j = 0; j < list.size(); j++) std::memcpy(&res[list[j] * w], &got[j * w], w * sizeof(double));
  h_exact_delta.swap(res);
  exact_delta_np = n_p;
  exact_delta_ms = ms;
  if (!list.empty()) note_kernel(paired ? "exact_paired_delta_quantiles" : "exact_delta_quantiles");
  exact_delta_done = true;
}

// A batch that holds posterior samples produced elsewhere -- parsed `.miso` files (summarize_miso / compare_miso
// work on directories of them, misopy/samples_utils.py:263-329, hypothesis_test.py:186-345): event i has K[i] isoforms
// and S samples in the file's layout (rows of K values).  Only the output pool exists; summarize / compare and their
// getters work on it as on a sampled batch.
void miso_batch::adopt_samples(int n, const int *K, int Sn, const double *const *samples, int dev) {
  adopt_pool(n, K, Sn, dev);
  std::vector<unsigned char> h(out_bytes, 0);
  for (int i = 0; i < n; i++) std::memcpy(h.data() + h_events[i].off_samples, samples[i], static_cast<size_t>(Sn) * K[i] * 8);
  HIP_OK(hipMemcpy(d_out, h.data(), out_bytes, hipMemcpyHostToDevice));
}

// The sample pool of such a batch, laid out and allocated but not filled: adopt_samples copies parsed samples into it,
// adopt_text (kernels_text.hip) has the device decode them from the files' text.
void miso_batch::adopt_pool(int n, const int *K, int Sn, int dev) {
  if (uploaded) release();
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device: the summaries have no CPU path");
  if (n < 0 || Sn < 1) MISO_FAIL(MISO_EINVAL, "Invalid number of events or samples");
  device = dev;
  HIP_OK(hipSetDevice(dev));
  events.assign(n, PackedEvent{});
  h_events.assign(n, DevEvent{});
  uint64_t off = 0;
  for (int i = 0; i < n; i++) {
    if (K[i] < 1 || K[i] > MISO_MAX_ISOFORMS) MISO_FAIL(MISO_EINVAL, "Invalid number of isoforms");
    events[i].K = K[i];
    DevEvent &d = h_events[i];
    d.K = K[i];
    d.off_samples = off; off = align_up(off + static_cast<uint64_t>(Sn) * K[i] * 8, 16);
    d.off_trace = NO_TRACE; d.off_dense = d.off_sfixd = NO_DENSE;
  }
  out_bytes = std::max<uint64_t>(off, 16);
  HIP_OK(hipStreamCreate(&stream));
  HIP_OK(hipEventCreate(&ev0));
  HIP_OK(hipEventCreate(&ev1));
  HIP_OK(hipMalloc(reinterpret_cast<void **>(&d_events), std::max<size_t>(n, 1) * sizeof(DevEvent)));
  HIP_OK(hipMalloc(reinterpret_cast<void **>(&d_out), out_bytes));
  if (n) HIP_OK(hipMemcpy(d_events, h_events.data(), n * sizeof(DevEvent), hipMemcpyHostToDevice));
  n_k2 = n_k2w = n_gen = 0; k2[0].count = k2[1].count = 0; gen_runs.clear(); plan = LaunchPlan{};
  uploaded = launched = true; downloaded = false; summarized = compared = exact_compared = pairs_compared = diagnosed = rank_diagnosed = false; adopted = true;
  text_status.clear();
}

void miso_batch::download() {
  if (!launched) MISO_FAIL(MISO_EINVAL, "batch not launched");
  finish_rounds(*this);
  HIP_OK(hipSetDevice(device));
  h_out.resize(out_bytes);
  HIP_OK(hipMemcpy(h_out.data(), d_out, out_bytes, hipMemcpyDeviceToHost));
  downloaded = true;
}

namespace miso {

miso_batch *batch_new(const miso_params_t &p) {
  validate_params(p);
  auto b = std::make_unique<miso_batch>();
  b->p = p;
  if (p.paired) {
    b->fd = normal_fragment(p.normalMean, p.normalVar, p.numDevs, p.readLength);
    // a fragment length is kept as a uint16_t index into fd.prob, FRAG_NONE = none (host.cpp pack_event, match_kernel):
    // every index has to stay below it
    if (b->fd.prob.size() > FRAG_NONE)
      MISO_FAIL(MISO_UNIMPLEMENTED, "Fragment-length distribution wider than 65535 lengths");
  }
  return b.release();
}

void selftest_detmath(const double *x, int n, double *e, double *l, double *s, double *q) {
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device");
  double *d[5];
  for (auto &ptr : d) HIP_OK(hipMalloc(reinterpret_cast<void **>(&ptr), std::max(n, 1) * 8));
  HIP_OK(hipMemcpy(d[0], x, n * 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(selftest_detmath_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, d[0], n, d[1],
                     d[2], d[3], d[4]);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  double *outs[4] = {e, l, s, q};
  for (int i = 0; i < 4; i++) HIP_OK(hipMemcpy(outs[i], d[i + 1], n * 8, hipMemcpyDeviceToHost));
  for (auto ptr : d) (void) hipFree(ptr);
}

void selftest_philox(const uint32_t *in6, int n, uint32_t *out4) {
  if (device_count() <= 0) MISO_FAIL(MISO_ENODEVICE, "no HIP device");
  uint32_t *din, *dout;
  HIP_OK(hipMalloc(reinterpret_cast<void **>(&din), std::max(n, 1) * 24));
  HIP_OK(hipMalloc(reinterpret_cast<void **>(&dout), std::max(n, 1) * 16));
  HIP_OK(hipMemcpy(din, in6, n * 24, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(selftest_philox_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, din, n, dout);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(out4, dout, n * 16, hipMemcpyDeviceToHost));
  (void) hipFree(din); (void) hipFree(dout);
}

}  // namespace miso
