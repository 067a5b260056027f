// launch.hip -- the batch object's launches: the sampler kernels' host stubs with their names, the one call that launches and
// records, the launches that follow the plan launch() made (runtime.hip), and the statistics read back from that plan.
//
// Which kernel a part of a batch takes is decided ONCE: run_kernel() for a general run, plan_k2 for a half of the two-isoform
// list.  The plan keeps the answer (LaunchPlan::Run::kind, K2Half::kind); the launch, the name in last_kernels and the
// record of miso_batch_launch_stats all switch on it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <utility>

#include "batch.hpp"
#include "coop.hpp"
#include "hip_host.hpp"
#include "miso_binomial.h"

namespace miso {

template <bool PE> __global__ void sampler_wave(const KernelArgs a);
template <int G, int MODE, int WPB> __global__ void sampler_k2(const KernelArgs a);
template <int GA, int GB> __global__ void sampler_k2_mix(const KernelArgs a);
template <int MODE, int WPB, bool NARROW = false> __global__ void sampler_k2_multi(const KernelArgs a);
template <bool PE> __global__ void sampler_big(const KernelArgs a);   // kernels_big.hip: 65 ... MISO_MAX_ISOFORMS isoforms
__global__ void sampler_lane(const KernelArgs a);   // kernels_lane.hip: collapsed Gibbs step, one chain per lane
__global__ void sampler_lane_ilp(const KernelArgs a);   // ... the form for at most two wavefronts per SIMD
template <int G> __global__ void sampler_k2c(const KernelArgs a);   // ... G lanes per chain (k2_body COLLAPSED)
__global__ void sampler_lane_k(const KernelArgs a); // ... three and more isoforms (vectors in LDS)
__global__ void sampler_marginal(const KernelArgs a); // kernels_marginal.hip: algorithm = MARGINAL, one chain per lane
__global__ void exact_sample(const KernelArgs a, const double *eff, int S);   // kernels_exact.hip: the exact-posterior mode, one wavefront per event
constexpr int LANEK_VECTORS = 9;
inline size_t lanek_lds_bytes(int ks) { return static_cast<size_t>(LANEK_VECTORS) * ks * 64 * 8 + static_cast<size_t>(ks) * 64 * 4; }
template <int G, bool PE, int KC, bool WIDE = false> __global__ void sampler_grp(const KernelArgs a);
template <int KC> __global__ void sampler_grp_multi(const KernelArgs a);
__global__ void sampler_grp_all(const KernelArgs a);   // kernels_grp_all.hip
template <int KC, int KS, bool UNI> __global__ void sampler_flat(const KernelArgs a);   // KS: the launch's largest isoform count at compile time (0: at run time)

// ---- the shader clock a launch ran at (miso_batch_set_clock_probe; bench.py's roofline prices its VALU peak with it) ----
// ONE wavefront beside the sampler kernels, on a stream of its own: it sleeps, looks at a flag the batch's stream sets
// behind its last kernel, and leaves with the two counters' values at both ends -- s_memtime counts shader cycles,
// wall_clock64() the constant reference clock (hipDeviceAttributeWallClockRate: 100 MHz here) -- so cycles / time over exactly the launch.  No VALU work, no LDS: it
// takes one wave slot of one SIMD.  The flag carries the launch's number (nothing to reset between launches).  It gives up after `max_ticks` of the reference clock (a flag that never comes must
// not hold the device).  out: {t0 real, t0 cycles, t1 real, t1 cycles, 1 = gave up}.
__global__ void clock_probe_kernel(const uint32_t *flag, uint32_t want, unsigned long long *out, unsigned long long max_ticks) {
  if (threadIdx.x != 0) return;
  const unsigned long long r0 = static_cast<unsigned long long>(wall_clock64()), c0 = __builtin_readcyclecounter();
  unsigned long long r1 = r0;
  uint32_t f = 0;
  do {
    __builtin_amdgcn_s_sleep(127);
    f = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    r1 = static_cast<unsigned long long>(wall_clock64());
  } while (f != want && r1 - r0 < max_ticks);
  const unsigned long long c1 = __builtin_readcyclecounter();
  r1 = static_cast<unsigned long long>(wall_clock64());
  out[0] = r0; out[1] = c0; out[2] = r1; out[3] = c1; out[4] = f != want;
}
__global__ void clock_probe_stop(uint32_t *flag, uint32_t value) {
  if (threadIdx.x == 0) __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- the sampler kernels' host stubs with their names, picked by their template arguments ----
// Only the instantiations the kernel units make (kernels_*.hip): a pointer to any other links into the library and fails
// when it is loaded.  A name lists the template arguments as written here, a defaulted trailing `false` left out.
static std::string arg(int x) { return std::to_string(x); }
static std::string arg(bool b) { return b ? "true" : "false"; }
template <class... A> static std::string targs(A... a) { std::string s; ((s += (s.empty() ? "<" : ", ") + arg(a)), ...); return s + ">"; }
// make(std::integral_constant<int, V>) for the listed V that equals v; none does: for the last one (or_last), or no kernel
template <int... V> using Ints = std::integer_sequence<int, V...>;
template <int... V, class F> static Kernel pick(int v, Ints<V...>, F &&make, bool or_last = false) {
  constexpr int list[] = {V...}, last = list[sizeof...(V) - 1];
  Kernel k{nullptr, ""};
  (void) ((v == V || (or_last && V == last) ? (k = make(std::integral_constant<int, V>{}), true) : false) || ...);
  return k;
}

template <int MODE, int WPB> static Kernel k2_kernel(int G) {
  const Kernel k = pick(G, Ints<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 21, 32, 64>{}, [](auto g) {
    constexpr int GG = decltype(g)::value;
    return Kernel{fn(&sampler_k2<GG, MODE, WPB>), "sampler_k2" + targs(GG, MODE, WPB)}; });
  if (!k.fn) MISO_FAIL(MISO_EINVAL, "MISO_LANES_PER_CHAIN must be one of 1-10,12,16,21,32,64");
  return k;
}
// the single-width launch of a half: MODE 2 / MODE 1 (paired-end), MODE 0 on paired 8-wavefront or on 4-wavefront workgroups
static Kernel k2_single_kernel(int mode, bool pair, int G) {
  return mode == 2 ? k2_kernel<2, 4>(G) : mode == 1 ? k2_kernel<1, 4>(G) : pair ? k2_kernel<0, 8>(G) : k2_kernel<0, 4>(G);
}
static Kernel k2_mix_kernel(int G) {   // sampler_k2_mix<G + 1, G>
  return pick(G, Ints<1, 2, 3, 4, 5, 6, 7>{}, [](auto g) {
    constexpr int GG = decltype(g)::value;
    return Kernel{fn(&sampler_k2_mix<GG + 1, GG>), "sampler_k2_mix" + targs(GG + 1, GG)}; }, true);
}
static Kernel k2_multi_kernel(int mode, int wpb, bool narrow) {
  if (mode == 2) return wpb == 8 ? Kernel{fn(&sampler_k2_multi<2, 8>), "sampler_k2_multi<2, 8>"} : Kernel{fn(&sampler_k2_multi<2, 4>), "sampler_k2_multi<2, 4>"};
  if (mode == 1) return {fn(&sampler_k2_multi<1, 4>), "sampler_k2_multi<1, 4>"};
  if (wpb == 8) return {fn(&sampler_k2_multi<0, 8>), "sampler_k2_multi<0, 8>"};
  if (wpb == 4) return narrow ? Kernel{fn(&sampler_k2_multi<0, 4, true>), "sampler_k2_multi<0, 4, true>"} : Kernel{fn(&sampler_k2_multi<0, 4>), "sampler_k2_multi<0, 4>"};
  return {fn(&sampler_k2_multi<0, 1>), "sampler_k2_multi<0, 1>"};
}
static Kernel lane_kernel(int G, bool ilp) {   // the collapsed step: one lane per chain, or G (sampler_k2c)
  if (G == 1) return ilp ? Kernel{fn(&sampler_lane_ilp), "sampler_lane_ilp"} : Kernel{fn(&sampler_lane), "sampler_lane"};
  return pick(G, Ints<2, 4, 8>{}, [](auto g) {
    constexpr int GG = decltype(g)::value;
    return Kernel{fn(&sampler_k2c<GG>), "sampler_k2c" + targs(GG)}; }, true);
}
template <int G, bool PE, bool WIDE = false> static Kernel grp_kc(int kc) {
  return pick(kc, Ints<4, 8, 12, 16, 32>{}, [](auto c) {
    constexpr int KC = decltype(c)::value;
    return Kernel{fn(&sampler_grp<G, PE, KC, WIDE>), "sampler_grp" + (WIDE ? targs(G, PE, KC, true) : targs(G, PE, KC))}; }, true);
}
static Kernel grp_kernel(int G, bool pe, int kc) {   // G < 64
  const Kernel k = pick(G, Ints<2, 4, 8, 16, 32>{}, [&](auto g) {
    constexpr int GG = decltype(g)::value;
    return pe ? grp_kc<GG, true>(kc) : grp_kc<GG, false>(kc); });
  if (!k.fn) MISO_FAIL(MISO_EINVAL, "MISO_GENERAL_LANES must be 2, 4, 8, 16, 32 or 64");
  return k;
}
static Kernel grp_multi_kernel(int kc) {
  return pick(kc, Ints<4, 8, 12, 16, 32>{}, [](auto c) {
    constexpr int KC = decltype(c)::value;
    return Kernel{fn(&sampler_grp_multi<KC>), "sampler_grp_multi" + targs(KC)}; }, true);
}
// ks: the run's largest isoform count at compile time (kc - 3 ... kc, 17 ... 20 for kc = 32), 0 = the layout at run time
template <int KC, int... KS> static Kernel flat_kc(int ks, bool uni, Ints<KS...> counts) {
  const Kernel k = pick(ks, counts, [&](auto c) {
    constexpr int S = decltype(c)::value;
    return uni ? Kernel{fn(&sampler_flat<KC, S, true>), "sampler_flat" + targs(KC, S, true)}
               : Kernel{fn(&sampler_flat<KC, S, false>), "sampler_flat" + targs(KC, S)}; });
  return k.fn ? k : Kernel{fn(&sampler_flat<KC, 0, false>), "sampler_flat" + targs(KC, 0)};
}
static Kernel flat_kernel(int kc, int ks, bool uni) {
  switch (kc) {
  case 4: return flat_kc<4>(ks, uni, Ints<3, 4>{});
  case 8: return flat_kc<8>(ks, uni, Ints<5, 6, 7, 8>{});
  case 12: return flat_kc<12>(ks, uni, Ints<9, 10, 11, 12>{});
  case 16: return flat_kc<16>(ks, uni, Ints<13, 14, 15, 16>{});
  default: return flat_kc<32>(ks, uni, Ints<17, 18, 19, 20>{});
  }
}
static Kernel wave_kernel(bool pe) { return pe ? Kernel{fn(&sampler_wave<true>), "sampler_wave<true>"} : Kernel{fn(&sampler_wave<false>), "sampler_wave<false>"}; }
static Kernel big_kernel(bool pe) { return pe ? Kernel{fn(&sampler_big<true>), "sampler_big<true>"} : Kernel{fn(&sampler_big<false>), "sampler_big<false>"}; }

}  // namespace miso

using namespace miso;

// The kernel of a general run that is launched on its own, with G lanes per chain: the workgroup-wide bucket's, sampler_flat,
// sampler_grp below a wavefront per chain; at a wavefront per chain the dense-record kernel of the one-wavefront bucket
// (only with this launch's dense records: dense_env), else the kernel with a lane per isoform, or with the vectors in LDS
// beyond 64 isoforms.  The plan (plan_runs), the trial launches and the launch (launch_grp) all ask here.
RunKernel miso_batch::run_kernel(const GenRun &run, int G, bool flat, bool dense_env, bool paired) {
  if (run.wide()) return RunKernel::GrpWide;
  if (flat) return RunKernel::Flat;
  if (G != 64) return RunKernel::Grp;
  if (run.wave64() && paired && dense_env && run.dense) return RunKernel::GrpWave64;
  return run.kc > 64 ? RunKernel::Big : RunKernel::Wave;
}

// the stub and name of a kind of general run: isoform-count class kc, the plan's lanes per chain and sampler_flat arguments
Kernel miso_batch::run_kernel_of(RunKernel kind, int kc, const LaunchPlan::Run &r) const {
  switch (kind) {
  case RunKernel::LaneK: return {fn(&sampler_lane_k), "sampler_lane_k"};
  case RunKernel::GrpAll: return {fn(&sampler_grp_all), "sampler_grp_all"};
  case RunKernel::GrpMulti: return grp_multi_kernel(kc);
  case RunKernel::GrpWide: return grp_kc<64, true, true>(kc);
  case RunKernel::GrpWave64: return grp_kc<64, true>(kc);
  case RunKernel::Big: return big_kernel(p.paired);
  case RunKernel::Wave: return wave_kernel(p.paired);
  case RunKernel::Flat: return flat_kernel(kc, r.flat_ks, r.flat_uni);
  case RunKernel::Grp: break;
  }
  return grp_kernel(r.G, p.paired, kc);
}

// ... and of a half of the two-isoform list
Kernel miso_batch::k2_kernel_of(const K2Half &h) const {
  switch (h.kind) {
  case K2Kernel::Lane: return lane_kernel(plan.lane_G, plan.lane_ilp);
  case K2Kernel::Multi: return k2_multi_kernel(h.mode, h.plan.wpb, plan.k2_narrow);
  case K2Kernel::Mix: return k2_mix_kernel(h.G);
  default: return k2_single_kernel(h.mode, plan.k2_pair, h.G);
  }
}

// Every sampler launch: its name into last_kernels (not a trial launch's), the dynamic LDS the kernel may use, the launch
// (what the triple-chevron stub calls too), its check.
void miso_batch::launch_kernel(const Kernel &k, unsigned grid, unsigned block, size_t lds, hipStream_t st, void **args) {
  if (!trial_launch) note_kernel(k.name);
  if (lds) HIP_OK(hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
  (void) hipLaunchKernel(k.fn, dim3(grid), dim3(block), args, lds, st);
  HIP_OK(hipGetLastError());
}
void miso_batch::launch_kernel(const Kernel &k, unsigned grid, unsigned block, size_t lds, hipStream_t st, const KernelArgs &ka) {
  void *args[] = {const_cast<KernelArgs *>(&ka)};
  launch_kernel(k, grid, block, lds, st, args);
}

// algorithm = MARGINAL / CLASSES: one chain per lane, every event of the batch in one launch (kernels_marginal.hip); its
// vectors live in LDS, [vector][isoform][lane], 64 lanes per workgroup up to 32 isoforms, 32 beyond.
void miso_batch::launch_marginal(const KernelArgs &a) {
  const int n = static_cast<int>(events.size());
  int ks = 2;
  for (const PackedEvent &e : events) ks = std::max(ks, e.K);
  const int lanes = ks <= 32 ? 64 : 32;
  KernelArgs ka = a;
  ka.slot_event = d_slots; ka.n_slots = n; ka.kstride = ks;
  const long chains = static_cast<long>(n) * p.noChains;
  const Kernel k{fn(&sampler_marginal), "sampler_marginal"};
  if (chains > 0) launch_kernel(k, static_cast<unsigned>((chains + lanes - 1) / lanes), lanes, marginal_lds_bytes(ks, lanes), stream, ka);
  else last_kernels = k.name;   // (a batch without events: the name of the mode, as ever)
}

// ---- the two-isoform part: sampler_k2<G> and its relatives ----
void miso_batch::launch_k2(KernelArgs ka, const K2Half &h, int G, hipStream_t st) {
  const long chains = static_cast<long>(h.count) * p.noChains;
  if (chains <= 0) return;
  ka.slot_event = d_slots + h.first; ka.n_slots = h.count;
  const int cpw = 64 / std::max(G, 1);
  const long waves = (chains + cpw - 1) / cpw;
  // single-end: workgroups of 8 wavefronts = one CU's resident slots; the two wavefronts of a SIMD
  // take a heavy and a light group of chains (sampler_k2's WPB = 8); knobs.k2_pair off: the 4-wavefront
  // workgroups in slot order (round-1 behaviour).
  const bool pair = plan.k2_pair;
  ka.pair_waves = pair ? 1 : 0;
  const unsigned grid = static_cast<unsigned>(pair ? (waves + 7) / 8 : (waves + 3) / 4);
  const size_t k2_lds = h.fp + 4 * static_cast<size_t>(cpw) * h.tab;
  if (k2_lds > 160 * 1024) MISO_FAIL(MISO_UNIMPLEMENTED, "Fragment-length distribution too wide for the two-isoform paired-end kernel");
  launch_kernel(k2_single_kernel(h.mode, pair, G), grid, !p.paired && pair ? 512 : 256, k2_lds, st, ka);
}

void miso_batch::launch_k2_mix(KernelArgs ka, hipStream_t st) {
  const K2Half &h = k2[1];
  const int C = p.noChains, G = h.G, cpwB = 64 / G;
  ka.slot_event = d_slots + h.first; ka.n_slots = h.count;
  ka.pair_waves = 1; ka.mix_slots = plan.k2_mix; ka.mix_blocks = plan.k2_mix_blocks;
  const long wavesB = (static_cast<long>(h.count - plan.k2_mix) * C + cpwB - 1) / cpwB;
  launch_kernel(k2_kernel_of(h), static_cast<unsigned>(plan.k2_mix_blocks + (wavesB + 7) / 8), 512, 0, st, ka);
}

// which chain every workgroup of a half's workgroup-wide run works on (coop.hpp); nothing to do when every chain
// has its workgroup to itself
void miso_batch::k2_coop(KernelArgs &ka, K2Half &h, hipStream_t st) {
  const LanePlan &pl = h.plan;
  CoopTable &cc = h.coop;
  ka.coop_tab = nullptr; ka.coop_mem = nullptr;
  if (pl.n_segs == 0 || pl.seg_lanes[0] != K2_WIDE) return;
  bool any = false;
  for (int m : pl.wide_wgs) any |= m > 1;
  if (!any) return;
  const long key = pl.seg_block[1] * 131 + static_cast<long>(pl.wide_wgs.size());
  if (cc.tab.key != key || !cc.tab.d) {
    std::vector<int32_t> tab;
    cc.chains = 0;
    for (size_t e = 0; e < pl.wide_wgs.size(); e++)
      for (int c = 0; c < p.noChains; c++) {
        const int m = pl.wide_wgs[e];
        for (int r = 0; r < m; r++) { tab.push_back(static_cast<int32_t>(e * p.noChains + c)); tab.push_back(r); tab.push_back(m); tab.push_back(m > 1 ? cc.chains : 0); }
        if (m > 1) cc.chains++;
      }
    if (static_cast<int>(tab.size() / 4) != pl.seg_block[1]) MISO_FAIL(MISO_EINTERNAL, "lane plan and cooperative table disagree");
    put(cc.tab, tab);
    put(cc.mem, {}, static_cast<size_t>(std::max(1, cc.chains)) * COOP_WORDS);
    cc.tab.key = key;
  }
  HIP_OK(hipMemsetAsync(cc.mem.d, 0, std::max(1, cc.chains) * COOP_WORDS * sizeof(uint32_t), st));
  ka.coop_tab = cc.tab.d; ka.coop_mem = cc.mem.d;
}

void miso_batch::launch_k2_multi(KernelArgs ka, K2Half &h, hipStream_t st) {
  const LanePlan &pl = h.plan;
  k2_coop(ka, h, st);
  ka.slot_event = d_slots + h.first; ka.n_slots = h.count;
  ka.n_segs = pl.n_segs;
  for (int i = 0; i <= pl.n_segs; i++) { ka.seg_block[i] = pl.seg_block[i]; ka.seg_slot[i] = pl.seg_slot[i]; }
  for (int i = 0; i < pl.n_segs; i++) ka.seg_lanes[i] = pl.seg_lanes[i];
  unsigned grid = static_cast<unsigned>(pl.seg_block[pl.n_segs]);
  const Kernel k = k2_kernel_of(h);
  if (p.paired) {   // MODE 2, MODE 1: the probabilities and, per chain of the workgroup's wavefronts, its score table; the reduction scratch behind them
    int cpw = 1;
    for (int i = 0; i < pl.n_segs; i++) if (pl.seg_lanes[i] != K2_WIDE) cpw = std::max(cpw, 64 / pl.seg_lanes[i]);
    const size_t tabs = align_up(h.fp + static_cast<size_t>(pl.wpb) * cpw * h.tab, 16);
    ka.pair_waves = 0;
    ka.red_off = static_cast<int32_t>(tabs);
    launch_kernel(k, grid, 64 * pl.wpb, tabs + K2_RED_BYTES, st, ka);
    return;
  }
  ka.pair_waves = (pl.rounds == 1 && pl.wpb == 8) ? 1 : 0;
  ka.red_off = 0;
  if (pl.wpb == 8 && k2_pair_grid > 0 && !k2_pair_tab.host.empty()) {   // wavefronts paired across the runs
    ka.wave_tab = k2_pair_tab.d; ka.mix_blocks = k2_pair_wide_blocks; ka.pair_waves = 0;
    grid = static_cast<unsigned>(k2_pair_grid);
  }
  // the whole launch resident at once: the two wavefronts of a SIMD keep step (kernels_k2.inl k2_balance)
  if (pl.wpb == 8 && pl.rounds == 1) ka.balance = knobs.k2_balance.off() ? 0 : 1;
  const int wpb = pl.wpb == 8 || pl.wpb == 4 ? pl.wpb : 1;
  launch_kernel(k, grid, 64 * wpb, wpb == 1 ? 0 : K2_RED_BYTES, st, ka);
}

// collapsed single-end batch: one chain per lane, no read loop (kernels_lane.hip)
void miso_batch::launch_lane(KernelArgs ka, hipStream_t st) {
  ka.slot_event = d_slots; ka.n_slots = n_k2; ka.pair_waves = 0;
  ka.logfact = logfact.d; ka.tstride = static_cast<int32_t>(logfact.host.size());   // (tstride: the table's entries, for sampler_lane_ilp's LDS copy)
  const long chains = static_cast<long>(n_k2) * p.noChains;
  const int G = plan.lane_G;
  unsigned grid = static_cast<unsigned>(((chains + 64 / G - 1) / (64 / G) + 3) / 4);
  if (G == 1) {
    grid = static_cast<unsigned>((chains + 255) / 256);
    // fewer wavefronts than SIMDs (or than two per SIMD): spread the chains over all of them (kernels_lane.hip lane_body)
    const long simds = wave_slots / 2, waves = (chains + 63) / 64;
    const int per_simd = knobs.lane_spread.v;
    if (plan.lane_ilp && per_simd > 0 && waves < simds * per_simd && chains >= 64) {
      const long target = simds * per_simd;
      const int cpw = static_cast<int>((chains + target - 1) / target);
      if (cpw >= 8 && cpw < 64) { ka.pair_waves = cpw; grid = static_cast<unsigned>(((chains + cpw - 1) / cpw + 3) / 4); }
    }
  }
  launch_kernel(k2_kernel_of(k2[1]), grid, 256, 0, st, ka);
}

// ---- more than two isoforms: sampler_grp<G, PE, KC> per isoform-count class ----
// Workgroup-wide chains of a run: which chain every workgroup works on (coop.hpp), built once per batch; returns the
// number of workgroups.
unsigned miso_batch::wide_setup(GenRun &run, long chains, hipStream_t st) {
  // Workgroups per chain: what upload() derived from the gene's share of the batch's work (coop_n), at most
  // COOP_MAX_N, all cooperative workgroups of the batch together at most COOP_MAX_WGS (coop.hpp: they must all be
  // resident at once).  knobs.no_coop: one workgroup per chain; knobs.coop_draws: one per n drawing pairs.
  CoopTable &cc = run.coop;
  if (!cc.tab.d) {
    std::vector<int32_t> tab;
    cc.chains = 0;
    const bool coop_on = coop_enabled();
    const int per_wg = knobs.coop_draws.v;
    for (long c = 0; c < chains; c++) {
      const int ev_i = h_slots[n_k2 + run.first + c / p.noChains];
      const int nd = events[ev_i].n_draw;
      int nw = !coop_on ? 1 : (knobs.coop_draws.set ? std::min(COOP_MAX_N, std::max(1, (nd + per_wg - 1) / per_wg)) : coop_n[ev_i]);
      if (nw > 1 && coop_wgs_used + nw > coop_gen_budget) nw = std::max(1, coop_gen_budget - coop_wgs_used);
      if (nw > 1) coop_wgs_used += nw;
      for (int r = 0; r < nw; r++) {
        tab.push_back(static_cast<int32_t>(c)); tab.push_back(r); tab.push_back(nw);
        tab.push_back(nw > 1 ? cc.chains : 0);
      }
      if (nw > 1) cc.chains++;
    }
    if (knobs.timing) {
      std::fprintf(stderr, "[miso] wide run kc=%d: %ld chains on %zu workgroups (%d on several:", run.kc, chains, tab.size() / 4, cc.chains);
      for (size_t i = 0; i < tab.size(); i += 4)
        if (tab[i + 1] == 0 && tab[i + 2] > 1)
          std::fprintf(stderr, " %d x %d draws K=%d", tab[i + 2], events[h_slots[n_k2 + run.first + tab[i] / p.noChains]].n_draw,
                       events[h_slots[n_k2 + run.first + tab[i] / p.noChains]].K);
      std::fprintf(stderr, ")\n");
    }
    put(cc.tab, tab);
    put(cc.mem, {}, static_cast<size_t>(std::max(1, cc.chains)) * COOP_WORDS);
  }
  HIP_OK(hipMemsetAsync(cc.mem.d, 0, std::max(1, cc.chains) * COOP_WORDS * sizeof(uint32_t), st));
  return static_cast<unsigned>(cc.tab.host.size() / 4);
}

void miso_batch::launch_grp(KernelArgs ka, GenRun &run, const GrpShape &sh, int G, hipStream_t st) {
  const long chains = static_cast<long>(run.count) * p.noChains;
  ka.slot_event = d_slots + n_k2 + run.first; ka.n_slots = run.count;
  ka.kstride = run.kmax; ka.cstride = sh.qs; ka.tstride = sh.ts;
  const RunKernel kind = run_kernel(run, G, false, plan.dense_env, p.paired != 0);
  LaunchPlan::Run r;
  r.G = G;
  const bool lane_per_isoform = kind == RunKernel::Wave || kind == RunKernel::Big;   // plain records, plain probabilities
  ka.pe_dense = lane_per_isoform ? 0 : fp_rows(run);
  const size_t fp_bytes = lane_per_isoform ? plan.fp_plain : fp_bytes_of(run);
  unsigned grid = static_cast<unsigned>((chains + 3) / 4), block = 256;   // a wavefront per chain
  size_t lds = 0;
  switch (kind) {
  case RunKernel::GrpWide:   // one chain per workgroup: four slices (one per wavefront) + the reduction scratch behind them
    if (!ka.pe_dense) MISO_FAIL(MISO_EINTERNAL, "workgroup-wide paired-end chains need the dense records");
    lds = align_up(fp_bytes + 4 * static_cast<size_t>(grp_slice_bytes(run.kmax, 0, sh.ts)), 16);
    ka.red_off = static_cast<int32_t>(lds);
    lds += 96;
    grid = wide_setup(run, chains, st);
    ka.coop_tab = run.coop.tab.d; ka.coop_mem = run.coop.mem.d;
    break;
  case RunKernel::GrpWave64:   // dense records (size bucket between 32 lanes and a workgroup)
    lds = fp_bytes + 4 * static_cast<size_t>(grp_slice_bytes(run.kmax, sh.qs, sh.ts));
    break;
  case RunKernel::Big:   // 65 ... MISO_MAX_ISOFORMS isoforms: one wavefront = one workgroup per chain, vectors in LDS (kernels_big.hip)
    lds = fp_bytes + static_cast<size_t>(run.kmax) * (11 * sizeof(double) + 2 * sizeof(int));
    grid = static_cast<unsigned>(chains); block = 64;
    break;
  case RunKernel::Wave:
    lds = fp_bytes + 4 * 64 * sizeof(int);
    break;
  default: {
    const int cpw = 64 / G;
    grid = static_cast<unsigned>(((chains + cpw - 1) / cpw + 3) / 4);
    lds = fp_bytes + 4 * static_cast<size_t>(cpw) * grp_slice_bytes(run.kmax, sh.qs, sh.ts);
  }
  }
  launch_kernel(run_kernel_of(kind, run.kc, r), grid, block, lds, st, ka);
}

// Which chains a wavefront of sampler_flat owns (kernels_flat.inl: a.wave_tab).  Uniform batches: `nc` consecutive
// chains each.  When the batch's events differ widely in size -- the heaviest wavefront of the uniform rule would
// carry more than twice the average wavefront's work units -- the wavefronts are packed by UNITS instead: as many
// consecutive chains (at most nc_max: the LDS) as make about the average wavefront's units, a chain of several
// times that alone in a WORKGROUP (FLAT_WIDE: 256 lanes), workgroups ordered heaviest first (the hardware starts
// them in index order); knobs.flat_pack: never / always.
// How many units per wavefront: as many as nc_max average chains have -- the scalar step costs a wavefront the same
// for 2 chains and for 13, so fewer, fuller wavefronts win (hg19-like read counts, 40 000 events, K = 5: 497 ms at 8
// average chains per wavefront, 425 ms at 13+) -- unless that leaves the device part empty: fewer wavefronts than
// resident slots, or a second round that is less than half full (K = 3: 3349 wavefronts on 3072 slots 286 ms,
// 5704 wavefronts 270 ms); then the wavefront count goes to 0.95 x one or two rounds
// (profiles/r03_flat_pack_sweep.txt).  A forced knobs.flat_nc sets the average chains per wavefront instead.
void miso_batch::flat_waves(GenRun &run, int nc, int nc_max_u, long resident_u, int nc_max_p, long resident_p) {
  const long chains = static_cast<long>(run.count) * p.noChains;
  const int C = p.noChains;
  const Opt<int> &fpack = knobs.flat_pack;
  const long ov_pct = knobs.flat_pack_ov.v;   // (per cent of the rule below)
  const long key = (((static_cast<long>(nc) * 4 + (fpack.set ? 1 + (fpack.v != 0) : 0)) * 128 + nc_max_u) * 128 + nc_max_p) * 1024 + (knobs.flat_pack_ov.set ? 1 + ov_pct % 1000 : 0);
  if (run.wave_tab.key == key && run.wave_tab.d) return;
  // (round 5) what a chain costs its wavefront, in work units: its units + the scalar step and thresholds, which do not
  // depend on the reads.  Measured per chain-iteration at eight / five chains per wavefront (profiles/r05_flat_chunks.txt):
  // K = 5 238 VALU against 1.33 per unit, K = 10 641 against 1.96, i.e. about 30 K + 25 units -- but the wavefronts this
  // matters for carry 14 - 18 small chains, whose flat passes and leader sections are shared by twice as many chains:
  // 16 K + 14.  Swept on hg19-like read counts at 25 ... 300 % of the first figure: K = 3 / 4 / 6 / 8 best at 50 % (208 /
  // 152 / 107 / 80 k events/s against 153 / 144 / 97 / 74 k at 100 %), K = 5 / 12 at 100 % (122 / 45 k against 114 / 43 k);
  // by units alone: 151 / 112 / 55 k at K = 3 / 5 / 10.
  auto units_of = [&](long c) {
    const PackedEvent &e = events[h_slots[n_k2 + run.first + c / C]];
    return static_cast<long>(e.n_units) + (16L * e.K + 14) * ov_pct / 100;
  };
  long total = 0, head = 0;
  for (long c = 0; c < chains; c++) { const long u = units_of(c); total += u; if (c < nc) head += u; }
  long heaviest = head;   // the list is ordered by isoforms first: look at every wavefront of the uniform rule
  for (long c = 0, sum = 0; c < chains; c++) {
    sum += units_of(c);
    if ((c + 1) % nc == 0 || c + 1 == chains) { heaviest = std::max(heaviest, sum); sum = 0; }
  }
  const double mean_wave = static_cast<double>(total) * nc / std::max<long>(1, chains);
  const bool pack = fpack.set ? fpack.v != 0 : (chains > nc && static_cast<double>(heaviest) > 2.0 * mean_wave);
  struct W { int32_t first, n; long units; };
  std::vector<W> waves, wides;
  if (!pack) {
    for (long c = 0; c < chains; c += nc) waves.push_back(W{static_cast<int32_t>(c), static_cast<int32_t>(std::min<long>(nc, chains - c)), 0});
    run.wave_nc = nc;
  } else {
    // (packed launches have their own sizing: launch_flat)
    const int nc_max = nc_max_p; const long resident = resident_p;
    const int cap = std::min(nc_max, 255);
    int most = 1;
    auto pack_with = [&](double U) {
      waves.clear(); wides.clear(); most = 1;
      const double wide_min = std::max(3.0 * U, 2048.0);
      for (long c = 0; c < chains;) {
        const long u = units_of(c);
        if (static_cast<double>(u) >= wide_min) { wides.push_back(W{static_cast<int32_t>(c), 1, u}); c++; continue; }
        W w{static_cast<int32_t>(c), 0, 0};
        while (c < chains && w.n < cap) {
          const long v = units_of(c);
          if (static_cast<double>(v) >= wide_min || (w.n > 0 && static_cast<double>(w.units + v) > 1.05 * U)) break;
          w.units += v; w.n++; c++;
        }
        most = std::max(most, static_cast<int>(w.n));
        waves.push_back(w);
      }
      return static_cast<long>(waves.size() + 4 * wides.size());
    };
    const double per_chain = static_cast<double>(total) / std::max<long>(1, chains);
    const bool forced = knobs.flat_nc.set;
    const long n_waves = pack_with(std::max(64.0, per_chain * (forced ? nc : cap)));
    if (!forced && n_waves < 3 * resident / 2) {
      // (round 6) ... and TWO rounds are aimed at from further below than one: the second round's workgroups start as the
      // first round's end, staggered, and a count within a few per cent of two full rounds runs into a third (hg19-like read
      // counts, K = 5, 2048 resident wavefronts: 4029 wavefronts 71.7 ms, 3793 64.6 ms, 3541 66.2 ms, 2956 -- the fullest
      // packing -- 67.7 ms; profiles/r06_flat_pack_rounds.txt): knobs.flat_rounds_frac.
      const bool two = n_waves > resident;
      const double frac2 = knobs.flat_rounds_frac.v;
      const double want = (two ? frac2 : 0.95) * static_cast<double>(two ? 2 * resident : resident);
      if (static_cast<double>(n_waves) < want) {
        // (round 5) ... and not a few wavefronts MORE than the round(s): the packing's bound is a target, the count it
        // makes lands some per cent off, and 3110 wavefronts on 3072 slots cost a second round for 38 of them
        // (K = 3, hg19-like read counts: 154 k events/s there, 212 k at 2960; profiles/r05_flat_chunks.txt)
        const long target = two ? static_cast<long>((frac2 + 0.04) * 2.0 * static_cast<double>(resident)) : resident;
        double U2 = std::max(64.0, static_cast<double>(total) / want);
        long n2 = pack_with(U2);
        for (int it = 0; it < 8 && n2 > target; it++) {
          const long before = n2;
          U2 *= static_cast<double>(n2) / (0.97 * static_cast<double>(target));
          n2 = pack_with(U2);
          if (n2 >= before) break;   // the chains per wavefront are at the LDS's limit: fuller wavefronts are not to be had
        }
      }
    }
    if (knobs.timing)
      std::fprintf(stderr, "[flat_waves] kc %d chains %ld cost/chain %.1f cap %d resident %ld first pack %ld waves -> %zu waves + %zu wide, most chains %d\n",
                   run.kc, chains, per_chain, cap, resident, n_waves, waves.size(), wides.size(), most);
    std::stable_sort(wides.begin(), wides.end(), [](const W &x, const W &y) { return x.units > y.units; });
    std::stable_sort(waves.begin(), waves.end(), [](const W &x, const W &y) { return x.units > y.units; });
    run.wave_nc = most;
  }
  std::vector<int32_t> tab;
  for (const W &w : wides) for (int i = 0; i < 4; i++) { tab.push_back(w.first); tab.push_back(1 | FLAT_WIDE); }
  for (const W &w : waves) { tab.push_back(w.first); tab.push_back(w.n); }
  while ((tab.size() / 2) % 4) { tab.push_back(0); tab.push_back(0); }   // padding wavefronts
  run.wave_wide = static_cast<int>(wides.size());
  run.wave_packed = pack;
  put(run.wave_tab, tab, 2);
  run.wave_tab.key = key;
}

// Workgroups per CU a run of sampler_flat is sized for: kernels_flat.inl's register budgets -- 3 up to four isoforms and for
// nine to twelve (measured round 4, profiles/r04_occupancy.txt), 2 otherwise (five to eight isoforms: the kernel allows 3,
// sizing for 3 gained nothing) -- unless knobs.flat_wgs says otherwise.
static inline int flat_wgs_for(int kc) { return kc <= 4 ? 3 : (kc == 12 ? 3 : 2); }
int miso_batch::flat_wgs(int kc) const { return knobs.flat_wgs.set ? knobs.flat_wgs.v : flat_wgs_for(kc); }

void miso_batch::launch_flat(KernelArgs ka, size_t ri, hipStream_t st) {
  GenRun &run = gen_runs[ri];
  const int nc = plan.runs[ri].flat_nc, nc_max = plan.runs[ri].flat_nc_max;
  {
    const long chains = static_cast<long>(run.count) * p.noChains;
    const int wgs = flat_wgs(run.kc);
    // Five to eight isoforms: the kernel's registers allow three workgroups per CU; launches of like-sized events are sized for
    // two (fuller wavefronts: K = 6 312 against 333 ms, K = 7 347 / 366), launches packed by cost for three -- more, smaller
    // wavefronts level the heavy tail better than fuller ones amortise the scalar step (hg19-like read counts, 40 000 events:
    // K = 5 276 -> 252 ms, K = 6 332 -> 278, K = 7 379 -> 339, K = 8 415 -> 393; profiles/r06_flat_licm.txt)
    int wgs_p = wgs, nc_max_p = nc_max;
    if (run.kc == 8 && !knobs.flat_wgs.set && !knobs.lds_max_kb.set && !knobs.flat_pack_wgs2) {
      wgs_p = 3;
      const int slice = flat_layout(run.kmax, std::max(run.maxcls, 1)).bytes;
      nc_max_p = std::max(1, std::min<int>(64, static_cast<int>(160 * 1024 / (4 * wgs_p) - 64) / slice));
    }
    flat_waves(run, nc, nc_max, std::max<long>(1, static_cast<long>(slots_for(chains)) * wgs / 2),
               nc_max_p, std::max<long>(1, static_cast<long>(slots_for(chains)) * wgs_p / 2));
  }
  ka.slot_event = d_slots + n_k2 + run.first; ka.n_slots = run.count;
  ka.kstride = run.kmax; ka.cstride = std::max(run.maxcls, 1); ka.tstride = 0; ka.nc = run.wave_nc;
  ka.wave_tab = run.wave_tab.d;
  // the descriptor read loop from four isoforms on (three: the walking loop is 2 % faster -- two thresholds per unit,
  // little to save) and whenever a chain owns a whole workgroup
  ka.flat_desc = ((!knobs.flat_no_desc && run.kmax >= 4) || run.wave_wide > 0) ? 1 : 0;
  // Thresholds only for the chains whose psi changed (kernels_flat.inl): the pass is one lane per (chain, class) and the
  // Metropolis-Hastings step rejects 45 - 65 % of the proposals, but numbering the chains that accepted costs every lane
  // a few instructions -- it pays where the thresholds weigh enough: from six isoforms on (K = 6 ... 12: + 4.5 ... 6.4 %)
  // and for small events (hg19-like read counts at K = 5: + 5.5 %; 1000 reads per event at K = 3 ... 5: - 1 ... 2 %,
  // profiles/r04_occupancy.txt); knobs.flat_thr_skip: never / always.
  {
    double units = 0;
    for (int j = 0; j < run.count; j++) units += events[h_slots[n_k2 + run.first + j]].n_units;
    ka.flat_thr_skip = knobs.flat_thr_skip.set ? (knobs.flat_thr_skip.v != 0) : (run.kmax >= 6 || units < 150.0 * run.count);
  }
  const unsigned grid = static_cast<unsigned>(run.wave_tab.host.size() / 8);
  const size_t lds = 4 * static_cast<size_t>(run.wave_nc) * flat_layout(ka.kstride, ka.cstride).bytes;
  // Priority by progress (device.hpp prio_by_progress) when the launch takes several rounds of like-sized wavefronts:
  // 40 000 events x 1000 reads, K = 5 348.0 -> 334.4 ms, K = 10 649.4 -> 631.4 ms, same box; wavefronts packed by cost
  // (hg19-like read counts) lose 1 % and keep the arbiter's own order; so do the paired-end and the two-isoform kernels
  // (+ 0.5 ... 4 %: profiles/r06_prio_by_progress.txt); knobs.prio_quartiles set: never here / everywhere (launch()).
  if (!knobs.prio_quartiles.set && !run.wave_packed && run.wave_wide == 0 &&
      static_cast<long>(grid) * 4 > static_cast<long>(slots_for(static_cast<long>(run.count) * p.noChains)) * flat_wgs_for(run.kc) / 2)
    ka.balance = 2;
  launch_kernel(run_kernel_of(RunKernel::Flat, run.kc, plan.runs[ri]), grid, 256, lds, st, ka);
}

// kernel i > 0 goes to its own stream, forked from and joined back into the batch's stream
hipStream_t miso_batch::stream_for_next() {
  const size_t i = kernel_no++;
  if (i == 0 || knobs.serial_kernels) return stream;
  while (aux_streams.size() < i) {
    hipStream_t st; hipEvent_t e;
    // (numerically lower = higher priority; the range has three levels on this device: the second and third kernel
    // of a launch at the middle one, the rest at the lowest)
    const int n_aux = static_cast<int>(aux_streams.size());
    const int pr = prio_hi == prio_lo ? prio_lo : std::min(prio_lo, prio_hi + 1 + n_aux / 2);
    if (prio_hi != prio_lo) HIP_OK(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, pr));
    else HIP_OK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    aux_streams.push_back(st); aux_done.push_back(e);
  }
  HIP_OK(hipStreamWaitEvent(aux_streams[i - 1], ev0, 0));
  return aux_streams[i - 1];
}

// The launches, in this order (the stream and priority every kernel gets follow from it): sampler_lane_k, the
// workgroup-wide runs (chains on several workgroups first: their workgroups must all be resident at once, coop.hpp,
// which the idle device guarantees; what is launched after them never waits for them) -- sampler_grp_all or the
// classes' sampler_grp_multi, then the runs of their own --, MODE 2, the other two-isoform events, the other runs.
void miso_batch::launch_planned(const KernelArgs &a, const KernelArgs &k2a) {
  const LaunchPlan &q = plan;
  if (q.lane_route || q.lane_gen) {   // log factorials (miso_binomial.h) up to the largest event's drawing reads
    size_t need = 2;
    for (int i = 0; i < n_k2 + n_gen; i++) need = std::max<size_t>(need, events[h_slots[i]].n_draw + 2);
    if (need > logfact.host.size()) {
      std::vector<double> lf(need);
      miso_logfact_fill(lf.data(), static_cast<int>(need));
      HIP_OK(hipStreamSynchronize(stream));   // (an earlier launch of this batch may still read the old table)
      put(logfact, lf);
    }
  }
  for (size_t ri = 0; ri < gen_runs.size(); ri++) {
    if (!q.runs[ri].lane()) continue;
    const GenRun &run = gen_runs[ri];
    const int ks = std::max(2, run.kmax);
    KernelArgs ka = a;
    ka.slot_event = d_slots + n_k2 + run.first; ka.n_slots = run.count; ka.kstride = ks; ka.logfact = logfact.d;
    const long chains = static_cast<long>(run.count) * p.noChains;
    launch_kernel(run_kernel_of(RunKernel::LaneK, run.kc, q.runs[ri]), static_cast<unsigned>((chains + 63) / 64), 64, lanek_lds_bytes(ks), stream_for_next(), ka);
  }
  if (q.grp_all) launch_grp_all(a);
  for (const auto &g : q.multi) launch_grp_multi(a, g.first, g.second);
  for (size_t ri = 0; ri < gen_runs.size(); ri++) if (q.runs[ri].kind == RunKernel::GrpWide) launch_run(a, ri);
  for (K2Half &h : k2) {
    if (h.count <= 0) continue;
    hipStream_t st = stream_for_next();
    switch (h.kind) {
    case K2Kernel::Lane: lanes_per_chain = q.lane_G; launch_lane(k2a, st); break;
    case K2Kernel::Multi: lanes_per_chain = h.plan.seg_lanes[h.plan.n_segs - 1]; launch_k2_multi(k2a, h, st); break;
    case K2Kernel::Mix: lanes_per_chain = h.G; launch_k2_mix(k2a, st); break;
    default: lanes_per_chain = h.G; launch_k2(k2a, h, h.G, st);
    }
  }
  for (size_t ri = 0; ri < gen_runs.size(); ri++) {
    const RunKernel kind = q.runs[ri].kind;
    if (kind != RunKernel::GrpWide && kind != RunKernel::LaneK && !q.runs[ri].grouped()) launch_run(a, ri);
  }
}

// The exact-posterior mode's events (kernels_exact.hip): one wavefront each, no chains; the launch's last kernel, on the
// next of its streams (the batch's own when the samplers' plan is empty).
static Kernel exact_kernel(bool paired) {
  return paired ? Kernel{exact_paired_sample_fn(), "exact_paired_sample"} : Kernel{fn(&exact_sample), "exact_sample"};
}
void miso_batch::launch_exact(const KernelArgs &a) {
  KernelArgs ka = a;
  ka.slot_event = d_slots + n_k2 + n_gen; ka.n_slots = n_exact;
  const double *eff = exact_eff.d;
  int Sn = S();
  void *args[] = {&ka, &eff, &Sn};
  launch_kernel(exact_kernel(p.paired != 0), static_cast<unsigned>(n_exact), 64, 0, stream_for_next(), args);
}

// general run ri in a launch of its own, or with the next run (merge_next); nothing when the run before took it
void miso_batch::launch_run(const KernelArgs &a, size_t ri) {
  const LaunchPlan::Run &r = plan.runs[ri];
  if (ri > 0 && plan.runs[ri - 1].merge_next) return;
  if (r.merge_next) {
    GenRun m = joined_run(ri, ri + 2);
    launch_grp(a, m, grp_shape(m), r.G, stream_for_next());
  } else if (r.kind == RunKernel::Flat) {
    launch_flat(a, ri, stream_for_next());
  } else {
    launch_grp(a, gen_runs[ri], r.sh, r.G, stream_for_next());
  }
}

void miso_batch::launch_grp_all(const KernelArgs &a) {
  struct Seg { size_t ri; int e0, e1; double cost; };
  std::vector<Seg> segs;
  // (a segment per isoform count, so that no wavefront carries two -- see sampler_grp_multi below; knobs.pe_all_order: other orders)
  const int order = knobs.pe_all_order.v;
  for (size_t ri = 0; ri < gen_runs.size(); ri++) {
    const GenRun &run = gen_runs[ri];
    if (order == 0) { segs.push_back(Seg{ri, 0, run.count, (static_cast<double>(run.maxq) / 16.0 + 8.0) * (run.kmax + 2)}); continue; }
    auto cost_at = [&](int e) {
      const PackedEvent &ev = events[h_slots[n_k2 + run.first + e]];
      return (static_cast<double>((ev.n_draw + 3) / 4) / 16.0 + 8.0) * (ev.K + 2);
    };
    int e0 = 0;   // pieces: one per isoform count
    for (int e = 1; e <= run.count; e++)
      if (e == run.count || events[h_slots[n_k2 + run.first + e]].K != events[h_slots[n_k2 + run.first + e0]].K) { segs.push_back(Seg{ri, e0, e, cost_at(e0)}); e0 = e; }
  }
  std::stable_sort(segs.begin(), segs.end(), [&](const Seg &x, const Seg &y) { return x.cost > y.cost; });
  if (order == 2) {   // heaviest, lightest, second heaviest, second lightest, ...
    std::vector<Seg> t;
    for (size_t i = 0, j = segs.size(); i < j;) { t.push_back(segs[i++]); if (i < j) t.push_back(segs[--j]); }
    segs = t;
  }
  if (order == 3) std::reverse(segs.begin(), segs.end());   // lightest first
  KernelArgs ka = a;
  hipStream_t st = stream_for_next();
  ka.slot_event = d_slots + n_k2; ka.n_slots = n_gen;
  ka.cstride = 0; ka.pe_dense = 1;
  size_t lds = 0; int blocks = 0;
  std::vector<GrpSeg> tab;
  for (const Seg &sg : segs) {
    const GenRun &run = gen_runs[sg.ri];
    const GrpShape &sh = plan.runs[sg.ri].sh;
    const long chains = static_cast<long>(sg.e1 - sg.e0) * p.noChains;
    GrpSeg g{};
    g.block0 = blocks; g.slot0 = run.first + sg.e0; g.n_slots = sg.e1 - sg.e0; g.kc = run.kc;
    g.kstride = run.kmax; g.tstride = sh.ts;
    lds = std::max(lds, fp_bytes_of(run) + 4 * 4 * static_cast<size_t>(grp_slice_bytes(run.kmax, 0, sh.ts)));
    blocks += static_cast<int>(((chains + 3) / 4 + 3) / 4);
    tab.push_back(g);
  }
  GrpSeg sentinel{}; sentinel.block0 = blocks;
  tab.push_back(sentinel);
  if (lds > plan.lds_max) MISO_FAIL(MISO_EINTERNAL, "sampler_grp_all: a segment's slices exceed the workgroup's LDS");
  // (uploaded when it changed: the batch's first launch, or another upload's events; the launch that read the old one has
  // been waited for by then)
  constexpr size_t GRP_SEGS_CAP = 256;
  if (tab.size() > GRP_SEGS_CAP) MISO_FAIL(MISO_EINTERNAL, "sampler_grp_all: too many segments");
  put(grp_segs, tab, GRP_SEGS_CAP);
  ka.grp_segs = grp_segs.d; ka.n_grp_segs = static_cast<int32_t>(segs.size());
  launch_kernel(run_kernel_of(RunKernel::GrpAll, 0, plan.runs[0]), static_cast<unsigned>(blocks), 256, lds, st, ka);
}

void miso_batch::launch_grp_multi(const KernelArgs &a, size_t r0, size_t r1) {
  const GenRun m = joined_run(r0, r1);
  const GrpShape msh = grp_shape(m);
  const size_t fp_bytes = fp_bytes_of(m);
  const size_t slice = grp_slice_bytes(m.kmax, 0, msh.ts);
  // (the small genes' segment: eight chains per wavefront, their score tables in global memory -- a tstride of its own)
  const size_t slice8 = grp_slice_bytes(m.kmax, 0, 0);
  KernelArgs ka = a;
  hipStream_t st = stream_for_next();
  ka.slot_event = d_slots + n_k2 + m.first; ka.n_slots = m.count;
  ka.kstride = m.kmax; ka.cstride = 0; ka.tstride = msh.ts;
  ka.pe_dense = 1;
  size_t lds = 0; int blocks = 0, segs = 0;
  // A run on 16 or 32 lanes per chain is one segment PER ISOFORM COUNT (the run's events are ordered by it): every segment starts
  // a new workgroup, so no wavefront carries chains of two isoform counts -- such a wavefront runs both counts' read loops one after
  // the other (kernels_grp.inl pe_fast), twice a chain's own time, and with the class's longest chains that was the launch's length
  // (round 6, profiles/r06_mix_timeline.txt).  As far as the segments suffice (knobs.pe_no_ksplit: a segment per run).
  auto k_pieces = [&](const GenRun &run) {
    std::vector<int> cuts{0};
    for (int e = 1; e < run.count; e++)
      if (events[h_slots[n_k2 + run.first + e]].K != events[h_slots[n_k2 + run.first + e - 1]].K) cuts.push_back(e);
    cuts.push_back(run.count);
    return cuts;
  };
  size_t want_segs = 0;
  for (size_t ri = r0; ri < r1; ri++)
    want_segs += (gen_runs[ri].wide() || plan.runs[ri].G == 64) ? 1 : k_pieces(gen_runs[ri]).size() - 1;
  const bool ksplit = want_segs <= static_cast<size_t>(K2_MAX_SEGS) && !knobs.pe_no_ksplit;
  for (size_t ri = r0; ri < r1; ri++) {
    GenRun &run = gen_runs[ri];
    const long chains = static_cast<long>(run.count) * p.noChains;
    if (run.wide()) {
      ka.seg_slot[segs] = run.first - m.first; ka.seg_block[segs] = blocks;
      const size_t lds0 = align_up(fp_bytes + 4 * slice, 16);
      ka.red_off = static_cast<int32_t>(lds0);
      lds = std::max(lds, lds0 + 96);
      blocks += static_cast<int>(wide_setup(run, chains, st));
      ka.coop_tab = run.coop.tab.d; ka.coop_mem = run.coop.mem.d;
      ka.seg_ts[segs] = msh.ts;
      ka.seg_lanes[segs++] = K2_WIDE;
    } else {
      const int G = plan.runs[ri].G, cpw = 64 / G;
      lds = std::max(lds, fp_bytes + 4 * static_cast<size_t>(cpw) * (G == 8 ? slice8 : slice));
      const std::vector<int> cuts = (ksplit && G != 64) ? k_pieces(run) : std::vector<int>{0, run.count};
      for (size_t c = 0; c + 1 < cuts.size(); c++) {
        const long pc = static_cast<long>(cuts[c + 1] - cuts[c]) * p.noChains;
        ka.seg_slot[segs] = run.first - m.first + cuts[c]; ka.seg_block[segs] = blocks;
        blocks += static_cast<int>(((pc + cpw - 1) / cpw + 3) / 4);
        ka.seg_ts[segs] = G == 8 ? 0 : msh.ts;
        ka.seg_lanes[segs++] = G;
      }
    }
  }
  ka.seg_slot[segs] = m.count; ka.seg_block[segs] = blocks; ka.n_segs = segs;
  launch_kernel(run_kernel_of(RunKernel::GrpMulti, m.kc, plan.runs[r0]), static_cast<unsigned>(blocks), 256, lds, st, ka);
}

// ---- what the last launch put on the device, kernel by kernel (miso_batch_launch_stats): from its plan, on demand ----
// Names and wavefront layouts are the plan's: a half's kind with its lane plan, a run's kind with its own layout (slices of
// G lanes per chain, sampler_flat's wave_tab, a workgroup per chain).
std::vector<miso_kernel_stat_t> miso_batch::launch_stats() const {
  std::vector<miso_kernel_stat_t> out;
  if (!plan.sampled) return out;
  const LaunchPlan &q = plan;
  const int C = p.noChains;
  auto add_stat = [&](const std::string &name, double waves, double trips, double chains, double words) {
    miso_kernel_stat_t ks{};
    std::snprintf(ks.name, sizeof ks.name, "%s", name.c_str());
    ks.waves = waves; ks.trips = trips; ks.iterations = static_cast<double>(p.noIterations) + 1.0;
    ks.chains = chains; ks.words = words;
    out.push_back(ks);
  };
  for (const K2Half &h : k2) {
    if (h.count <= 0) continue;
    // slot order = events by drawing reads, descending, each with its noChains chains
    std::vector<int> nd(h.count);
    for (int i = 0; i < h.count; i++) nd[i] = events[h_slots[h.first + i]].n_draw;
    const long chains = static_cast<long>(h.count) * C;
    double trips = 0, words = 0;
    long waves = 0;
    const int bshift = p.paired ? 2 : 3;   // draws per Philox block: four, single-end eight (half-words, miso_philox.h)
    // chains [c0, c1) of the list with G lanes per chain; a chain wider than a wavefront: on `copies` wavefronts, each with its trips
    auto slice = [&](long c0, long c1, int G, int copies = 1) {
      const int cpw = std::max(1, 64 / G);
      for (long s0 = c0; s0 < c1; s0 += cpw, waves += copies) {
        int mx = 0;   // blocks of the wavefront's largest chain (single-end: the partial block is one of the stride's)
        for (long sl = s0; sl < std::min(c1, s0 + cpw); sl++) {
          const int n = nd[sl / C];
          mx = std::max(mx, (n >> bshift) + ((!p.paired && (n & ((1 << bshift) - 1))) ? 1 : 0));
          words += n;
        }
        const int t = (mx + 2 * G - 1) / (2 * G);             // paired-end: trips of two Philox blocks per lane
        trips += copies * (p.paired ? 2 * t + 1 : (mx + G - 1) / G);   // counted in blocks per lane (single-end: stride positions)
      }
    };
    switch (h.kind) {
    case K2Kernel::Lane:
      for (int n : nd) words += static_cast<double>(n) * C;
      waves = (chains * q.lane_G + 63) / 64;
      break;
    case K2Kernel::Multi: {
      const LanePlan &pl = h.plan;
      for (int sg = 0; sg < pl.n_segs; sg++) {
        const long c0 = static_cast<long>(pl.seg_slot[sg]) * C, c1 = static_cast<long>(pl.seg_slot[sg + 1]) * C;
        if (pl.seg_lanes[sg] == K2_WIDE) {
          for (long c = c0; c < c1; c++) {
            const size_t we = static_cast<size_t>(c / C - pl.seg_slot[sg]);
            const int m = we < pl.wide_wgs.size() ? pl.wide_wgs[we] : 1;     // workgroups of the chain (coop.hpp)
            slice(c, c + 1, 64 * pl.wpb * m, pl.wpb * m);
          }
        } else slice(c0, c1, pl.seg_lanes[sg]);
      }
      break;
    }
    case K2Kernel::Mix:
      slice(0, static_cast<long>(q.k2_mix) * C, h.G + 1);
      slice(static_cast<long>(q.k2_mix) * C, chains, h.G);
      break;
    default:
      slice(0, chains, h.G);
    }
    add_stat(k2_kernel_of(h).name, static_cast<double>(waves), trips, static_cast<double>(chains), words);
  }
  for (size_t ri = 0; ri < gen_runs.size() && ri < q.runs.size(); ri++) {
    const GenRun &run = gen_runs[ri];
    const LaunchPlan::Run &r = q.runs[ri];
    const std::string name = run_kernel_of(r.kind, run.kc, r).name;
    const long chains = static_cast<long>(run.count) * C;
    std::vector<const PackedEvent *> evs;   // the run's events in slot order
    for (int j = 0; j < run.count; j++) evs.push_back(&events[h_slots[n_k2 + run.first + j]]);   // the list upload made
    double trips = 0, words = 0;
    long waves = 0;
    switch (r.layout) {
    case RunKernel::LaneK:
      for (const PackedEvent *e : evs) words += static_cast<double>(e->n_draw) * C;
      waves = (chains + 63) / 64;
      break;
    case RunKernel::Flat: {   // the wavefronts as flat_waves laid them out
      const std::vector<int32_t> &tab = run.wave_tab.host;
      for (size_t w = 0; w + 1 < tab.size(); w += 2) {
        const int first = tab[w], n = tab[w + 1] & 0xFF;
        const bool wide = (tab[w + 1] & FLAT_WIDE) != 0;
        if (n == 0) continue;
        long units = 0;
        for (long sl = first; sl < first + n; sl++) { units += evs[sl / C]->n_units; if (!wide || (w / 2) % 4 == 0) words += evs[sl / C]->n_draw; }
        trips += wide ? (units + 255) / 256 : (units + 63) / 64;
        waves++;
      }
      break;
    }
    default: {   // G lanes per chain (a workgroup per chain: four wavefronts, the quads dealt over 256 lanes); a lane per isoform
                 // (sampler_wave, sampler_big): a trip per drawing quad
      const bool wide = r.layout == RunKernel::GrpWide;
      const int G = wide ? 256 : r.G, cpw = std::max(1, 64 / G), copies = wide ? 4 : 1;
      const bool per_quad = r.layout == RunKernel::Wave || r.layout == RunKernel::Big;
      const bool cls = !p.paired && r.sh.qs > 0;
      for (long s0 = 0; s0 < chains; s0 += cpw, waves += copies) {
        int mx = 0, kmx = 0;
        for (long sl = s0; sl < std::min(chains, s0 + cpw); sl++) {
          const PackedEvent &e = *evs[sl / C];
          mx = std::max(mx, cls ? e.n_units : (e.n_draw + 3) / 4);
          kmx = std::max(kmx, e.K);
          words += e.n_draw;
        }
        const int nw = (cls && kmx - 1 <= 3) ? 2 : 1;         // Philox blocks in flight (class path, K <= 4)
        trips += copies * (per_quad ? mx : nw * ((mx + nw * G - 1) / (nw * G)));
      }
    }
    }
    add_stat(name, static_cast<double>(waves), trips, static_cast<double>(chains), words);
  }
  if (n_exact > 0) {   // one wavefront per event, no chains: `chains` counts the events, `words` their sample uniforms
    add_stat(exact_kernel(p.paired != 0).name, static_cast<double>(n_exact), 0.0, static_cast<double>(n_exact), static_cast<double>(n_exact) * S());
    out.back().iterations = 1.0;
  }
  return out;
}

// The clock probe of this launch (clock_probe_kernel above).  First the flag's store, behind the launch's last kernel on the
// batch's stream; then the probe on a stream of its own: on a hardware queue of its own it starts at once, beside the
// sampler kernels.  Should its stream share the batch's queue (or a profiler serialise the dispatches) it starts when
// everything before it is done, finds the flag set and reports a window of no length, which sync() discards -- in no
// order of execution does it wait for something queued behind it.  Give-up time: 1.5 x the last launch's kernel time + 20 ms.
void miso_batch::start_clock_probe() {
  probe_armed = false;
  if (!clock_probe || probe_failed) return;
  if (!probe_stream) {
    HIP_OK(hipStreamCreateWithFlags(&probe_stream, hipStreamNonBlocking));
    HIP_OK(hipMalloc(&d_probe, 8 * sizeof(unsigned long long)));
    HIP_OK(hipMemset(d_probe, 0, 8 * sizeof(unsigned long long)));
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0) wall_khz = khz;
  }
  probe_gen++;
  uint32_t *flag = reinterpret_cast<uint32_t *>(d_probe + 7);
  hipLaunchKernelGGL(clock_probe_stop, dim3(1), dim3(64), 0, stream, flag, probe_gen);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamWaitEvent(probe_stream, ev0, 0));
  const double cap_ms = 1.5 * (last_ms > 0.f ? last_ms : 2000.0) + 20.0;
  hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, probe_stream, flag, probe_gen, d_probe,
                     static_cast<unsigned long long>(cap_ms * wall_khz));
  HIP_OK(hipGetLastError());
  probe_armed = true;
}

void miso_batch::read_clock_probe() {
  last_clock_ghz = 0.0; last_probe_ms = 0.0;
  if (!probe_armed) return;
  probe_armed = false;
  HIP_OK(hipStreamSynchronize(probe_stream));
  unsigned long long h[5];
  HIP_OK(hipMemcpy(h, d_probe, sizeof(h), hipMemcpyDeviceToHost));
  if (h[4] != 0) { probe_failed = true; return; }   // it gave up: never again for this batch (each time would cost its give-up time)
  const double ms = static_cast<double>(h[2] - h[0]) / wall_khz;
  // a window much shorter than the launch: the probe ran behind the kernels, not beside them
  if (ms < 0.5 * last_ms || ms <= 0.0) return;
  last_probe_ms = ms;
  last_clock_ghz = static_cast<double>(h[3] - h[1]) / (ms * 1e6);
}
