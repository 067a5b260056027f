// knobs.hpp -- the MISO_* tuning knobs of the planner (runtime.hip), read from the environment in ONE place.
//
// Host-only, no HIP: batch.hpp includes it, no kernel unit does.  miso_batch::knobs is refreshed at the entry of
// resolve_pending(), upload() and launch(); everything below those reads the member, so a plan is a function of the batch,
// the device and this struct.  The field declarations are the documentation: what the knob does and its kind --
// [test] forces a path the rule of thumb would not take on a small batch, [A/B] switches a measured decision, [exp] is an
// experiment's dial -- and the profile that justifies the default.  Clamps and defaults that depend on the batch stay at
// the use site; range errors are raised where the value is used, from_env() never fails.
// (Not here: alnio.cpp's MISO_TIMING, plan.cpp's MISO_PLAN_DEBUG, capi.hip's load-time reads, the Python front end's names.)
#pragma once

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace miso {

// A number from the environment: `v` holds the default while unset.  Where being set matters by itself the code asks `set`;
// the three-state switches (unset: the rule of thumb, 0: never, non-zero: always) ask off() / on().
template <class T> struct Opt {
  T v{};
  bool set = false;
  bool off() const { return set && v == 0; }
  bool on() const { return set && v != 0; }
};

struct Knobs {
  // ---- present or absent, whatever the value ("=0" counts as present) ----
  bool no_coop = false;         // MISO_NO_COOP [A/B, test]: every chain on its own workgroup only (coop.hpp)
  bool timing = false;          // MISO_TIMING [exp]: stage times and the packing's figures on stderr
  bool quiet = false;           // MISO_QUIET [test]: no warning for genes of more than 80 isoforms
  bool k2_general = false;      // MISO_K2_GENERAL [test]: paired-end two-isoform events take sampler_grp
  bool no_pe_delta = false;     // MISO_NO_PE_DELTA [A/B, test]: every paired-end two-isoform event to MODE 1 (fixed at upload: the slot order)
  bool no_pe_buckets = false;   // MISO_NO_PE_BUCKETS [A/B, test]: one launch per class, no size buckets (profiles/r03_pe_buckets.txt)
  bool no_pe_dense = false;     // MISO_NO_PE_DENSE [A/B, test]: the quad loops over the plain records, no dense path
  bool k2_settle_all = false;   // MISO_K2_SETTLE_ALL [test]: kernels_k2.inl rescans for high halves on the threshold
  bool k2_full_math = false;    // MISO_K2_FULL_MATH [test]: the step's exp / log with their special cases at every call (detmath_n.hpp)
  bool serial_kernels = false;  // MISO_SERIAL_KERNELS [A/B, test]: every kernel of a launch on the batch's own stream
  bool no_autotune = false;     // MISO_NO_AUTOTUNE [A/B]: no trial launches, the rule of thumb's lanes per chain
  bool autotune_k2 = false;     // MISO_AUTOTUNE_K2 [exp]: trial launches for sampler_k2 too (the rule is the measured optimum)
  bool k2_no_narrow = false;    // MISO_K2_NO_NARROW [A/B, test]: never the three-wavefront kernel of the several-rounds plan
  bool no_class_path = false;   // MISO_NO_CLASS_PATH [test]: sampler_grp's direct mask path, no class thresholds
  bool pe_force_exact = false;  // MISO_PE_FORCE_EXACT [test]: sampler_grp leaves every read to pe_pick_exact
  bool flat_no_desc = false;    // MISO_FLAT_NO_DESC [A/B, test]: sampler_flat's walking loop everywhere (not with workgroup-wide chains)
  bool flat_no_ks = false;      // MISO_FLAT_NO_KS [A/B, test]: sampler_flat's run-time layout everywhere
  bool flat_no_uni = false;     // MISO_FLAT_NO_UNI [A/B, test]: never the kernel that knows every event's isoform count
  bool no_flat = false;         // MISO_NO_FLAT [A/B, test]: sampler_grp instead of sampler_flat
  bool no_pe_all = false;       // MISO_NO_PE_ALL [A/B, test]: no sampler_grp_all, the launches per run
  bool no_pe_multi = false;     // MISO_NO_PE_MULTI [A/B, test]: every run its own launch (also rules out sampler_grp_all)
  bool pe_all = false;          // MISO_PE_ALL [test]: sampler_grp_all also under a forced MISO_GENERAL_LANES=16 (small batches)
  bool pe_multi = false;        // MISO_PE_MULTI [test]: sampler_grp_multi whatever the launch count (profiles/r03_pe_buckets.txt)
  bool no_pe_merge = false;     // MISO_NO_PE_MERGE [A/B]: a size bucket never joins the class's normal launch
  bool pe_merge = false;        // MISO_PE_MERGE [A/B]: ... joins it whatever the hardware queue count (default: fewer than 8)
  bool pe_no_ksplit = false;    // MISO_PE_NO_KSPLIT [A/B]: sampler_grp_multi with a segment per run, not per isoform count (profiles/r06_mix_timeline.txt)
  bool flat_pack_wgs2 = false;  // MISO_FLAT_PACK_WGS2 [A/B]: packed five-to-eight-isoform launches sized for two workgroups per CU, not three (profiles/r06_flat_licm.txt)

  // ---- unset / 0 / non-zero: rule of thumb / never / always ----
  Opt<int> k2_pair;             // MISO_K2_PAIR [A/B]: 0: 4-wavefront workgroups in slot order; set at all: 8-wavefront pairs even beyond one round
  Opt<int> k2_mix;              // MISO_K2_MIX [A/B]: 0: no sampler_k2_mix
  Opt<int> k2_multi;            // MISO_K2_MULTI [A/B, test]: 0: the single-width / two-width launches, no sampler_k2_multi
  Opt<int> lane_ilp;            // MISO_LANE_ILP [A/B, test]: sampler_lane_ilp never / always (profiles/r05_sampler_lane_ilp.txt)
  Opt<int> k2_global_pair;      // MISO_K2_GLOBAL_PAIR [A/B, test]: wavefronts paired across the runs never / always (default: from seven runs; profiles/r03_wave_time.txt)
  Opt<int> flat_thr_skip;       // MISO_FLAT_THR_SKIP [A/B, test]: thresholds only for chains whose psi changed (profiles/r04_occupancy.txt)
  Opt<int> k2_wide_dedup;       // MISO_K2_WIDE_DEDUP [A/B]: 0: a workgroup-wide chain's step on all eight wavefronts, not four (kernels_k2.inl)
  Opt<int> k2_balance;          // MISO_K2_BALANCE [A/B]: 0: the two wavefronts of a SIMD do not keep step (kernels_k2.inl k2_balance)
  Opt<int> stream_prio;         // MISO_STREAM_PRIO [exp]: non-zero: stream priorities, fixed at upload (off: profiles/r05_stream_priorities.txt)
  Opt<int> pe_mix_lanes;        // MISO_PE_MIX_LANES [exp]: 16 | 32 lanes for a class of a mix (default: 16 below a mean of 400 quads; profiles/r05_pe_mix_lanes.txt)
  Opt<int> pe_lanes8;           // MISO_PE_LANES8 [A/B]: eight lanes 0 never / 1 always / 2 by the rule in a mix too (profiles/r05_lanes_sweep.txt)
  Opt<int> prio_quartiles;      // MISO_PRIO_QUARTILES [A/B]: priority by progress; launch(): non-zero everywhere; launch_flat(): set at all: not by its own rule (profiles/r06_prio_by_progress.txt)
  Opt<int> flat_pack;           // MISO_FLAT_PACK [A/B, test]: sampler_flat's wavefronts packed by work units never / always

  // ---- numbers whose presence also matters ----
  Opt<int> lds_max_kb{80};      // MISO_LDS_MAX_KB [exp]: a workgroup's LDS budget; set: plan_flat sizes by it, launch_flat keeps its sizing for packed runs
  Opt<int> flat_nc;             // MISO_FLAT_NC [exp, test]: sampler_flat's chains per wavefront; set: no flat/grp contest, no re-sizing of packed runs
  Opt<int> general_lanes;       // MISO_GENERAL_LANES [test]: sampler_grp's lanes per chain; set: no size-bucket widths, no grp_all / grp_multi
  Opt<int> lanes_per_chain;     // MISO_LANES_PER_CHAIN [test]: sampler_k2's lanes per chain; set: no multi-width plans
  Opt<double> k2_target;        // MISO_K2_TARGET [test]: the bound on a wavefront's step in plan_lanes (small batches with many widths); set: re-plan
  bool k2_cost_set = false;     // MISO_K2_COST [exp]: "block,step1,step2,step3,step4" over the lane plans' cost model; set: re-plan
  std::vector<double> k2_cost;  // ... the numbers that parsed, in that order (at most five)
  Opt<int> coop_min_quads;      // MISO_COOP_MIN_QUADS [test]: LaneCost::coop_min_quads, at least 1; set: re-plan
  Opt<int> k2_wpb;              // MISO_K2_WPB [A/B, test]: the single-end plan's wavefronts per workgroup, 8, 4 or 1 (profiles/r03_k2_multi_ab.txt); set: re-plan
  Opt<int> k2w_wpb;             // MISO_K2W_WPB [A/B]: 8: the MODE 2 plan on 8-wavefront workgroups, else never (profiles/r03_pe_k2_wpb.txt); set: re-plan
  Opt<int> coop_draws{8192};    // MISO_COOP_DRAWS [test]: one workgroup per n drawing pairs of a wide chain, at least 256; set: the table decides chain by chain
  Opt<int> flat_wgs;            // MISO_FLAT_WGS [exp]: workgroups per CU sampler_flat is sized for, at least 1 (default by class: profiles/r04_occupancy.txt)
  Opt<long> flat_pack_ov{100};  // MISO_FLAT_PACK_OV [exp]: a chain's fixed cost in the packing, per cent of the rule (0: by units alone; profiles/r05_flat_chunks.txt)
  Opt<int> wave_slots;          // MISO_WAVE_SLOTS [exp]: what the planners take as resident wavefronts, at least 64 (fixed at upload)
  Opt<double> pe_t_32;          // MISO_PE_T_32 [exp]: lanes needed for the "at least 32 lanes" bucket (default 24 or 32 by the batch: profiles/r05_pe_mix_lanes.txt)
  Opt<int> k2_split;            // MISO_K2_SPLIT [exp]: events of sampler_k2_mix's wide part
  Opt<int> collapsed_lanes;     // MISO_COLLAPSED_LANES [exp, test]: 1, 2, 4 or 8 lanes per chain of the collapsed step (profiles/r03_collapsed.txt)
  Opt<long> coop_max_polls;     // MISO_COOP_MAX_POLLS [test]: polls after which a cooperative chain gives up, at least 1
  bool general_lanes_by_class_set = false;                // MISO_GENERAL_LANES_BY_CLASS [exp]: "4:16,8:16,12:32,16:32,32:32", a class not named: 16
  std::vector<std::pair<int, int>> general_lanes_by_class;   // ... {class, lanes} as listed

  // ---- plain numbers ----
  Opt<double> pe_share{2.0};    // MISO_PE_SHARE [exp]: a chain should be done in 1 / this of the batch's time (size buckets)
  Opt<double> pe_t_wave{64.0};  // MISO_PE_T_WAVE [exp, test]: lanes needed for a wavefront of its own (profiles/r03_pe_buckets.txt)
  Opt<double> pe_t_wide{256.0}; // MISO_PE_T_WIDE [exp, test]: ... for a workgroup of its own
  Opt<int> pe_t_small{96};      // MISO_PE_T_SMALL [exp, test]: drawing quads up to which a gene joins the small bucket, 0: none (profiles/r06_small_genes.txt)
  Opt<double> flat_rounds_frac{0.85};   // MISO_FLAT_ROUNDS_FRAC [exp]: the fraction of two rounds a packed launch aims at (profiles/r06_flat_pack_rounds.txt)
  Opt<int> pe_all_order{1};     // MISO_PE_ALL_ORDER [A/B]: sampler_grp_all's segments 0 per run, 1 heaviest first, 2 alternating, 3 lightest first (777 / 705 / 767 / 851 ms)
  Opt<int> lane_spread{1};      // MISO_LANE_SPREAD [exp]: sampler_lane_ilp's chains spread to n wavefronts per SIMD, 0: never

  // some knob that a cached lane plan does not carry in its key is set: plan again (plan_k2)
  bool replan_k2() const { return k2_target.set || k2_cost_set || coop_min_quads.set; }

  // every field by its name: from_env() reads through it, dump() prints through it
  template <class K, class F> static void each(K &k, F &&f) {
    f("MISO_NO_COOP", k.no_coop); f("MISO_TIMING", k.timing); f("MISO_QUIET", k.quiet); f("MISO_K2_GENERAL", k.k2_general);
    f("MISO_NO_PE_DELTA", k.no_pe_delta); f("MISO_NO_PE_BUCKETS", k.no_pe_buckets); f("MISO_NO_PE_DENSE", k.no_pe_dense);
    f("MISO_K2_SETTLE_ALL", k.k2_settle_all); f("MISO_K2_FULL_MATH", k.k2_full_math); f("MISO_SERIAL_KERNELS", k.serial_kernels);
    f("MISO_NO_AUTOTUNE", k.no_autotune); f("MISO_AUTOTUNE_K2", k.autotune_k2); f("MISO_K2_NO_NARROW", k.k2_no_narrow);
    f("MISO_NO_CLASS_PATH", k.no_class_path); f("MISO_PE_FORCE_EXACT", k.pe_force_exact); f("MISO_FLAT_NO_DESC", k.flat_no_desc);
    f("MISO_FLAT_NO_KS", k.flat_no_ks); f("MISO_FLAT_NO_UNI", k.flat_no_uni); f("MISO_NO_FLAT", k.no_flat);
    f("MISO_NO_PE_ALL", k.no_pe_all); f("MISO_NO_PE_MULTI", k.no_pe_multi); f("MISO_PE_ALL", k.pe_all); f("MISO_PE_MULTI", k.pe_multi);
    f("MISO_NO_PE_MERGE", k.no_pe_merge); f("MISO_PE_MERGE", k.pe_merge); f("MISO_PE_NO_KSPLIT", k.pe_no_ksplit);
    f("MISO_FLAT_PACK_WGS2", k.flat_pack_wgs2);
    f("MISO_K2_PAIR", k.k2_pair); f("MISO_K2_MIX", k.k2_mix); f("MISO_K2_MULTI", k.k2_multi); f("MISO_LANE_ILP", k.lane_ilp);
    f("MISO_K2_GLOBAL_PAIR", k.k2_global_pair); f("MISO_FLAT_THR_SKIP", k.flat_thr_skip); f("MISO_K2_WIDE_DEDUP", k.k2_wide_dedup);
    f("MISO_K2_BALANCE", k.k2_balance); f("MISO_STREAM_PRIO", k.stream_prio); f("MISO_PE_MIX_LANES", k.pe_mix_lanes);
    f("MISO_PE_LANES8", k.pe_lanes8); f("MISO_PRIO_QUARTILES", k.prio_quartiles); f("MISO_FLAT_PACK", k.flat_pack);
    f("MISO_LDS_MAX_KB", k.lds_max_kb); f("MISO_FLAT_NC", k.flat_nc); f("MISO_GENERAL_LANES", k.general_lanes);
    f("MISO_LANES_PER_CHAIN", k.lanes_per_chain); f("MISO_K2_TARGET", k.k2_target); f("MISO_COOP_MIN_QUADS", k.coop_min_quads);
    f("MISO_K2_WPB", k.k2_wpb); f("MISO_K2W_WPB", k.k2w_wpb); f("MISO_COOP_DRAWS", k.coop_draws); f("MISO_FLAT_WGS", k.flat_wgs);
    f("MISO_FLAT_PACK_OV", k.flat_pack_ov); f("MISO_WAVE_SLOTS", k.wave_slots); f("MISO_PE_T_32", k.pe_t_32);
    f("MISO_K2_SPLIT", k.k2_split); f("MISO_COLLAPSED_LANES", k.collapsed_lanes); f("MISO_COOP_MAX_POLLS", k.coop_max_polls);
    f("MISO_PE_SHARE", k.pe_share); f("MISO_PE_T_WAVE", k.pe_t_wave); f("MISO_PE_T_WIDE", k.pe_t_wide); f("MISO_PE_T_SMALL", k.pe_t_small);
    f("MISO_FLAT_ROUNDS_FRAC", k.flat_rounds_frac); f("MISO_PE_ALL_ORDER", k.pe_all_order); f("MISO_LANE_SPREAD", k.lane_spread);
  }

  // The environment as it is now (nothing cached).  Numbers parse as atoi / atol / atof do: text that is no number is 0.
  static Knobs from_env() {
    struct Read {
      void operator()(const char *n, bool &b) const { b = std::getenv(n) != nullptr; }
      void operator()(const char *n, Opt<int> &o) const { if (const char *s = std::getenv(n)) { o.v = std::atoi(s); o.set = true; } }
      void operator()(const char *n, Opt<long> &o) const { if (const char *s = std::getenv(n)) { o.v = std::atol(s); o.set = true; } }
      void operator()(const char *n, Opt<double> &o) const { if (const char *s = std::getenv(n)) { o.v = std::atof(s); o.set = true; } }
    };
    Knobs k;
    each(k, Read{});
    if (k.coop_min_quads.set) k.coop_min_quads.v = std::max(1, k.coop_min_quads.v);
    if (k.coop_draws.set) k.coop_draws.v = std::max(256, k.coop_draws.v);
    if (k.flat_wgs.set) k.flat_wgs.v = std::max(1, k.flat_wgs.v);
    if (k.wave_slots.set) k.wave_slots.v = std::max(64, k.wave_slots.v);
    if (k.coop_max_polls.set) k.coop_max_polls.v = std::max(1L, k.coop_max_polls.v);
    if (const char *s = std::getenv("MISO_K2_COST")) {
      double c[5];
      const int got = std::sscanf(s, "%lf,%lf,%lf,%lf,%lf", &c[0], &c[1], &c[2], &c[3], &c[4]);
      k.k2_cost_set = true;
      k.k2_cost.assign(c, c + std::max(0, got));
    }
    if (const char *s = std::getenv("MISO_GENERAL_LANES_BY_CLASS")) {
      k.general_lanes_by_class_set = true;
      while (s && *s) {
        int kc = 0, g = 0;
        if (std::sscanf(s, "%d:%d", &kc, &g) == 2) k.general_lanes_by_class.emplace_back(kc, g);
        s = std::strchr(s, ',');
        if (s) s++;
      }
    }
    return k;
  }

  // One "NAME=value" line per field that is set (miso_selftest_knobs): a switch as 1, a number as parsed and clamped.
  std::string dump() const {
    struct Write {
      std::string &out;
      void line(const char *n, const std::string &v) const { out += std::string(n) + "=" + v + "\n"; }
      void operator()(const char *n, const bool &b) const { if (b) line(n, "1"); }
      void operator()(const char *n, const Opt<int> &o) const { if (o.set) line(n, std::to_string(o.v)); }
      void operator()(const char *n, const Opt<long> &o) const { if (o.set) line(n, std::to_string(o.v)); }
      void operator()(const char *n, const Opt<double> &o) const { if (o.set) line(n, num(o.v)); }
      static std::string num(double x) { char b[32]; std::snprintf(b, sizeof b, "%.17g", x); return b; }
    };
    std::string out;
    const Write w{out};
    each(*this, w);
    std::string list;
    for (double x : k2_cost) list += (list.empty() ? "" : ",") + Write::num(x);
    if (k2_cost_set) w.line("MISO_K2_COST", list);
    list.clear();
    for (const auto &c : general_lanes_by_class) list += (list.empty() ? "" : ",") + std::to_string(c.first) + ":" + std::to_string(c.second);
    if (general_lanes_by_class_set) w.line("MISO_GENERAL_LANES_BY_CLASS", list);
    return out;
  }
};

}  // namespace miso
