"""GPU: what a launch reports -- last_kernels() and launch_stats() -- for a fixed list of small batches, field for field
against tests/golden/launch_records.json, recorded on an MI355X before the launch plan became the one place that decides a
kernel (csrc/launch.hip run_kernel, runtime.hip plan_k2).  The names are parsed by bench.py and asserted by some thirty
tests; the statistics price bench.py's roofline.

Every batch stays under 2048 chains per run and 2000 iterations, so no timing-dependent trial launch decides anything, and
every random choice is seeded.  The knobs that depend on the host (the hardware queue count behind the merge of a size bucket
into its class's launch) are pinned by the cases themselves.

The recorder (`python tests/test_gpu_launch_records.py record`) is run by hand and is no part of the test run.

The drift case: a launch under MISO_NO_PE_DENSE=1 of a batch uploaded without it sends a one-wavefront-per-gene bucket to
sampler_wave<true>; name and statistics used to be derived a second time without that switch and said sampler_grp<64, true, KC>."""
import json
import os
import re
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "tests")]

import miso_amd
from miso_amd import capi, workload
from _libs import OrcLib
from _problems import expr_for, flat, se_gene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_records.json")
SCHEDULE = dict(iters=24, burn=8, lag=2)
MEAN, VAR = 250.0, 900.0
K2_SIZES = [20, 6000, 300, 5, 0, 2500, 40, 1000, 150, 64, 3, 511]
# ... with events large enough for a workgroup of their own, or several (tests/test_gpu_heavy_tail.py SIZES)
K2_TAIL_SIZES = [20, 60000, 300, 5, 0, 2500, 20000, 40, 1000, 150, 7000, 64, 33000, 3, 511]
# tests/test_gpu_heavy_tail.py test_mixed_pair_counts_three_or_more_isoforms_paired_end_bit_exact
PE_TAIL_SIZES = [30, 22000, 200, 5, 0, 1800, 9000, 60, 700, 120, 90, 200, 35, 400, 150, 80]
NO_MERGE = dict(MISO_NO_PE_MERGE="1")
LANES16 = dict(MISO_GENERAL_LANES="16", MISO_NO_PE_BUCKETS="1", MISO_PE_ALL="1")

PAIRED = {"k2_pe", "k2_pe_tail", "k2_pe_bad", "wide_pe", "pe_tail_5", "pe_wave_5", "pe_all", "pe_small", "fuzz_pe"}   # event lists, below

_events_cache = {}


def _genes(orc, paired, counts, sizes, seed0, rand=None):
    """events of counts[j] isoforms and sizes[j] reads (pairs), made as tests/test_gpu_heavy_tail.py makes its own; rand: a
    seed for tests/test_gpu_fuzz.py's random genes in the place of the skip-one-exon ones"""
    from test_gpu_fuzz import random_gene
    rng = None if rand is None else np.random.default_rng(rand)
    out = []
    for j, (K, n) in enumerate(zip(counts, sizes)):
        if rng is not None:
            exons, isoforms = random_gene(rng, K, 400 if paired else 90, 300 if paired else 80)
        else:
            exons, isoforms = se_gene(K, exlen=500 + 11 * j if paired else 90 + 7 * j, gap=300 if paired else 100)
        g = orc.gene(flat(exons), isoforms)
        orc.rng_seed(seed0 + j)
        if paired:
            rc, _, pos, cig = orc.simulate_paired_reads(g, expr_for(K), max(n, 1), 36, MEAN, VAR)
            pos, cig = pos[:2 * n], cig[:2 * n]
        else:
            rc, _, pos, cig = orc.simulate_reads(g, expr_for(K), max(n, 1), 36)
            pos, cig = pos[:n], cig[:n]
        assert rc == 0
        out.append((exons, isoforms, g, pos, cig))
    return out


def _short_gene_pairs(orc):
    """Two-isoform paired-end events under an overhang of 8, the second on a gene whose short isoform (two exons of 110) is no
    longer than the fragments: a pair of 208 ... 220 bases on it is compatible with both isoforms and its score there is
    log(0) -- the event keeps the two-isoform kernels' MODE 1, the clean ones beside it take MODE 2."""
    from test_gpu_heavy_tail import _events
    evs = _events(orc, True, [150, 400, 60, 900])
    exons, isoforms = se_gene(2, exlen=110, gap=300)
    g = orc.gene(flat(exons), isoforms)
    orc.rng_seed(4242)
    rc, _, pos, cig = orc.simulate_paired_reads(g, np.array([0.5, 0.5]), 600, 36, MEAN, VAR)
    assert rc == 0
    m, fl = capi.Gene(exons, isoforms).match_iso_paired(pos, cig, 36, MEAN, VAR, overhang=8)
    both = (m[:, 0] != 0) & (m[:, 1] != 0)
    assert (both & (fl[:, 1] > 220 - 2 * 7 + 1 - 1)).any(), "no drawing pair on a non-finite score entry"
    evs[1] = (exons, isoforms, g, pos, cig)
    return evs


def events_of(orc, key):
    """the named list of events, built once per process: (exons, isoforms, checker gene, pos, cigars) each"""
    if key not in _events_cache:
        from test_gpu_heavy_tail import _events
        make = {
            "k2_se": lambda: _events(orc, False, K2_SIZES),
            "k2_pe": lambda: _events(orc, True, [s // 2 for s in K2_SIZES]),
            "k2_se_tail": lambda: _events(orc, False, K2_TAIL_SIZES),
            "k2_pe_tail": lambda: _events(orc, True, [s // 2 for s in K2_TAIL_SIZES]),
            "k2_pe_bad": lambda: _short_gene_pairs(orc),
            "flat_3": lambda: _genes(orc, False, [3] * 8, [20, 3000, 300, 5, 0, 1200, 40, 150], 5000),
            "flat_mix": lambda: _genes(orc, False, [3, 4, 5, 7, 4, 3, 7, 6, 10, 18, 25], [300, 260, 20, 900, 0, 64, 150, 511, 200, 90, 120], 5100),
            "flat_tail": lambda: _genes(orc, False, [5] * 12, [20, 20000, 300, 5, 0, 2500, 6000, 40, 1000, 150, 64, 511], 5000),
            "fuzz_se": lambda: _genes(orc, False, [3, 5, 8, 9, 13, 17, 2, 2], [400, 120, 900, 50, 300, 200, 700, 30], 5200, rand=7),
            "wide_se": lambda: _genes(orc, False, [40, 5, 70, 2, 40], [400, 300, 90, 200, 60], 700),
            "wide_pe": lambda: _genes(orc, True, [40, 5, 2, 40], [400, 300, 200, 90], 700),
            "pe_tail_5": lambda: _genes(orc, True, [5] * len(PE_TAIL_SIZES), PE_TAIL_SIZES, 7000),
            # ... without its two largest genes: none for a workgroup, two for a wavefront of their own
            "pe_wave_5": lambda: _genes(orc, True, [5] * 9, [30, 200, 5, 0, 1800, 60, 700, 120, 90], 7000),
            "pe_all": lambda: _genes(orc, True, [3, 10, 4, 12, 3, 9, 4, 11, 3, 10], [300, 260, 200, 350, 220, 180, 0, 260, 400, 320], 7100),
            # tests/test_gpu_heavy_tail.py test_small_genes_of_a_whole_gene_batch_on_eight_lanes_bit_exact
            "pe_small": lambda: _genes(orc, True, [3, 18, 5, 10, 14, 4, 7, 12, 20, 9, 3, 5, 16, 8, 11, 6, 5, 5, 9, 13],
                                       [30, 60, 200, 5, 120, 1800, 0, 60, 700, 90, 90, 200, 35, 400, 150, 80, 40, 45, 55, 65], 7300),
            "fuzz_pe": lambda: _genes(orc, True, [3, 6, 2, 9, 2, 14], [300, 150, 500, 80, 40, 220], 7400, rand=9),
        }[key]
        _events_cache[key] = make()
    return _events_cache[key]


class Case:
    def __init__(self, name, events, env=None, chains=2, seed=11, first_id=700, **batch_kw):
        self.name, self.events, self.env, self.chains, self.seed, self.first_id = name, events, dict(env or {}), chains, seed, first_id
        self.batch_kw = batch_kw


CASES = [
    # ---- two isoforms, single-end: a lane width per event on 8-, 4- (also the narrow kernel) and 1-wavefront workgroups, workgroup-wide
    # chains on one and on several workgroups, one forced width on paired and on slot-ordered workgroups, two widths (300 events from
    # miso_amd.workload on a device taken to hold 64 wavefronts)
    Case("k2_se", "k2_se", chains=3),
    Case("k2_se_wpb4", "k2_se", dict(MISO_K2_WPB="4"), chains=3),
    Case("k2_se_narrow", "k2_se", dict(MISO_K2_WPB="4", MISO_K2_TARGET="1e12"), chains=3),
    Case("k2_se_wpb1", "k2_se", dict(MISO_K2_WPB="1"), chains=3),
    Case("k2_se_tail", "k2_se_tail", chains=3),
    Case("k2_se_tail_wide", "k2_se_tail", dict(MISO_K2_TARGET="1400", MISO_NO_COOP="1"), chains=3),
    Case("k2_se_tail_coop", "k2_se_tail", dict(MISO_K2_TARGET="1400", MISO_COOP_MIN_QUADS="1"), chains=3),
    Case("k2_se_lanes4", "k2_se", dict(MISO_LANES_PER_CHAIN="4"), chains=3),
    Case("k2_se_lanes4_slots", "k2_se", dict(MISO_LANES_PER_CHAIN="4", MISO_K2_PAIR="0"), chains=3),
    Case("k2_se_mix", "workload:300", dict(MISO_LANES_PER_CHAIN="1", MISO_WAVE_SLOTS="64"), chains=6),
    # ---- two isoforms, paired-end: MODE 2 on 4- and 8-wavefront workgroups, MODE 1, both halves in one launch, forced widths,
    # the general kernel
    Case("k2_pe", "k2_pe"),
    Case("k2_pe_wpb8", "k2_pe", dict(MISO_K2W_WPB="8")),
    Case("k2_pe_tail", "k2_pe_tail"),
    Case("k2_pe_tail_wide", "k2_pe_tail", dict(MISO_K2_TARGET="1400", MISO_NO_COOP="1")),
    Case("k2_pe_tail_coop", "k2_pe_tail", dict(MISO_K2_TARGET="1400", MISO_COOP_MIN_QUADS="1")),
    Case("k2_pe_tail_coop_wpb8", "k2_pe_tail", dict(MISO_K2W_WPB="8", MISO_K2_TARGET="1400", MISO_COOP_MIN_QUADS="1")),
    Case("k2_pe_tail_mode1_coop", "k2_pe_tail", dict(MISO_NO_PE_DELTA="1", MISO_K2_TARGET="1400", MISO_COOP_MIN_QUADS="1")),
    Case("k2_pe_mode1", "k2_pe", dict(MISO_NO_PE_DELTA="1")),
    Case("k2_pe_lanes8", "k2_pe", dict(MISO_LANES_PER_CHAIN="8")),
    Case("k2_pe_lanes8_mode1", "k2_pe", dict(MISO_LANES_PER_CHAIN="8", MISO_NO_PE_DELTA="1")),
    Case("k2_pe_bad", "k2_pe_bad", overhang=8),
    Case("k2_pe_bad_lanes8", "k2_pe_bad", dict(MISO_LANES_PER_CHAIN="8"), overhang=8),
    Case("k2_pe_general", "k2_pe", dict(MISO_K2_GENERAL="1")),
    # ---- the collapsed step
    Case("lane_ilp", "k2_se", chains=3, collapsed=True),
    Case("lane", "k2_se", dict(MISO_LANE_ILP="0"), chains=3, collapsed=True),
    Case("k2c", "k2_se", dict(MISO_COLLAPSED_LANES="2"), chains=3, collapsed=True),
    Case("lane_k", "wide_se", collapsed=2),
    # ---- three and more isoforms, single-end: sampler_flat uniform, per isoform count, with the run-time layout, packed with
    # workgroup-wide chains; sampler_grp on the class path and without; 33 ... 64 and more isoforms
    Case("flat_3", "flat_3"),
    Case("flat_mix", "flat_mix"),
    Case("flat_mix_rt", "flat_mix", dict(MISO_FLAT_NO_KS="1")),
    Case("flat_tail", "flat_tail"),
    Case("flat_tail_pack", "flat_tail", dict(MISO_FLAT_PACK="1", MISO_FLAT_NC="2", MISO_FLAT_NO_DESC="1")),
    Case("fuzz_se", "fuzz_se", chains=3),
    Case("grp_se", "flat_mix", dict(MISO_NO_FLAT="1")),
    Case("grp_se_masks", "flat_mix", dict(MISO_NO_FLAT="1", MISO_NO_CLASS_PATH="1")),
    Case("grp_se_lanes4", "fuzz_se", dict(MISO_NO_FLAT="1", MISO_GENERAL_LANES="4")),
    Case("wide_se", "wide_se"),
    # ---- three and more isoforms, paired-end: size buckets side by side (workgroup-wide, a wavefront per chain, 32 lanes,
    # normal), chains on several workgroups, the buckets of a class in one launch, a bucket merged into the normal launch,
    # no buckets, plain records, every class in one launch, the small genes' bucket
    Case("pe_tail", "pe_tail_5", NO_MERGE, chains=1),
    Case("pe_tail_wave", "pe_tail_5", dict(NO_MERGE, MISO_PE_T_WAVE="1", MISO_PE_T_WIDE="1e9"), chains=1),
    Case("pe_tail_wave_wide", "pe_tail_5", dict(NO_MERGE, MISO_PE_T_WAVE="64", MISO_PE_T_WIDE="1500"), chains=1),
    Case("pe_tail_coop", "pe_tail_5", dict(NO_MERGE, MISO_COOP_DRAWS="1024"), chains=1),
    Case("pe_tail_multi", "pe_tail_5", dict(MISO_PE_MULTI="1", MISO_PE_T_WAVE="64", MISO_PE_T_WIDE="1500"), chains=1),
    Case("pe_tail_merge", "pe_tail_5", dict(MISO_PE_MERGE="1"), chains=1),
    Case("pe_tail_one", "pe_tail_5", dict(MISO_NO_PE_BUCKETS="1"), chains=1),
    Case("pe_tail_plain", "pe_tail_5", dict(NO_MERGE, MISO_NO_PE_DENSE="1"), chains=1),
    Case("pe_all", "pe_all", LANES16),
    Case("pe_all_apart", "pe_all", dict(LANES16, MISO_NO_PE_ALL="1")),
    Case("pe_small", "pe_small", NO_MERGE),
    Case("pe_small_apart", "pe_small", dict(NO_MERGE, MISO_NO_PE_MULTI="1")),
    Case("fuzz_pe", "fuzz_pe", NO_MERGE),
    Case("wide_pe", "wide_pe", NO_MERGE),
    # ---- MARGINAL, and the exact-posterior modes beside the samplers
    Case("marginal", "flat_mix", algo=capi.MISO_ALGO_MARGINAL),
    Case("exact_se", "fuzz_se", chains=3, exact=True),
    Case("exact_pe", "fuzz_pe", NO_MERGE, exact_paired=True),
]
CASE_NAMES = [c.name for c in CASES]

# every kernel kind, as a pattern some recorded name matches in full
KINDS = [
    r"sampler_k2<4, 0, 8>", r"sampler_k2<4, 0, 4>", r"sampler_k2<8, 1, 4>", r"sampler_k2<8, 2, 4>", r"sampler_k2_mix<2, 1>",
    r"sampler_k2_multi<0, 8>", r"sampler_k2_multi<0, 4>", r"sampler_k2_multi<0, 4, true>", r"sampler_k2_multi<0, 1>",
    r"sampler_k2_multi<1, 4>", r"sampler_k2_multi<2, 4>", r"sampler_k2_multi<2, 8>",
    r"sampler_lane", r"sampler_lane_ilp", r"sampler_k2c<2>", r"sampler_lane_k",
    r"sampler_flat<\d+, [1-9]\d*, true>", r"sampler_flat<\d+, [1-9]\d*>", r"sampler_flat<\d+, 0>",
    r"sampler_grp<\d+, false, \d+>", r"sampler_grp<(2|4|8|16|32), true, \d+>",
    r"sampler_grp<64, true, \d+>", r"sampler_grp<64, true, \d+, true>",
    r"sampler_grp_multi<\d+>", r"sampler_grp_all",
    r"sampler_wave<false>", r"sampler_wave<true>", r"sampler_big<false>", r"sampler_marginal",
    r"exact_sample", r"exact_paired_sample",
]


def split_names(last_kernels):
    """the names of a launch (a name's template arguments hold commas too)"""
    return re.findall(r"\w+(?:<[^>]*>)?", last_kernels)


def run_case(orc, case):
    """the case's batch on the device, under its environment from the upload on: {"last_kernels", "kernels", "uniforms"}"""
    from test_gpu_heavy_tail import _env
    paired = case.events in PAIRED
    with _env(**case.env):
        if case.events.startswith("workload:"):
            b = workload.build_batch(0, int(case.events[9:]), n_reads=120, chains=case.chains, **SCHEDULE)
        else:
            b = miso_amd.Batch(36, paired=paired, mean=MEAN if paired else 0.0, var=VAR if paired else 0.0, chains=case.chains,
                               **dict(SCHEDULE, **case.batch_kw))
            for exons, isoforms, g, pos, cig in events_of(orc, case.events):
                b.add_event(miso_amd.Gene(exons, isoforms), pos, cig)
        b.run(seed=case.seed, first_event_id=case.first_id)
        st = b.launch_stats()
        return {"last_kernels": b.last_kernels(), "kernels": st["kernels"], "uniforms": st["uniforms"]}


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_launch_reports_what_was_recorded(orc, name):
    want = _golden()[name]
    got = run_case(orc, CASES[CASE_NAMES.index(name)])
    assert got["last_kernels"] == want["last_kernels"]
    assert len(got["kernels"]) == len(want["kernels"]), (got["kernels"], want["kernels"])
    for g, w in zip(got["kernels"], want["kernels"]):
        for field in ("name", "waves", "trips", "chains", "words", "iterations"):
            assert g[field] == w[field], (name, field, g, w)
    assert got["uniforms"] == want["uniforms"]


def test_recorded_launches_reach_every_kernel_kind():
    """From the fixture alone: a case list that stops reaching a kind fails here, on any machine."""
    rec = _golden()
    assert sorted(rec) == sorted(CASE_NAMES)
    names = set()
    for r in rec.values():
        names.update(split_names(r["last_kernels"]))
        names.update(k["name"] for k in r["kernels"])
    for kind in KINDS:
        assert any(re.fullmatch(kind, n) for n in names), (kind, sorted(names))
    # one event on a non-finite score beside clean ones: both halves of the two-isoform list in one launch
    for case in ("k2_pe_bad", "k2_pe_bad_lanes8"):
        got = split_names(rec[case]["last_kernels"])
        assert len(got) == 2 and got[0].endswith("2, 4>") and got[1].endswith("1, 4>"), got
    # a size bucket merged into its class's normal launch: one name fewer than runs
    assert len(split_names(rec["pe_tail_merge"]["last_kernels"])) < len(rec["pe_tail_merge"]["kernels"]), rec["pe_tail_merge"]
    assert len(split_names(rec["pe_tail"]["last_kernels"])) == len(rec["pe_tail"]["kernels"]), rec["pe_tail"]
    # workgroup-wide chains in the two-isoform plans: eight (four) wavefronts per chain at the least, more on several workgroups
    for wide, coop, chains, wpb in (("k2_se_tail_wide", "k2_se_tail_coop", 3, 8), ("k2_pe_tail_wide", "k2_pe_tail_coop", 2, 4)):
        w, c = rec[wide]["kernels"][0], rec[coop]["kernels"][0]
        assert w["waves"] > wpb * chains and c["waves"] > w["waves"], (w, c)


@pytest.mark.gpu
def test_name_and_statistics_follow_the_kernel_under_no_pe_dense_at_launch(orc):
    """Uploaded with the default environment, the batch has a one-wavefront-per-gene bucket (the genes of 1800 and 700 pairs);
    launched with MISO_NO_PE_DENSE=1 that run goes to sampler_wave<true> (plain records).  Its name in last_kernels() and in
    launch_stats() must say so, and the samples equal the checker's counter mode bit for bit."""
    from test_gpu_heavy_tail import _env
    evs = events_of(orc, "pe_wave_5")
    sizes = [len(e[3]) // 2 for e in evs]
    kw = dict(iters=50, burn=10, lag=2, chains=1)
    with _env(MISO_NO_PE_DENSE=None):
        b = miso_amd.Batch(36, paired=True, mean=MEAN, var=VAR, **kw)
        for exons, isoforms, g, pos, cig in evs:
            b.add_event(miso_amd.Gene(exons, isoforms), pos, cig)
        b.upload(0)
        with _env(MISO_NO_PE_DENSE="1"):
            b.launch(seed=17, first_event_id=300)
            b.sync()
            b.download()
            names, stats = split_names(b.last_kernels()), b.launch_stats()["kernels"]
    print(names, [k["name"] for k in stats])
    assert "sampler_wave<true>" in names and not any(n.startswith("sampler_grp<64") for n in names), names
    assert {k["name"] for k in stats} == set(names), (names, stats)
    for i, (exons, isoforms, g, pos, cig) in enumerate(evs):
        r = orc.miso_paired(g, pos, cig, 36, MEAN, VAR, mode=OrcLib.COUNTER, seed=17, event_id=300 + i, **kw)
        assert r.rc == 0
        gpu = b.result(i)
        assert np.array_equal(gpu.samples, r.samples, equal_nan=True), (i, sizes[i])
        assert np.array_equal(gpu.loglik, r.loglik, equal_nan=True), (i, sizes[i])
        assert (gpu.assignment == r.assignment).all(), (i, sizes[i])


def record(path=GOLDEN):
    """Run every case once and write the fixture: by hand, on an MI355X, at the commit whose reports are to be kept."""
    orc = OrcLib()
    rec = {}
    for case in CASES:
        rec[case.name] = run_case(orc, case)
        print(case.name, rec[case.name]["last_kernels"], flush=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if sys.argv[1:2] == ["record"]:
        record(*sys.argv[2:3])
