"""GPU: stop = CONVERGENT_MEAN through every sampler kernel family, bit for bit against the CPU checker.

The device re-runs an unconverged event from iteration 0 through its latest round and is told where the later rounds
open (runtime.hip converge_rounds, device.hpp RoundOpen): every kernel consults that table in its own loop.  One batch
per family (tests/_convergent_cases.py; tests/test_convergent_cases.py shows on the checker that each takes several
rounds and that its events leave at different ones), forced onto the family's layouts with the switches of
tests/test_gpu_heavy_tail.py and tests/test_gpu_collapsed.py.  Each variant must name the family among the first
launch's kernels AND among the later rounds'."""
import contextlib
import os

import numpy as np
import pytest

import _convergent_cases as cc

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _equal(gpu, cpu, where):
    assert cpu.rc == 0
    assert np.array_equal(gpu.samples, cpu.samples), where
    assert np.array_equal(gpu.loglik, cpu.loglik, equal_nan=True), where
    assert np.array_equal(gpu.assignment, cpu.assignment), where
    assert (gpu.rundata.noAccepted, gpu.rundata.noRejected) == (cpu.accepted, cpu.rejected), where
    assert (gpu.rundata.noIters, gpu.rundata.noBurnIn, gpu.rundata.noSamples) == tuple(int(cpu.rundata[i]) for i in (1, 3, 8)), where


def _check(orc, name, env, families, device_match=False, absent=()):
    c = cc.case(orc, name)
    cpu, rounds = c.reference(orc), c.rounds(orc)
    with _env(**env):
        b = cc.run_device(c, device_match=device_match)
    first, later = b.first_kernels, cc.later_kernels(b)
    print(name, env, "rounds", rounds, "kernels", first, "|", later)
    for i, r in enumerate(cpu):
        _equal(b.result(i), r, (name, env, i, c.events[i].K, c.events[i].n, rounds[i], first, later))
    assert b.rounds() == max(rounds), (name, env, b.rounds(), rounds)
    for f in families:
        assert f in first and f in later, (name, env, f, first, later)
    for f in absent:
        assert f not in first and f not in later, (name, env, f, first, later)


LANES16 = dict(MISO_GENERAL_LANES="16", MISO_NO_PE_BUCKETS="1", MISO_PE_ALL="1")

CASES = [
    # two isoforms, single-end: the planner's widths, one width per launch, a small bound on a wavefront's step (wide chains,
    # sampler_k2_multi), chains on several workgroups and on one, one lane per chain, a wavefront per chain
    ("k2_se", {}, ["sampler_k2"]),
    ("k2_se", dict(MISO_K2_MULTI="0"), ["sampler_k2<"]),
    ("k2_se", dict(MISO_K2_TARGET="1400"), ["sampler_k2_multi<0, "]),
    ("k2_se", dict(MISO_K2_TARGET="1400", MISO_COOP_MIN_QUADS="1"), ["sampler_k2_multi<0, "]),
    ("k2_se", dict(MISO_NO_COOP="1"), ["sampler_k2"]),
    ("k2_se", dict(MISO_LANES_PER_CHAIN="1"), ["sampler_k2<1, 0, "]),
    ("k2_se", dict(MISO_LANES_PER_CHAIN="64"), ["sampler_k2<64, 0, "]),
    # two isoforms, paired-end: MODE 2 (score differences), MODE 1, eight wavefronts per workgroup, the general kernel
    ("k2_pe", {}, ["sampler_k2_multi<2, "]),
    ("k2_pe", dict(MISO_NO_PE_DELTA="1"), ["sampler_k2_multi<1, "], False, ["sampler_k2_multi<2, "]),
    ("k2_pe", dict(MISO_K2W_WPB="8"), ["sampler_k2_multi<2, 8>"]),
    ("k2_pe", dict(MISO_K2_GENERAL="1"), ["sampler_grp<"], False, ["sampler_k2"]),
    # sampler_flat: the instantiations of 4, 8, 12 and 32 isoforms; packed wavefronts of two chains on the walking loop
    ("flat_3", {}, ["sampler_flat<4, "]),
    ("flat_5", {}, ["sampler_flat<8, "]),
    ("flat_10", {}, ["sampler_flat<12, "]),
    ("flat_18", {}, ["sampler_flat<32, "]),
    ("flat_3", dict(MISO_FLAT_PACK="1", MISO_FLAT_NC="2", MISO_FLAT_NO_DESC="1"), ["sampler_flat<4, "]),
    ("flat_5", dict(MISO_FLAT_PACK="1", MISO_FLAT_NC="2", MISO_FLAT_NO_DESC="1"), ["sampler_flat<8, "]),
    ("flat_10", dict(MISO_FLAT_PACK="1", MISO_FLAT_NC="2", MISO_FLAT_NO_DESC="1"), ["sampler_flat<12, "]),
    ("flat_18", dict(MISO_FLAT_PACK="1", MISO_FLAT_NC="2", MISO_FLAT_NO_DESC="1"), ["sampler_flat<32, "]),
    # sampler_grp, paired-end: size buckets (workgroup-wide and cooperative chains), the buckets in one launch, the exact scan
    ("grp_pe_3", {}, ["sampler_grp<"]),
    ("grp_pe_5", {}, ["sampler_grp<"]),
    ("grp_pe_10", {}, ["sampler_grp<"]),
    ("grp_pe_3", dict(MISO_PE_MULTI="1"), ["sampler_grp_multi<4>"]),
    ("grp_pe_5", dict(MISO_PE_MULTI="1"), ["sampler_grp_multi<8>"]),
    ("grp_pe_10", dict(MISO_PE_MULTI="1"), ["sampler_grp_multi<12>"]),
    ("grp_pe_3", dict(MISO_PE_FORCE_EXACT="1"), ["sampler_grp<"]),
    ("grp_pe_5", dict(MISO_PE_FORCE_EXACT="1"), ["sampler_grp<"]),
    ("grp_pe_10", dict(MISO_PE_FORCE_EXACT="1"), ["sampler_grp<"]),
    ("grp_all", LANES16, ["sampler_grp_all"]),
    # 33 - 64 and 65 - 256 isoforms beside small genes
    ("wave_se", {}, ["sampler_wave<false>"]),
    ("wave_pe", {}, ["sampler_wave<true>"]),
    ("big_se", {}, ["sampler_big<false>"]),
    # the collapsed Gibbs step against the checker's collapsed mode
    ("collapsed_k2", dict(MISO_COLLAPSED_LANES=None, MISO_LANE_ILP=None), ["sampler_lane_ilp"]),
    ("collapsed_k2", dict(MISO_COLLAPSED_LANES="1", MISO_LANE_ILP="1"), ["sampler_lane_ilp"]),
    ("collapsed_k2", dict(MISO_COLLAPSED_LANES="1", MISO_LANE_ILP="0"), ["sampler_lane"], False, ["sampler_lane_ilp"]),
    ("collapsed_k2", dict(MISO_COLLAPSED_LANES="2", MISO_LANE_ILP=None), ["sampler_k2c<2>"]),
    ("collapsed_k2", dict(MISO_COLLAPSED_LANES="8", MISO_LANE_ILP=None), ["sampler_k2c<8>"]),
    ("collapsed_mix", {}, ["sampler_lane_k", "sampler_wave<false>"]),
    # reads matched on the device in the first launch; the later rounds run from the packed events
    ("k2_se", {}, ["sampler_k2"], True),
    ("grp_pe_5", {}, ["sampler_grp<"], True),
]


def _id(c):
    env = "-".join("%s=%s" % (k[5:].lower(), v) for k, v in c[1].items() if v is not None) or "default"
    return "%s-%s%s" % (c[0], env, "-device_match" if len(c) > 3 and c[3] else "")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_rounds_bit_exact_on_every_layout(orc, case):
    name, env, families = case[:3]
    _check(orc, name, env, families, device_match=len(case) > 3 and case[3], absent=case[4] if len(case) > 4 else ())
