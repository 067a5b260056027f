"""Row f1 on reads and genes no simulator makes: match_kernel (csrc/kernels_match.hip) against what the real reference
returned for tests/_match_cases.py (tests/golden/match/adversarial.npz) -- reads on an exon's last base, one base past
it, to a splice site one base off, inside a retained intron, shorter than the read length; overlapping, abutting and
one-base exons; 33 to 256 isoforms around every 32-bit mask word boundary; the fragment window's two ends.  Then the
sampler on what the kernel packed: more than half of these reads match no isoform.  Integer work: all exact."""
import os

import numpy as np
import pytest

import _match_cases as mc
from _libs import OrcLib
from _problems import flat
from miso_amd import capi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match", "adversarial.npz")
CUTS = (0, 1, 255, 256, 257, 513)      # reads (pairs) of the cut events: around one and two blocks of 256 threads


@pytest.fixture(scope="module")
def gold():
    return mc.Golden(GOLDEN)


def _events(paired):
    """(gene name, cut or None): isoform counts 7, 33, 64 (single-end also 65, 256) interleaved, so that a paired
    event's output offset is rounded up to a multiple of its own K after events of another K."""
    ev = [("tangled", None), ("wide33", None), ("tangled", 1), ("wide64", None), ("tangled", 255), ("shifted", None),
          ("tangled", 0), ("wide33", 257), ("tangled", 256), ("wide64", 1), ("tangled", 257), ("wide33", 255),
          ("tangled", 513)]
    if not paired:
        ev[5:5] = [("wide65", None), ("tangled", 513), ("wide256", None), ("wide65", 257)]
    assert {cut for name, cut in ev if name == "tangled" and cut is not None} == set(CUTS)
    return ev


def _genes():
    return {name: capi.Gene(*mc.gene(name)) for name in mc.gene_names(False)}


def _check_batch(gold, paired, ov, rl, mean=0.0, var=0.0):
    kw = dict(mean=mean, var=var) if paired else {}
    b = capi.Batch(rl, iters=20, burn=10, lag=1, chains=1, overhang=ov, paired=paired, counts_trace=True,
                   device_match=True, **kw)
    pos, cig, _ = mc.paired_reads(mean, var, rl) if paired else mc.single_reads()
    genes, mates = _genes(), 2 if paired else 1
    for name, cut in _events(paired):
        n = len(pos) if cut is None else cut * mates
        b.add_event(genes[name], pos[:n] + (mc.SHIFT if name == "shifted" else 0), cig[:n])
    b.upload(0)
    for i, (name, cut) in enumerate(_events(paired)):
        m, fl = b.device_match_of(i)
        if paired:
            wm, wfl = gold.pe(name, ov, rl, mean, var)
        else:
            wm, wfl = gold.se(name, ov, rl), None
        n = len(wm) if cut is None else cut
        assert m.shape == (n, wm.shape[1]), (i, name, cut)
        assert np.array_equal(m != 0, wm[:n] != 0), (i, name, cut)
        if paired:
            assert np.array_equal(fl, wfl[:n]), (i, name, cut)
        else:
            assert np.isin(m, (0.0, 1.0)).all() and fl is None


@pytest.mark.parametrize("rl", mc.READ_LENS)
@pytest.mark.parametrize("ov", mc.OVERHANGS)
def test_one_launch_many_events_single_end(gold, ov, rl):
    _check_batch(gold, False, ov, rl)


@pytest.mark.parametrize("mean,var", mc.MEAN_VARS)
@pytest.mark.parametrize("rl", mc.READ_LENS)
@pytest.mark.parametrize("ov", mc.OVERHANGS)
def test_one_launch_many_events_paired_end(gold, ov, rl, mean, var):
    _check_batch(gold, True, ov, rl, mean, var)


def _same_run(a, b):
    assert np.array_equal(a.samples, b.samples) and np.array_equal(a.loglik, b.loglik, equal_nan=True)
    assert np.array_equal(a.assignment, b.assignment) and np.array_equal(a.counts_hash, b.counts_hash)
    assert np.array_equal(a.class_templates, b.class_templates) and np.array_equal(a.class_counts, b.class_counts)


def _same_as_checker(gpu, cpu, reassign=True):
    assert cpu.rc == 0
    assert np.array_equal(gpu.samples, cpu.samples) and np.array_equal(gpu.loglik, cpu.loglik, equal_nan=True)
    assert np.array_equal(gpu.assignment, cpu.assignment)
    if reassign:     # (MARGINAL keeps no counts, and its templates are divided by the effective lengths)
        assert np.array_equal(gpu.class_templates, cpu.class_templates) and np.array_equal(gpu.class_counts, cpu.class_counts)
        assert np.array_equal(gpu.counts_hash, cpu.trace["counts_hash"])
        assert np.array_equal(gpu.counts_trace, cpu.trace["counts_trace"])


@pytest.mark.parametrize("paired", [False, True])
def test_packing_of_reads_that_match_nothing(orc, gold, paired):
    """"tangled" and a wide gene, device-matched and host-matched, 60 iterations of 2 chains: the same samples, scores,
    assignment and read classes, and the checker's in counter mode."""
    mean, var = (120.0, 400.0) if paired else (0.0, 0.0)
    kw = dict(iters=60, burn=20, lag=2, chains=2, overhang=1)
    bkw = dict(kw, paired=paired, counts_trace=True, **(dict(mean=mean, var=var) if paired else {}))
    pos, cig, _ = mc.paired_reads(mean, var, 36) if paired else mc.single_reads()
    names = ("tangled", "wide33")
    for name in names:      # what this test is about: most of these reads (pairs) match no isoform
        m = gold.pe(name, 1, 36, mean, var)[0] if paired else gold.se(name, 1, 36)
        assert (m.any(axis=1)).mean() < 0.5
    dev, host = capi.Batch(36, device_match=True, **bkw), capi.Batch(36, **bkw)
    genes = _genes()
    for name in names:
        assert dev.add_event(genes[name], pos, cig) == host.add_event(genes[name], pos, cig)
    dev.run(seed=9, first_event_id=40); host.run(seed=9, first_event_id=40)
    for i, name in enumerate(names):
        a = dev.result(i, trace=True)
        _same_run(a, host.result(i, trace=True))
        og = orc.gene(flat(mc.gene(name)[0]), mc.gene(name)[1])
        if paired:
            cpu = orc.miso_paired(og, pos, cig, 36, mean, var, mode=OrcLib.COUNTER, seed=9, event_id=40 + i,
                                  trace=True, **kw)
        else:
            cpu = orc.miso(og, pos, cig, 36, mode=OrcLib.COUNTER, seed=9, event_id=40 + i, trace=True, **kw)
        _same_as_checker(a, cpu)


def test_marginal_reassignment_reads_the_raw_masks(orc):
    """algorithm = MARGINAL: sampler_marginal's final reassignment reads the masks as the kernel wrote them"""
    kw = dict(iters=60, burn=20, lag=2, chains=2, overhang=1, algo=capi.MISO_ALGO_MARGINAL)
    pos, cig, _ = mc.single_reads()
    dev, host = capi.Batch(36, device_match=True, **kw), capi.Batch(36, **kw)
    genes, names = _genes(), ("tangled", "wide33")
    for name in names:
        dev.add_event(genes[name], pos, cig); host.add_event(genes[name], pos, cig)
    dev.run(seed=4, first_event_id=7); host.run(seed=4, first_event_id=7)
    assert dev.last_kernels() == "sampler_marginal"
    for i, name in enumerate(names):
        a, h = dev.result(i), host.result(i)
        assert np.array_equal(a.samples, h.samples) and np.array_equal(a.loglik, h.loglik, equal_nan=True)
        assert np.array_equal(a.assignment, h.assignment)
        assert np.array_equal(a.class_templates, h.class_templates) and np.array_equal(a.class_counts, h.class_counts)
        og = orc.gene(flat(mc.gene(name)[0]), mc.gene(name)[1])
        cpu = orc.miso(og, pos, cig, 36, mode=OrcLib.COUNTER, seed=4, event_id=7 + i, **kw)
        _same_as_checker(a, cpu, reassign=False)
