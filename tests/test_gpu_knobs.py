"""GPU: WHEN the planner's MISO_* knobs (miso_amd/csrc/knobs.hpp) take effect.  The batch reads them at upload() and at
every launch(): a knob the plan depends on works from the next launch of an uploaded batch on, what upload() fixed -- the
slot order, the MODE 2 part -- stays until the next upload.  Bit for bit against the CPU checker either way."""
import pytest

import _convergent_cases as cc
from test_gpu_convergent_layouts import _env, _equal

pytestmark = pytest.mark.gpu


def _batch(case):
    import miso_amd
    b = miso_amd.Batch(36, paired=case.paired, mean=cc.MEAN if case.paired else 0.0, var=cc.VAR if case.paired else 0.0, **case.kw)
    for e in case.events:
        b.add_event(miso_amd.Gene(e.exons, e.isoforms), e.pos, e.cig)
    return b


def _launch(b, case):
    """one launch of the uploaded batch (bench.py time_batch): the first launch's kernels, then its results"""
    b.launch(seed=case.seed, first_event_id=case.first_id)
    first = b.last_kernels()            # (sync() appends the later rounds' kernels)
    b.sync()
    b.download()
    return first


def test_a_launch_knob_works_from_the_next_launch_on(orc):
    evs = [cc._event(orc, 2, 40, False, 8600 + j, 90 + 7 * j, 100) for j in range(16)]
    c = cc.Case("knobs_k2_se", False, dict(iters=200, burn=20, lag=2, chains=1), seed=29, first_id=4100, events=evs)
    cpu = c.reference(orc)
    b = _batch(c)
    with _env(MISO_LANES_PER_CHAIN="1"):
        b.upload(0)
        first = _launch(b, c)
    assert "sampler_k2<1, 0," in first, first
    for i, r in enumerate(cpu):
        _equal(b.result(i), r, ("one lane", i, first))
    with _env(MISO_LANES_PER_CHAIN="64"):
        again = _launch(b, c)           # the same uploaded batch
    assert "sampler_k2<64, 0," in again and "sampler_k2<1, 0," not in again, again
    for i, r in enumerate(cpu):
        _equal(b.result(i), r, ("a wavefront", i, again))


def test_what_upload_fixed_stays_fixed(orc):
    c = cc.case(orc, "k2_pe")
    cpu = c.reference(orc)
    with _env(MISO_NO_PE_DELTA=None):
        b = _batch(c)
        b.upload(0)
        first = _launch(b, c)
    assert "sampler_k2_multi<2, " in first, first
    stats = b.launch_stats()
    with _env(MISO_NO_PE_DELTA="1"):
        again = _launch(b, c)           # no new upload: the MODE 2 events keep their place in the list
        assert "sampler_k2_multi<2, " in again, again
        # ... and the launch still knows which they are: its statistics sort the events by the upload's use_delta, so a
        # launch that re-read the switch without rebuilding the lists would count other events' reads here
        assert b.launch_stats() == stats
        for i, r in enumerate(cpu):
            _equal(b.result(i), r, ("launched again", i, again))
        fresh = _batch(c)               # a batch uploaded under the setting
        fresh.upload(0)
        new = _launch(fresh, c)
    assert "sampler_k2_multi<1, " in new and "sampler_k2_multi<2, " not in new, new
    for i, r in enumerate(cpu):
        _equal(fresh.result(i), r, ("uploaded under the setting", i, new))
