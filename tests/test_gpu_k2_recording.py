"""GPU: which iterations of the two-isoform single-end sampler become samples (miso_amd/csrc/kernels_k2.inl, the recording
block of k2_body; the reference: miso.c:882-893).

From iteration `burn` on, every lag-th iteration's state is kept: iterations burn + lag - 1, burn + 2 lag - 1, ... below
`iters`, floor((iters - burn) / lag) per chain, the chains' samples interleaved (sample j of chain c in row j chains + c).
The kernel keeps that schedule per writing lane -- the next iteration to record and where its sample goes -- instead of the
reference's two counters, so every edge of the schedule is run here against the checker, bit for bit: no burn-in, a
burn-in that leaves one iteration, lags of 1, of more than one, of more than the iterations that remain (no sample at
all), 1, 3 and 6 chains, and a run of no iterations; in the planner's own launch and at 1, 2, 3, 4 and 8 forced lanes per
chain (every lane layout's copy of the block).

The checker returns chains (iters - burn) // lag rows, the reference's allocation; the rows beyond the kept ones stay
zero in both.  A kept row is a psi, which sums to 1, so the kept rows are counted as the rows that are not all zero."""
import itertools
import os
import re

import numpy as np
import pytest

import miso_amd
from _libs import OrcLib
from test_gpu_k2_read_loop import _drawing_reads, _event

ITERS = 37
BURNS = (0, 1, 5, 36)
LAGS = (1, 2, 3, 10, 40)
CHAINS = (1, 3, 6)
N_DRAW = (40, 57, 64, 83, 101, 128, 163, 200)       # 8 events of 40 .. 200 drawing reads
LANES = (1, 2, 3, 4, 8)
NAMES = ("MISO_LANES_PER_CHAIN", "MISO_K2_FULL_MATH", "MISO_K2_SETTLE_ALL", "MISO_K2_TARGET")
SEED, FIRST_ID = 311, 4200
CASES = [(ITERS, b, l, c) for b, l, c in itertools.product(BURNS, LAGS, CHAINS)] + [(0, 0, 1, c) for c in CHAINS]

_events, _cpu = [], {}


def kept_per_chain(iters, burn, lag):
    """iterations m in [burn, iters) with (m - burn) % lag == lag - 1"""
    return (iters - burn) // lag if iters > burn else 0


def last_iteration_kept(iters, burn, lag):
    return iters > burn and (iters - burn) % lag == 0


def _problem(orc):
    if not _events:
        for i, n in enumerate(N_DRAW):
            exons, isoforms, g, pos, cig = _event(orc, n, seed=8800 + i)
            _events.append((exons, isoforms, g, pos, cig))
    return _events


def _checker(orc, iters, burn, lag, chains):
    """the checker's outputs for every event of the problem, computed once per case and left unchanged"""
    key = (iters, burn, lag, chains)
    if key not in _cpu:
        out = [orc.miso(g, pos, cig, 36, iters=iters, burn=burn, lag=lag, chains=chains, mode=OrcLib.COUNTER, seed=SEED,
                        event_id=FIRST_ID + i, trace=True) for i, (_, _, g, pos, cig) in enumerate(_problem(orc))]
        assert all(c.rc == 0 for c in out), key
        _cpu[key] = out
    return _cpu[key]


def _kept_rows(samples):
    return int((np.asarray(samples).sum(axis=1) != 0.0).sum())


def test_cases_cover_the_schedules_edges(orc):
    """no GPU: the cases hold a run whose last iteration is a sample and runs without any sample, both read from the
    checker's own output; and the checker keeps floor((iters - burn) / lag) rows per chain in every case"""
    last, none = [], []
    for iters, burn, lag, chains in CASES:
        cpu = _checker(orc, iters, burn, lag, chains)
        want = chains * kept_per_chain(iters, burn, lag)
        for c in cpu:
            assert c.samples.shape[0] == chains * max(iters - burn, 0) // lag, (iters, burn, lag, chains)
            assert _kept_rows(c.samples) == want and int(c.rundata[8]) == c.samples.shape[0], (iters, burn, lag, chains)
        if want == 0 and iters > 0:
            none.append((iters, burn, lag, chains))
        if iters > 0 and want > 0:
            # the last iteration is a sample iff the run one iteration shorter keeps one sample per chain less (the draws
            # of an iteration depend on its number, not on the run's length: the shorter run's samples are a prefix)
            short = _checker(orc, iters - 1, burn, lag, chains) if iters - 1 >= 0 else None
            is_last = all(_kept_rows(s.samples) == want - chains and
                          np.array_equal(s.samples[:want - chains], c.samples[:want - chains]) for s, c in zip(short, cpu))
            assert is_last == last_iteration_kept(iters, burn, lag), (iters, burn, lag, chains)
            if is_last:
                last.append((iters, burn, lag, chains))
    assert last and none, (last, none)
    assert (ITERS, 36, 1, 1) in last and (ITERS, 5, 40, 3) in none and (ITERS, 36, 2, 1) in none


def _run_case(orc, iters, burn, lag, chains):
    cpu = _checker(orc, iters, burn, lag, chains)
    b = miso_amd.Batch(36, iters=iters, burn=burn, lag=lag, chains=chains)
    for exons, isoforms, _, pos, cig in _problem(orc):
        b.add_event(miso_amd.Gene(exons, isoforms), pos, cig)
    assert [_drawing_reads(b, i) for i in range(len(N_DRAW))] == list(N_DRAW)
    want = chains * kept_per_chain(iters, burn, lag)
    saved = {k: os.environ.pop(k, None) for k in NAMES}
    try:
        for env in [dict()] + [dict(MISO_LANES_PER_CHAIN=str(w)) for w in LANES]:
            for k in NAMES:
                os.environ.pop(k, None)
            os.environ.update(env)
            b.run(seed=SEED, first_event_id=FIRST_ID)
            if iters > 0:      # the layout asked for is the one that ran: the planner's kernel, or sampler_k2<lanes, ...>
                if not env:
                    assert "sampler_k2_multi<0, 8>" in b.last_kernels(), b.last_kernels()
                else:
                    assert re.match(r"sampler_k2<%s\b" % env["MISO_LANES_PER_CHAIN"], b.last_kernels()), (env, b.last_kernels())
            for i in range(len(N_DRAW)):
                got, what = b.result(i), (env, i)
                assert got.samples.shape == cpu[i].samples.shape and _kept_rows(got.samples) == want, what
                for c in range(chains):    # every chain keeps its own floor((iters - burn) / lag)
                    assert _kept_rows(got.samples[c::chains][:kept_per_chain(iters, burn, lag)]) == kept_per_chain(iters, burn, lag), what
                assert got.rundata.noSamples == int(cpu[i].rundata[8]), what
                assert np.array_equal(got.samples, cpu[i].samples), what
                assert np.array_equal(got.loglik, cpu[i].loglik), what
                assert (got.rundata.noAccepted, got.rundata.noRejected) == (cpu[i].accepted, cpu[i].rejected), what
                assert np.array_equal(got.counts_hash, cpu[i].trace["counts_hash"]), what
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.mark.gpu
@pytest.mark.parametrize("chains", CHAINS)
@pytest.mark.parametrize("burn", BURNS)
def test_recorded_iterations_are_the_checkers(orc, burn, chains):
    for lag in LAGS:
        _run_case(orc, ITERS, burn, lag, chains)


@pytest.mark.gpu
@pytest.mark.parametrize("chains", CHAINS)
def test_a_run_of_no_iterations_records_nothing(orc, chains):
    _run_case(orc, 0, 0, 1, chains)
