"""The tail of the single-end two-isoform read loop (miso_amd/csrc/kernels_k2.inl, gibbs()).

Lane `sub` of a chain on GE lanes owns blocks sub + k GE, k = 0, 1, ... (stride position k); the chain's partial block is
block nfq = n_draw // 8.  A wavefront runs its stride positions in three parts: steady trips of UQ positions (every
block of every lane a full one, no range test), masked trips of UQ positions while at least UQ remain for the
wavefront's longest chain, and masked steps of ONE position for the fewer-than-UQ left.  These batches put the
drawing-read counts on every edge of that rule, for every lane layout the kernels have, bit for bit against the checker's
counter mode -- and assert, from the drawing-read counts the library itself reports, that every edge is met.
"""
import numpy as np
import pytest

import miso_amd
from _libs import OrcLib
from test_gpu_k2_read_loop import UQ, WIDE_LANES, WIDTHS, _drawing_reads, _event, _pred, _run_layouts

KW = dict(iters=300, burn=50, lag=5, chains=2)
# drawing reads per event, chosen on the CPU with _coverage() below so that every label of _wanted() is met: at most 2100
N_DRAW = [2100, 2049, 1999, 1543, 1537, 1417, 1409, 1031, 1025, 777, 775, 521, 519, 393, 385, 263, 257, 135, 129, 103,
          97, 71, 65, 41, 33, 23, 17, 15, 9, 7, 1, 0]
# The one-round launch gives a chain a whole workgroup of 512 lanes only from 16 x 512 drawing reads up (plan.cpp), so the
# workgroup-wide layout needs two larger events, in a batch of their own: two and three stride positions on 512 lanes
WIDE_DRAW = [8193, 8192]
# widths whose wavefronts hold chains of more than one event when every event has two chains: only there can a shorter
# chain's partial block sit in a masked UQ trip with a single step (the longer chain's) behind it
MIXED = tuple(w for w in WIDTHS if 64 // w > KW["chains"])


def _wave_parts(wave, lanes):
    """(steady trips, masked UQ trips, single steps) of a wavefront holding chains of `wave` drawing reads each, `lanes`
    lanes per chain: kernels_k2.inl's set-up, restated."""
    full, npos = None, 0
    for n in wave:
        nfq, rem = n >> 3, n & 7
        nblk = nfq + (1 if rem else 0)
        npos = max(npos, (nblk + lanes - 1) // lanes)
        for sub in range(lanes):
            fb = ((nfq - 1 - sub) // lanes + 1) if sub < nfq else 0
            full = fb // UQ if full is None else min(full, fb // UQ)
    left = npos - UQ * full
    return full, left // UQ, left % UQ


def _coverage(draws, chains, widths=WIDTHS):
    """Which of the tail's edges the events of one batch meet in single-width launches of `widths` lanes per chain and
    on whole workgroups: a set of labels, from their drawing-read counts alone."""
    seen = set()
    if 0 in draws:
        seen.add("n_draw=0")
    for n in draws:
        nblk = (n + 7) >> 3
        for lanes in WIDE_LANES[-1:]:   # a chain on a whole workgroup (512 lanes in a one-round launch), from 16 reads per lane up
            if n < 16 * lanes:
                continue
            npos = (nblk + lanes - 1) // lanes
            seen.add("%s single step, %d lanes" % ("one" if npos % UQ else "no", lanes))
            if npos % UQ and (n & 7) and (n >> 3) // lanes == npos - 1:
                seen.add("partial block in a single step, %d lanes" % lanes)
    # single-width launches: the launch's list is ordered by drawing reads, most first, every event with its chains,
    # 64 // lanes chains per wavefront
    order = sorted(draws, reverse=True)
    slots = [n for n in order for _ in range(chains)]
    for lanes in widths:
        cpw = 64 // lanes
        for s0 in range(0, len(slots), cpw):
            wave = slots[s0:s0 + cpw]
            full, masked, single = _wave_parts(wave, lanes)
            if max(wave) == 0:
                continue
            if single == 0:
                seen.add("no single step, %d lanes" % lanes)
            if single == 1 and full + masked > 0:
                seen.add("one single step, %d lanes" % lanes)
            if single == 1 and full + masked == 0:
                seen.add("single steps only, %d lanes" % lanes)
            for n in wave:
                nfq, rem = n >> 3, n & 7
                if rem == 0:
                    continue
                pos = nfq // lanes   # the partial block's stride position
                if single == 1 and pos == UQ * (full + masked) and rem in (1, 7):
                    seen.add("partial block in a single step, rem=%d, %d lanes" % (rem, lanes))
                if single == 1 and UQ * full <= pos < UQ * (full + masked):
                    seen.add("partial block in a masked trip, single step behind, %d lanes" % lanes)
    return seen


def _per_width(lanes):
    """The labels of one width; the last only where a wavefront holds chains of more than one event."""
    want = {"no single step, %d lanes" % lanes, "one single step, %d lanes" % lanes,
            "single steps only, %d lanes" % lanes, "partial block in a single step, rem=1, %d lanes" % lanes,
            "partial block in a single step, rem=7, %d lanes" % lanes}
    if lanes in MIXED:
        want.add("partial block in a masked trip, single step behind, %d lanes" % lanes)
    return want


def _wanted():
    """What the large batch meets.  A launch of one, two, three or four lanes per chain puts all its 64 chains on one to
    four wavefronts, whose tails the longest chains decide: those widths' other edges are the small batches' (_cases)."""
    want = {"n_draw=0"}
    for lanes in WIDTHS:
        want |= _per_width(lanes) if lanes >= 5 else {"one single step, %d lanes" % lanes}
    for lanes in MIXED:
        want.add("partial block in a masked trip, single step behind, %d lanes" % lanes)
    return want


def _cases(lanes):
    """Small batches (drawing reads per event) for a launch of `lanes` lanes per chain: every edge of _per_width()."""
    cases = [[16 * lanes], [24 * lanes], [8 * lanes], [16 * lanes + 1], [16 * lanes + 7], [7], [1], [0]]
    if lanes in MIXED:
        cases.append([24 * lanes, 7])
    return cases


def test_chosen_counts_cover_every_edge():
    assert UQ == 2, "the labels count at most one single step per wavefront"
    assert max(N_DRAW) <= 2100 and max(max(c) for w in WIDTHS for c in _cases(w)) <= 2100
    missing = _wanted() - _coverage(N_DRAW, KW["chains"])
    assert not missing, sorted(missing)
    assert not WIDE_WANTED - _coverage(WIDE_DRAW, KW["chains"], ()), sorted(WIDE_WANTED - _coverage(WIDE_DRAW, KW["chains"], ()))
    for lanes in WIDTHS:
        seen = set().union(*[_coverage(c, KW["chains"], (lanes,)) for c in _cases(lanes)])
        assert not _per_width(lanes) - seen, sorted(_per_width(lanes) - seen)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", WIDTHS)
def test_loop_tail_edges_of_one_width(orc, lanes):
    """Every edge of the tail in a launch of one width, each on a small batch of its own, with and without the rescan."""
    import os
    seen = set()
    names = ("MISO_LANES_PER_CHAIN", "MISO_K2_SETTLE_ALL", "MISO_K2_TARGET")
    saved = {k: os.environ.pop(k, None) for k in names}
    try:
        os.environ["MISO_LANES_PER_CHAIN"] = str(lanes)
        for ci, case in enumerate(_cases(lanes)):
            b = miso_amd.Batch(36, counts_trace=True, **KW)
            keep = []
            for i, n in enumerate(case):
                exons, isoforms, g, pos, cig = _event(orc, n, seed=6300 + 10 * ci + i)
                b.add_event(miso_amd.Gene(exons, isoforms), pos, cig)
                keep.append((g, pos, cig))
            draws = [_drawing_reads(b, i) for i in range(len(case))]
            assert draws == case, draws
            seen |= _coverage(draws, KW["chains"], (lanes,))
            cpu = [orc.miso(g, pos, cig, 36, mode=OrcLib.COUNTER, seed=80, event_id=800 + i, trace=True, **KW)
                   for i, (g, pos, cig) in enumerate(keep)]
            assert all(c.rc == 0 for c in cpu)
            for settle in (None, "1"):
                os.environ.pop("MISO_K2_SETTLE_ALL", None)
                if settle:
                    os.environ["MISO_K2_SETTLE_ALL"] = settle
                b.run(seed=80, first_event_id=800)
                for i in range(len(case)):
                    got = b.result(i, trace=True)
                    assert np.array_equal(got.counts_trace, cpu[i].trace["counts_trace"]), (case, settle, i)
                    assert np.array_equal(got.samples, cpu[i].samples), (case, settle, i)
                    assert np.array_equal(got.assignment, cpu[i].assignment), (case, settle, i)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert not _per_width(lanes) - seen, sorted(_per_width(lanes) - seen)


@pytest.mark.gpu
def test_loop_tail_edges_on_every_lane_layout(orc):
    b = miso_amd.Batch(36, counts_trace=True, **KW)
    keep = []
    for i, n in enumerate(N_DRAW):
        exons, isoforms, g, pos, cig = _event(orc, n, seed=6100 + i)
        b.add_event(miso_amd.Gene(exons, isoforms), pos, cig)
        keep.append((g, pos, cig))
    draws = [_drawing_reads(b, i) for i in range(len(N_DRAW))]
    assert draws == N_DRAW, draws
    missing = _wanted() - _coverage(draws, KW["chains"])
    assert not missing, sorted(missing)
    cpu = [orc.miso(g, pos, cig, 36, mode=OrcLib.COUNTER, seed=79, event_id=700 + i, trace=True, **KW)
           for i, (g, pos, cig) in enumerate(keep)]
    assert all(c.rc == 0 for c in cpu)
    _run_layouts(b, cpu, len(N_DRAW), seed=79, first_id=700)


WIDE_WANTED = {"no single step, 512 lanes", "one single step, 512 lanes", "partial block in a single step, 512 lanes"}


@pytest.mark.gpu
def test_loop_tail_of_chains_on_whole_workgroups(orc):
    """MISO_K2_TARGET=900: a bound on a wavefront's step so small that these events' chains take a whole workgroup each
    (GE = 512), with and without the rescan."""
    import os
    b = miso_amd.Batch(36, counts_trace=True, **KW)
    keep = []
    for i, n in enumerate(WIDE_DRAW):
        exons, isoforms, g, pos, cig = _event(orc, n, seed=6200 + i)
        b.add_event(miso_amd.Gene(exons, isoforms), pos, cig)
        keep.append((g, pos, cig))
    draws = [_drawing_reads(b, i) for i in range(len(WIDE_DRAW))]
    assert draws == WIDE_DRAW, draws
    assert not WIDE_WANTED - _coverage(draws, KW["chains"], ())
    cpu = [orc.miso(g, pos, cig, 36, mode=OrcLib.COUNTER, seed=81, event_id=750 + i, trace=True, **KW)
           for i, (g, pos, cig) in enumerate(keep)]
    assert all(c.rc == 0 for c in cpu)
    names = ("MISO_LANES_PER_CHAIN", "MISO_K2_SETTLE_ALL", "MISO_K2_TARGET")
    saved = {k: os.environ.pop(k, None) for k in names}
    try:
        os.environ["MISO_K2_TARGET"] = "900"
        for settle in (None, "1"):
            os.environ.pop("MISO_K2_SETTLE_ALL", None)
            if settle:
                os.environ["MISO_K2_SETTLE_ALL"] = settle
            b.run(seed=81, first_event_id=750)
            # a chain on up to 64 lanes is at most one wavefront: eight wavefronts per chain means every chain has a workgroup
            k = [x for x in b.launch_stats()["kernels"] if "sampler_k2_multi<0" in x["name"]]
            assert k and k[0]["waves"] >= 8 * k[0]["chains"], k
            for i in range(len(WIDE_DRAW)):
                got = b.result(i, trace=True)
                assert np.array_equal(got.counts_trace, cpu[i].trace["counts_trace"]), (settle, i)
                assert np.array_equal(got.samples, cpu[i].samples), (settle, i)
                assert np.array_equal(got.assignment, cpu[i].assignment), (settle, i)
    finally:
        for k_, v in saved.items():
            os.environ.pop(k_, None)
            if v is not None:
                os.environ[k_] = v


# (lanes per chain, seed): found on the CPU with the checker -- see _on_threshold_in_single_step().  The event has
# 8 x 3 x lanes drawing reads: three stride positions of full blocks, one steady trip and one single step.
FLAGGED = [(1, 10), (2, 7), (3, 3), (4, 4), (8, 1), (64, 1)]
FLAG_KW = dict(iters=400, burn=0, lag=1, chains=2)
FLAG_EVENT_ID = 900


def _on_threshold_in_single_step(orc, cpu, lanes, n_draw, seed):
    """Reads (iteration, chain, read) of the single step's blocks whose high half-word equals the threshold's while its
    low half-word is not 0, from the checker's psi samples and draws.  With burn = 0 and lag = 1 sample m of a chain is
    the psi the Gibbs step of iteration m draws with (kernels_k2.inl: recorded, then gibbs(m)); the test u < t is
    monotone in u, so hi == t >> 16 and t & 0xFFFF != 0 exactly where it holds at (hi << 16) and fails at (hi << 16) | 0xFFFF."""
    nblk = (n_draw + 7) >> 3
    npos = (nblk + lanes - 1) // lanes
    assert npos % UQ == 1, "the last stride position is a single step"
    first = 8 * (npos - 1) * lanes
    C = FLAG_KW["chains"]
    s = cpu.samples.reshape(-1, C, 2)
    found = []
    for m in range(FLAG_KW["iters"]):
        for ch in range(C):
            p0, p1 = s[m, ch]
            for r in range(first, n_draw):
                hi = orc.split_word(seed, FLAG_EVENT_ID, ch, m, r) >> 16
                if _pred(float(hi << 16), p0, p1) and not _pred(float((hi << 16) | 0xFFFF), p0, p1):
                    found.append((m, ch, r))
    return found


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,seed", FLAGGED)
def test_a_read_on_the_threshold_inside_a_single_block_step(orc, lanes, seed):
    """The flagged-step path (one flagged step of a lane: look() settles exactly its one block), without
    MISO_K2_SETTLE_ALL.  That such a read exists is asserted from the checker's own draws."""
    import os
    n_draw = 8 * 3 * lanes
    exons, isoforms, g, pos, cig = _event(orc, n_draw, seed=6500 + lanes)
    b = miso_amd.Batch(36, counts_trace=True, **FLAG_KW)
    b.set_event_id(b.add_event(miso_amd.Gene(exons, isoforms), pos, cig), FLAG_EVENT_ID)
    assert _drawing_reads(b, 0) == n_draw
    cpu = orc.miso(g, pos, cig, 36, mode=OrcLib.COUNTER, seed=seed, event_id=FLAG_EVENT_ID, trace=True, **FLAG_KW)
    assert cpu.rc == 0
    assert _on_threshold_in_single_step(orc, cpu, lanes, n_draw, seed), "no read on the threshold in the single step"
    names = ("MISO_LANES_PER_CHAIN", "MISO_K2_SETTLE_ALL", "MISO_K2_TARGET")
    saved = {k: os.environ.pop(k, None) for k in names}
    try:
        os.environ["MISO_LANES_PER_CHAIN"] = str(lanes)
        b.run(seed=seed, first_event_id=0)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    got = b.result(0, trace=True)
    assert np.array_equal(got.counts_trace, cpu.trace["counts_trace"])
    assert np.array_equal(got.samples, cpu.samples)
    assert np.array_equal(got.assignment, cpu.assignment)
