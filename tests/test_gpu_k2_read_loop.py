"""The single-end two-isoform read loop at its edges (miso_amd/csrc/kernels_k2.inl, gibbs()).

The loop runs a wavefront's first `full_trips` trips without any range test and the remaining ones masked; the chain's
partial generator block (n_draw % 8 reads) is block number nfq = n_draw // 8 of its lanes' stride.  These batches put the
drawing-read counts on every edge of that arithmetic, for every lane layout the kernels have, bit for bit against the
checker's counter mode -- and assert, from the drawing-read counts the library itself reports, that every edge is met.
"""
import os

import numpy as np
import pytest

import miso_amd
from _libs import OrcLib
from _problems import expr_for, flat, se_gene

pytestmark = pytest.mark.gpu

UQ = 2                      # blocks per lane and trip (MISO_K2_UQ)
WIDTHS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 32, 64)
WIDE_LANES = (256, 512)     # lanes of a workgroup-wide chain on one workgroup: four or eight wavefronts
KW = dict(iters=300, burn=50, lag=5, chains=2)
# drawing reads per event.  1920 = 15 * 128 full blocks is a whole number of trips for every width up to 64 lanes and 2048
# for a whole workgroup, so 15363 and 16387 need the extra trip for the partial block on every layout; 15357 / 15369 sit
# one block below / above; 15360 has no partial block and no tail trip at all.
N_DRAW = [16387, 15369, 15363, 15360, 15357, 3001, 1203, 777, 250, 100, 41, 33, 31, 23, 17, 16, 15, 9, 8, 7, 1, 0]
SKEW_DRAW = 43              # the two events with psi pinned to an end of [0, 1]: five full blocks and three reads


def _event(orc, n_draw, seed):
    """An exon-skipping event with exactly n_draw reads compatible with both isoforms."""
    exons, isoforms = se_gene(2)
    g = orc.gene(flat(exons), isoforms)
    orc.rng_seed(seed)
    rc, _, pos, cig = orc.simulate_reads(g, expr_for(2), max(3 * n_draw, 0) + 400, 36)
    assert rc == 0
    rc, m = orc.match_iso(g, pos, cig, 36)
    assert rc == 0
    both = (m[:, 0] != 0) & (m[:, 1] != 0)
    amb = np.flatnonzero(both)
    assert len(amb) >= n_draw
    rest = np.flatnonzero(~both & ((m[:, 0] != 0) | (m[:, 1] != 0)))[:max(n_draw // 2, 12)]
    idx = np.sort(np.concatenate([amb[:n_draw], rest]))
    return exons, isoforms, g, pos[idx], [cig[i] for i in idx]


def _drawing_reads(b, i):
    """Drawing reads of event i as the library classed them: the reads compatible with both isoforms."""
    ct, cc = b.classes(i)
    return int(sum(c for t, c in zip(ct, cc) if t[0] != 0 and t[1] != 0))


def _lane_trips(n_draw, sub, lanes):
    """(steady trips, trips) of lane `sub` of a chain on `lanes` lanes: kernels_k2.inl's set-up, restated."""
    nfq, rem = n_draw >> 3, n_draw & 7
    nblk = nfq + (1 if rem else 0)
    full = ((nfq - 1 - sub) // lanes + 1) if sub < nfq else 0
    return full // UQ, (nblk + UQ * lanes - 1) // (UQ * lanes)


def _coverage(draws, chains):
    """Which of the loop's edges the events meet: a set of labels, from their drawing-read counts alone."""
    seen = set()
    for n in draws:
        nfq, rem = n >> 3, n & 7
        if n == 0:
            seen.add("n_draw=0")
        if 0 < n < 8:
            seen.add("partial block only")
        for r in (0, 1, 7):
            if n > 0 and rem == r:
                seen.add("rem=%d" % r)
        for lanes in WIDTHS + WIDE_LANES:
            per = UQ * lanes
            if nfq > 0 and nfq % per == 0 and rem != 0:
                seen.add("extra trip, %d lanes" % lanes)
            if nfq > 1 and (nfq + 1) % per == 0 and rem != 0:
                seen.add("one below, %d lanes" % lanes)
            if nfq > 1 and (nfq - 1) % per == 0 and rem != 0:
                seen.add("one above, %d lanes" % lanes)
    # chains of very different sizes in one wavefront of a single-width launch: the launch's list is ordered by drawing
    # reads, most first, every event with its chains, 64 // lanes chains per wavefront
    order = sorted(draws, reverse=True)
    slots = [n for n in order for _ in range(chains)]
    for lanes in WIDTHS:
        cpw = 64 // lanes
        for s0 in range(0, len(slots), cpw):
            wave = slots[s0:s0 + cpw]
            per_lane = [_lane_trips(n, sub, lanes) for n in wave for sub in range(lanes)]
            full, trips = min(f for f, _ in per_lane), max(t for _, t in per_lane)
            if full == 0 and trips >= 3:
                seen.add("no steady trip, several tail trips")
            if 0 < full <= trips - 3:
                seen.add("steady trips and several tail trips")
            if 0 < full == trips:
                seen.add("no tail trip")
            if 0 < full == trips - 1:
                seen.add("one tail trip")
    return seen


def _wanted():
    want = {"n_draw=0", "partial block only", "rem=0", "rem=1", "rem=7", "no steady trip, several tail trips",
            "steady trips and several tail trips", "no tail trip", "one tail trip"}
    for lanes in WIDTHS + WIDE_LANES:
        want |= {"extra trip, %d lanes" % lanes}
    for lanes in WIDTHS:
        want |= {"one below, %d lanes" % lanes, "one above, %d lanes" % lanes}
    return want


def _layouts():
    """Every lane layout, each with and without the forced rescan: the planner's own mix, a bound on a wavefront's step
    so small that the largest events take a whole workgroup, and the single-width launches."""
    envs = [dict(), dict(MISO_K2_TARGET="900")] + [dict(MISO_LANES_PER_CHAIN=str(w)) for w in WIDTHS]
    return [dict(e, **s) for e in envs for s in (dict(), dict(MISO_K2_SETTLE_ALL="1"))]


def _run_layouts(b, cpu, n_events, seed, first_id):
    names = ("MISO_LANES_PER_CHAIN", "MISO_K2_SETTLE_ALL", "MISO_K2_TARGET")
    saved = {k: os.environ.pop(k, None) for k in names}
    stats = {}
    try:
        for env in _layouts():
            for k in names:
                os.environ.pop(k, None)
            os.environ.update(env)
            b.run(seed=seed, first_event_id=first_id)
            stats[tuple(sorted(env.items()))] = b.launch_stats()
            for i in range(n_events):
                got = b.result(i, trace=True)
                assert np.array_equal(got.counts_trace, cpu[i].trace["counts_trace"]), (env, i)
                assert np.array_equal(got.samples, cpu[i].samples), (env, i)
                assert np.array_equal(got.assignment, cpu[i].assignment), (env, i)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return stats


def test_read_loop_edges_on_every_lane_layout(orc):
    b = miso_amd.Batch(36, counts_trace=True, **KW)
    keep = []
    for i, n in enumerate(N_DRAW):
        exons, isoforms, g, pos, cig = _event(orc, n, seed=5100 + i)
        b.add_event(miso_amd.Gene(exons, isoforms), pos, cig)
        keep.append((g, pos, cig))
    draws = [_drawing_reads(b, i) for i in range(len(N_DRAW))]
    assert draws == N_DRAW, draws
    missing = _wanted() - _coverage(draws, KW["chains"])
    assert not missing, sorted(missing)
    cpu = [orc.miso(g, pos, cig, 36, mode=OrcLib.COUNTER, seed=77, event_id=300 + i, trace=True, **KW)
           for i, (g, pos, cig) in enumerate(keep)]
    assert all(c.rc == 0 for c in cpu)
    stats = _run_layouts(b, cpu, len(N_DRAW), seed=77, first_id=300)
    # the small bound did put chains on whole workgroups (the layouts whose stride is WIDE_LANES): a chain on up to 64
    # lanes is at most one wavefront, so more wavefronts than chains means workgroup-wide chains
    for env, st in stats.items():
        if dict(env).get("MISO_K2_TARGET"):
            k = [x for x in st["kernels"] if "sampler_k2_multi<0" in x["name"]]
            assert k and k[0]["waves"] > k[0]["chains"], st


def _pred(u, p0, p1):
    """The reference's test of uniform word u, in the device's own double arithmetic: u 2^-32 (psi_0 + psi_1) < psi_0.
    It is monotone in u, so the threshold t = #{u : test} is > u exactly where it holds."""
    return (u * (1.0 / 4294967296.0)) * ((0.0 + p0) + p1) < p0


@pytest.mark.parametrize("end", [0, 1])
def test_threshold_high_half_at_an_end_of_its_range(orc, end):
    """psi pinned to 1 (end = 0) or to 0 by a prior of 10^13 to 1: the chain spends thousands of steps at t = 2^32 (the
    closed form: th = 65536 does not fit a half-word, every read picks isoform 0, the partial block's owner adds its rem
    reads), some at th = 0xFFFF on its way there, or at th = 0 -- on events with a partial block, beside an ordinary event
    in the same wavefronts.  Which thresholds occurred is computed from the checker's psi samples and asserted."""
    kw = dict(iters=3000, burn=0, lag=1, chains=2)
    hyper = [1e13, 1.0] if end == 0 else [1.0, 1e13]
    b = miso_amd.Batch(36, counts_trace=True, **kw)
    keep = []
    for i, (n, hy) in enumerate([(SKEW_DRAW, hyper), (250, None), (8 * 12 + 5, hyper)]):
        exons, isoforms, g, pos, cig = _event(orc, n, seed=5300 + 10 * end + i)
        b.add_event(miso_amd.Gene(exons, isoforms), pos, cig, hyper=hy)
        keep.append((g, pos, cig, hy))
    draws = [_drawing_reads(b, i) for i in range(3)]
    assert draws == [SKEW_DRAW, 250, 8 * 12 + 5] and SKEW_DRAW % 8 != 0, draws
    cpu = [orc.miso(g, pos, cig, 36, mode=OrcLib.COUNTER, seed=78, event_id=500 + i, trace=True, hyper=hy, **kw)
           for i, (g, pos, cig, hy) in enumerate(keep)]
    assert all(c.rc == 0 for c in cpu)
    for i in (0, 2):
        s = cpu[i].samples.reshape(-1, 2)
        closed = _pred(4294967295.0, s[:, 0], s[:, 1])                    # t = 2^32: th = 65536
        at_ffff = _pred(float(0xFFFEFFFF), s[:, 0], s[:, 1]) & ~closed    # 0xFFFF0000 <= t < 2^32: th = 0xFFFF
        zero = ~_pred(float(0xFFFF), s[:, 0], s[:, 1])                    # t <= 0xFFFF: th = 0
        if end == 0:
            assert closed.sum() > 500 and at_ffff.sum() > 50, (i, closed.sum(), at_ffff.sum())
        else:
            assert zero.sum() > 500, (i, zero.sum())
    _run_layouts(b, cpu, 3, seed=78, first_id=500)
