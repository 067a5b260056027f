"""The batches of tests/_convergent_cases.py are not vacuous: on the CPU checker alone, the rounds every event takes under
stop = CONVERGENT_MEAN.  The GPU tests compare the device with the checker on these batches; a batch whose events all
stopped after one round would compare nothing of the rule."""
import pytest

import _convergent_cases as cc


def _rounds(orc, names):
    return {n: cc.case(orc, n).rounds(orc) for n in names}


def test_rounds_are_recovered_from_the_accept_counts(orc):
    """rounds_of against a schedule whose rounds are known: max_iters stops the loop after exactly r rounds when the chains
    have no chance to converge first (two kept iterations in the first round)"""
    for paired in (False, True):
        ev = cc._event(orc, 5, 200, paired, 8400, 500 if paired else 120, 300 if paired else 100)
        for r in range(1, 7):
            kw = dict(iters=10, burn=8, lag=1, chains=2, stop=1)
            kw["max_iters"] = cc.schedule(kw, r)[-1][0]
            c = cc.Case("known", paired, kw, seed=3, first_id=0, events=[ev])
            free = cc.Case("free", paired, dict(kw, max_iters=10 ** 7), seed=3, first_id=0, events=[ev])
            assert c.rounds(orc) == [min(r, free.rounds(orc)[0])], (paired, r)
        assert free.rounds(orc)[0] >= 6, free.rounds(orc)


def test_deep_batches_go_beyond_eight_rounds(orc):
    r = _rounds(orc, cc.DEEP_NAMES)
    se = [x for n in cc.DEEP_NAMES if "_se_" in n for x in r[n]]
    pe = [x for n in cc.DEEP_NAMES if "_pe_" in n for x in r[n]]
    assert sum(x >= 9 for x in se) >= 3, r
    assert sum(x >= 9 for x in pe) >= 1, r
    both = se + pe
    assert 4 in both and 8 in both and any(5 <= x <= 7 for x in both), r


@pytest.mark.parametrize("name", cc.LAYOUT_NAMES)
def test_layout_batches_take_several_rounds_and_not_all_the_same(orc, name):
    r = cc.case(orc, name).rounds(orc)
    assert len(set(r)) >= 2 and max(r) >= 3, (name, r)


def test_collapsed_batches_hold_events_of_no_and_of_one_ambiguous_read(orc):
    for name in ("collapsed_k2", "collapsed_mix"):
        c = cc.case(orc, name)
        amb = [cc.ambiguous_reads(x) for x, e in zip(c.reference(orc), c.events) if e.mode == cc.OrcLib.COLLAPSED]
        assert 0 in amb and 1 in amb, (name, amb)


def test_lag_remainder_batches_leave_rows_unfilled(orc):
    """24 / 8 with three chains: the kept windows are 16 and 32 iterations.  Lag 3 leaves a remainder in both rounds and a row
    nobody fills in both (16 rows for 3 x 5 samples, 32 for 3 x 10); lag 7 leaves a remainder of the chains' total in both
    (3 x 16 = 48, 3 x 32 = 96) and an unfilled row in the second (13 rows for 3 x 4), which is among the last noSamples = 6
    that a second round returns."""
    for name in cc.LAG_NAMES:
        c = cc.case(orc, name)
        kw = c.kw
        for N, B in cc.schedule(kw, 2):
            assert (N - B) % kw["lag"] != 0, (name, N, B)
        r = c.rounds(orc)
        assert len(set(r)) >= 2 and min(r) >= 2 and max(r) >= 3, (name, r)
    lag3, lag7 = cc.case(orc, "lag3").kw, cc.case(orc, "lag7").kw
    assert cc.unfilled_rows(lag3, 1) == 1 and cc.unfilled_rows(lag3, 2) == 2
    for N, B in cc.schedule(lag7, 2):
        assert lag7["chains"] * (N - B) % lag7["lag"] != 0, (N, B)
    assert cc.unfilled_rows(lag7, 2) == 1


def test_schedule_edges_are_the_edges(orc):
    for ev in cc.EDGE_EVENTS:
        r = {s: cc.case(orc, "edge_%s_%s" % (ev, s)).rounds(orc)[0] for s in cc.EDGE_SCHEDULES}
        assert r["burn_is_iters"] == 1, (ev, r)                 # no kept sample: nothing to assess
        assert r["burn0"] >= 2, (ev, r)
        # maxIterations <= noIterations ends the loop (miso.c:908): a second round of N = max_iters is the last, one more allows a third
        assert r["max_is_second_N"] == 2 and r["max_is_second_N_plus_1"] == 3, (ev, r)
        assert r["chains2"] >= 2 and r["chains6"] >= 2, (ev, r)
