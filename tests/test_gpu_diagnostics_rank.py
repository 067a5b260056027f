"""GPU: miso_batch_diagnose_rank (miso_amd/csrc/kernels_diagnose_rank.hip) against the restatement of
tests/_diag_rank_ref.py (rank_fixed, with the checker library's orc_det_qnorm): the five doubles bit for bit, `distinct`
as an integer.  Batches are adopted with SamplesBatch, at the smallest shapes at which each piece can go wrong:

    C = 1, S = 8, L = 0.5         N = 8, lo = 1, hi = 5: the minimum, the sort padded to 8
    C = 2, S = 18, L = 0.5        n = 9 odd, N = 16: the middle draw is not ranked
    C = 6, S = 51, L = 0.8        N = 48, lo = 4, hi = 42: a sort of 64 with padding, trailing columns ignored
    C = 1, S = 8192 and 8193      N = 8192: the largest accepted, the full network of 91 stages
    C = 512, S = 8192             h = 8, M = 1024: the most local memory, 152 KB
    C = 6, S = 2700               MISO's defaults
    K = 2, 3 and 40 in one batch: the grid's `k >= K` guard

(tests/test_diag_rank_ref.py test_shapes_of_the_device_tests holds those figures.)
"""
import math

import numpy as np
import pytest

import _diag_rank_ref as RR
import _diag_ref as R
from miso_amd import capi, workload

pytestmark = pytest.mark.gpu


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def qnorm(orc):
    return orc.lib.orc_det_qnorm


def _check_event(b, i, samples, C, L, qnorm, label):
    """Event i's six outputs against rank_fixed on every column; returns them."""
    got = b.rank_diagnostics(i)
    assert len(got) == 6 and got[5].dtype == np.int64
    for k in range(samples.shape[1]):
        want = RR.rank_fixed(samples[:, k], C, L, qnorm)
        g = [float(col[k]) for col in got[:5]]
        w = [want[name] for name in RR.OUTPUTS[:5]]
        print("%s event %d column %d: got %r %d want %r %d" % (label, i, k, g, got[5][k], w, want["distinct"]))
        assert int(got[5][k]) == want["distinct"], (label, i, k)
        for name, a, c in zip(RR.OUTPUTS, g, w):
            if math.isnan(c):
                assert math.isnan(a), (label, i, k, name, a)
            else:
                assert _bits(a) == _bits(c), (label, i, k, name, a, c)
    return got


def _psi_like(rng, S, K, C, phi=0.3):
    """[S, K] columns of AR(1) chains around distinct means (so the columns differ), rows in the file's layout."""
    cols = [R.ar1(rng, phi, C, -(-S // C), mean=0.2 + 0.6 * k / K, sd=0.04)[:S] for k in range(K)]
    return np.ascontiguousarray(np.stack(cols, axis=1))


SHAPES = [(8, 1, 0.5), (18, 2, 0.5), (51, 6, 0.8), (8192, 1, 0.95), (8193, 1, 0.95), (8192, 512, 0.95), (2700, 6, 0.95)]


@pytest.mark.parametrize("S,C,L", SHAPES)
def test_chosen_columns_bit_for_bit(S, C, L, qnorm):
    rng = np.random.default_rng(2025)
    events = [_psi_like(rng, S, K, C) for K in ((2, 3, 40) if S < 100 else (2,))]
    b = capi.SamplesBatch(events)
    b.diagnose_rank(C, L)
    for i, ev in enumerate(events):
        _check_event(b, i, ev, C, L, qnorm, "S=%d C=%d" % (S, C))
    many = b.rank_diagnostics_many(range(len(events)), [e.shape[1] for e in events])
    for i in range(len(events)):
        one = b.rank_diagnostics(i)
        assert len(many[i]) == 6 and many[i][5].dtype == np.int64
        for a, c in zip(many[i], one):
            assert np.array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(c) if c.dtype == np.float64 else c)
    assert b.rank_pass_ms() > 0.0


@pytest.mark.parametrize("S,C,L,why", [
    (8194, 1, 0.95, "Too many samples for rank diagnostics"),
    (513 * 8, 513, 0.95, "Too many chains for rank diagnostics"),
    (8, 1, 0.95, "Too few samples for a credible interval"),
    (7, 1, 0.95, "Too few samples per chain for diagnostics"),
])
def test_refusals(S, C, L, why):
    assert RR.refusal(S, C, L) == why
    b = capi.SamplesBatch([np.random.default_rng(1).random((S, 2))])
    with pytest.raises(capi.InternalError, match=why):
        b.diagnose_rank(C, L)
    with pytest.raises(capi.InternalError, match="has not run"):
        b.rank_diagnostics(0)


def test_ties(qnorm):
    rng = np.random.default_rng(8)
    repeats = np.stack([RR.four_decimal_repeats(rng, 6, 450), RR.four_decimal_repeats(rng, 6, 450)], axis=1)
    # two values, as many of the one as of the other: the median lies halfway and the folded column is constant
    two = np.stack([rng.permutation(np.repeat([0.25, 0.75], 1350)), rng.permutation(np.repeat([0.0, 1.0], 1350))], axis=1)
    b = capi.SamplesBatch([repeats, two])
    b.diagnose_rank(6, 0.95)
    got = _check_event(b, 0, repeats, 6, 0.95, qnorm, "repeats")
    assert (got[5] < 2700 // 2).all() and np.isfinite(np.stack(got[:5])).all()
    got = _check_event(b, 1, two, 6, 0.95, qnorm, "two-valued")
    assert got[5].tolist() == [2, 2] and np.isnan(got[1]).all()
    assert np.isfinite(np.stack([got[0], got[2], got[3], got[4]])).all()


@pytest.mark.parametrize("bad", ["constant", "nan", "inf", "huge"])
def test_degenerate_columns_beside_an_ordinary_one(bad, qnorm):
    S, C, L = 51, 6, 0.8
    rng = np.random.default_rng(7)
    ev = _psi_like(rng, S, 3, C)
    if bad == "constant":
        ev[:, 1] = 0.25
    else:
        ev[S // 3, 1] = {"nan": math.nan, "inf": math.inf, "huge": 1e300}[bad]
    other = _psi_like(rng, S, 2, C)
    b = capi.SamplesBatch([ev, other])
    b.diagnose_rank(C, L)
    got = _check_event(b, 0, ev, C, L, qnorm, bad)
    _check_event(b, 1, other, C, L, qnorm, "beside " + bad)
    mid = np.array([col[1] for col in got[:5]])
    if bad == "huge":
        assert np.isfinite(mid).all() and got[5][1] == 48
    else:
        assert np.isnan(mid).all() and got[5][1] == (1 if bad == "constant" else 0)
    assert np.isfinite(np.stack(got[:5])[:, [0, 2]]).all()


def test_an_outlier_is_its_rank(qnorm):
    """A draw that is the largest value and the largest fold stays both wherever it moves: six outputs bit-identical at
    0.99 and at 1e300, where the raw pass has nothing to say."""
    S, C = 600, 6
    base = _psi_like(np.random.default_rng(12), S, 2, C)
    base[:, 0] = np.clip(base[:, 0] - base[:, 0].mean() + 0.5, 0.3, 0.7)
    near, far = base.copy(), base.copy()
    near[100, 0], far[100, 0] = 0.99, 1e300
    b = capi.SamplesBatch([near, far])
    b.diagnose_rank(C, 0.95)
    b.diagnose(C)
    a = _check_event(b, 0, near, C, 0.95, qnorm, "outlier 0.99")
    c = _check_event(b, 1, far, C, 0.95, qnorm, "outlier 1e300")
    for x, y in zip(a, c):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))
    assert np.isfinite(np.stack(a[:5])).all()
    assert np.isfinite(b.diagnostics(0)[0]).all()
    assert math.isnan(b.diagnostics(1)[0][0]) and math.isfinite(b.diagnostics(1)[0][1])


def test_a_monotone_map_keeps_the_ranks(qnorm):
    """x -> x * x * x is strictly increasing on the four-decimal lattice in (0, 1): neighbours are 1e-4 apart, their cubes
    at least 1e-12, the two roundings move a cube by 2e-16 of itself.  Ranks, order statistics and ties are the same, so
    everything but the folded R-hat -- whose distances from the median the map does change -- is."""
    rng = np.random.default_rng(13)
    x = RR.four_decimal_repeats(rng, 6, 450, repeat=0.3)
    assert (x > 0).all() and (x < 1).all()
    cube = x * x * x
    assert len(np.unique(cube)) == len(np.unique(x))
    ev = np.stack([x, cube], axis=1)
    b = capi.SamplesBatch([ev])
    b.diagnose_rank(6, 0.95)
    got = _check_event(b, 0, ev, 6, 0.95, qnorm, "cube")
    for j in (0, 2, 3, 4, 5):
        assert got[j].view(np.int64)[0] == got[j].view(np.int64)[1], RR.OUTPUTS[j]
    assert np.isfinite(np.stack(got[:5])).all()


def test_sampler_batch(qnorm):
    b = capi.Batch(36, iters=600, burn=100, lag=5, chains=6)
    for e in range(4):
        exons, isoforms, pos, cig = workload.event_reads(e, K=2, n_reads=50)
        b.add_event(capi.Gene(exons, isoforms), pos, cig)
    with pytest.raises(capi.InternalError, match="not launched"):
        b.diagnose_rank()
    with pytest.raises(capi.InternalError):
        b.rank_diagnostics(0)
    b.run(device=0, seed=11, first_event_id=0)
    b.summarize(0.95)
    b.diagnose()
    before = [(b.summary(i), b.diagnostics(i)) for i in range(4)]
    b.diagnose_rank()
    for i in range(4):
        samples = b.result(i).samples
        assert samples.shape == (600, 2)
        _check_event(b, i, samples, 6, 0.95, qnorm, "sampled")
        for was, now in zip(before[i], (b.summary(i), b.diagnostics(i))):
            for x, y in zip(was, now):
                assert np.array_equal(x, y, equal_nan=True)
    b.launch(seed=12, first_event_id=0)
    with pytest.raises(capi.InternalError, match="has not run"):
        b.rank_diagnostics(0)
    b.sync()
    s = capi.SamplesBatch([np.random.default_rng(3).random((64, 2))])
    with pytest.raises(capi.InternalError, match="no chain count"):
        s.diagnose_rank()
    with pytest.raises(capi.InternalError, match="has not run"):
        s.rank_diagnostics(0)
    with pytest.raises(capi.InternalError):
        s.diagnose_rank(-1)
    s.diagnose_rank(2)
    assert s.rank_diagnostics(0)[0].shape == (2,)
