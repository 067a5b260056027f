"""CPU: the restatement of the rank-normalised diagnostics (tests/_diag_rank_ref.py) against independent
routes -- scipy's average ranks and ndtri -- and against answers worked out by hand.  What the device computes is held
to rank_fixed bit for bit in tests/test_gpu_diagnostics_rank.py; this file is about rank_fixed being the definitions.
"""
import math

import numpy as np
import pytest
from scipy import special, stats

import _diag_rank_ref as RR
import _diag_ref as R


def all_ties_but_one(S):
    x = np.full(S, 0.25)
    x[S // 3] = 0.75
    return x


def scaled_chain(rng=None):
    """Four chains of 500 draws with the same mean; chain 3 has four times the spread of the others."""
    rng = rng or np.random.default_rng(41)
    x = R.ar1(rng, 0.0, 4, 500, mean=0.5, sd=0.02).reshape(500, 4)
    x[:, 3] = 0.5 + 4.0 * (x[:, 3] - 0.5)
    return x.reshape(-1)


@pytest.fixture(scope="module")
def qnorm(orc):
    return orc.lib.orc_det_qnorm


COLUMNS = {
    "no ties": lambda: R.ar1(np.random.default_rng(3), 0.3, 6, 50),
    "four decimals, 60 % repeats": lambda: RR.four_decimal_repeats(np.random.default_rng(4), 6, 50),
    "all ties but one": lambda: all_ties_but_one(300),
}


@pytest.mark.parametrize("name", list(COLUMNS))
def test_r2_is_twice_the_average_rank(name, qnorm):
    x = COLUMNS[name]()
    got = RR.rank_fixed(x, 6, 0.9, qnorm)
    v = x[RR.used_index(len(x), 6)]
    twice = 2.0 * stats.rankdata(v, method="average")
    assert got["r2"].dtype.kind == "i"
    assert np.array_equal(got["r2"].astype(np.float64), twice), name
    fold = np.abs(v - got["med"])
    assert np.array_equal(got["r2_fold"].astype(np.float64), 2.0 * stats.rankdata(fold, method="average")), name
    if name == "no ties":
        assert got["distinct"] == len(v)
    if name == "all ties but one":
        assert got["distinct"] == 2


def test_normal_scores_against_ndtri(qnorm):
    """Both routines are documented within about 1e-15 relative of the exact quantile (tests/test_detmath.py measures
    8.04e-16 for this one): 1e-14 between them.  p = 0.5 gives exactly 0."""
    worst = 0.0
    for N in (8, 48, 2700, 8192):
        r2 = np.arange(2, 2 * N + 1)                        # every value r2 can take: ranks 1, 1.5, .. N
        p = (0.5 * r2 - 0.375) / (N + 0.25)
        z = RR.normal_scores(r2, N, qnorm)
        want = special.ndtri(p)
        mid = r2 == N + 1
        assert mid.sum() == 1 and p[mid][0] == 0.5 and z[mid][0] == 0.0 and not np.signbit(z[mid][0])
        rel = np.abs(z[~mid] - want[~mid]) / np.abs(want[~mid])
        worst = max(worst, float(rel.max()))
        assert (np.diff(z) > 0).all()
    print("normal scores against ndtri: worst relative difference %.3e" % worst)
    assert worst <= 1e-14


def test_known_answers_of_sixteen_draws(qnorm):
    """C = 2, S = 18: n = 9, h = 4, N = 16; the middle draw of each chain (row 4) and nothing else is left out.  L = 0.5:
    lo = floor(4.5) - 1 = 3, hi = floor(12.5) - 1 = 11."""
    chain0 = [0.10, 0.20, 0.20, 0.35, 9.99, 0.40, 0.50, 0.50, 0.60]
    chain1 = [0.15, 0.20, 0.30, 0.35, 9.99, 0.45, 0.50, 0.55, 0.70]
    x = np.array([v for pair in zip(chain0, chain1) for v in pair])
    got = RR.rank_fixed(x, 2, 0.5, qnorm)
    # sorted used draws: .10 .15 .20 .20 .20 .30 .35 .35 | .40 .45 .50 .50 .50 .55 .60 .70
    assert (got["lo"], got["hi"]) == (3, 11)
    assert got["thr_lo"] == 0.20 and got["thr_hi"] == 0.50
    assert got["med"] == 0.5 * 0.35 + 0.5 * 0.40
    assert got["distinct"] == 11
    # e = j h + i: sequence 0 = chain 0's first four, 1 = its last four, 2 and 3 chain 1's
    assert got["r2"].tolist() == [2, 8, 8, 15,  18, 24, 24, 30,  4, 8, 12, 15,  20, 24, 28, 32]
    assert RR.used_index(18, 2).tolist() == [0, 2, 4, 6, 10, 12, 14, 16, 1, 3, 5, 7, 11, 13, 15, 17]
    for name in RR.OUTPUTS[:5]:
        assert math.isfinite(got[name]), name


@pytest.mark.parametrize("S,C,L,why", [
    (7, 1, 0.95, "Too few samples per chain for diagnostics"),
    (8, 1, 0.95, "Too few samples for a credible interval"),
    (8, 1, 0.5, None),
    (8192, 1, 0.95, None), (8193, 1, 0.95, None),
    (8194, 1, 0.95, "Too many samples for rank diagnostics"),
    (8192, 512, 0.95, None),
    (513 * 8, 513, 0.95, "Too many chains for rank diagnostics"),
    (513 * 16, 513, 0.95, "Too many samples for rank diagnostics"),     # N = 8208: the draws are counted first
    (18, 2, 0.5, None), (51, 6, 0.8, None), (2700, 6, 0.95, None),
    (16, 3, 0.5, "Too few samples per chain for diagnostics"),
    (40, 1, 0.95, "Too few samples for a credible interval"),           # lo = floor(1.5) - 1 = 0
    (60, 1, 0.95, None),                                                # lo = floor(2) - 1 = 1
])
def test_refusal_rules(S, C, L, why):
    assert RR.refusal(S, C, L) == why
    if why:
        with pytest.raises(ValueError, match=why):
            RR.rank_fixed(np.zeros(S), C, L, None)


def test_shapes_of_the_device_tests():
    """What tests/test_gpu_diagnostics_rank.py says about its shapes."""
    assert R.shape(8, 1)[3] == 8 and RR.bounds(8, 0.5) == (1, 5)
    assert R.shape(18, 2)[3] == 16
    assert R.shape(51, 6)[3] == 48 and RR.bounds(48, 0.8) == (4, 42)
    assert R.shape(8192, 512)[1:] == (8, 1024, 8192)


def test_a_chain_of_four_times_the_spread(qnorm):
    """Same mean, four times the spread: the raw R-hat and the bulk R-hat compare locations and stay near 1; the folded
    one sees it.  An ordering, not numbers."""
    x = scaled_chain()
    got = RR.rank_fixed(x, 4, 0.95, qnorm)
    classic = R.diag_fixed(x, 4)[0]
    print("scaled chain: classic rhat %.4f, rhat_bulk %.4f, rhat_fold %.4f" % (classic, got["rhat_bulk"], got["rhat_fold"]))
    assert got["rhat_fold"] > classic and got["rhat_fold"] > got["rhat_bulk"]


@pytest.mark.parametrize("name", ["no ties", "four decimals, 60 % repeats"])
def test_fixed_against_plain(name, qnorm):
    """The two restatements agree to rounding: same ranks, normal scores within 1e-14, sums in another order."""
    x = COLUMNS[name]()
    a, b = RR.rank_fixed(x, 6, 0.9, qnorm), RR.rank_plain(x, 6, 0.9)
    assert a["distinct"] == b["distinct"]
    for k in RR.OUTPUTS[:5]:
        assert a[k] == pytest.approx(b[k], rel=1e-9), k


def test_degenerate_columns(qnorm):
    x = R.ar1(np.random.default_rng(5), 0.3, 2, 40)
    for bad in (math.nan, math.inf, -math.inf):
        y = x.copy()
        y[7] = bad
        got = RR.rank_fixed(y, 2, 0.8, qnorm)
        assert all(math.isnan(got[k]) for k in RR.OUTPUTS[:5]) and got["distinct"] == 0
    const = RR.rank_fixed(np.full(80, 0.25), 2, 0.8, qnorm)
    assert all(math.isnan(const[k]) for k in RR.OUTPUTS[:5]) and const["distinct"] == 1
    y = x.copy()
    y[7] = 1e300
    huge = RR.rank_fixed(y, 2, 0.8, qnorm)
    assert all(math.isfinite(huge[k]) for k in RR.OUTPUTS[:5])
    assert math.isnan(R.diag_fixed(y, 2)[0])                # the raw pass overflows V
    # two values, as many of the one as of the other: the median lies halfway and every folded value is the same
    two = RR.rank_fixed(np.random.default_rng(6).permutation(np.repeat([0.25, 0.75], 40)), 2, 0.8, qnorm)
    assert math.isnan(two["rhat_fold"]) and two["distinct"] == 2
    assert all(math.isfinite(two[k]) for k in ("rhat_bulk", "ess_bulk", "ess_ci_low", "ess_ci_high"))
