"""GPU: the exp / log of the two-isoform Metropolis-Hastings step with the route chosen per wavefront
(miso_amd/csrc/detmath_n.hpp det_exp_r / det_log_r, through miso_selftest_detmath_routed).

A wavefront whose 64 arguments all lie in the routine's domain -- exp: |x| <= 700; log: positive, normal, finite -- takes the
routine without special cases, any other wavefront the full routine for all of its lanes.  Both must return the host's
bits (orc_det_exp / orc_det_log, which tests/test_detmath.py ties to mpmath) on every lane, and the route each wavefront
took is asserted: without that, a test of the fast routines could pass on the full ones alone.

Every argument inside the domain runs once in a wavefront of such arguments only.  The specials do not go into all of those
wavefronts (thousands, times 10 specials, times 3 lanes) but into three of them -- the first, which holds the edges, the one a
third of the way in and the last -- each once per special and per lane 0, 37 and 63: the route test looks at one lane mask,
so which in-domain values sit beside the special does not matter to it, and every lane's bits are compared all the same.

Mutants this file is built to fail (docs/history.md says whether they were run): the exp bound widened to 720 -- the
wavefronts holding nextafter(700, inf), 709.79, 710 and 720 must report the full route; the class test without its "normal"
requirement -- the wavefronts holding a subnormal must, and the fast routine does not rescale one."""
import math

import numpy as np
import pytest

import _detmath_points as P
from miso_amd import capi

W = 64                       # lanes of a wavefront: elements 64 w .. 64 w + 63 of a call share one
LANES = (0, 37, 63)          # where a special replaces one argument of a wavefront
DBL_MIN, DBL_MAX = 2.2250738585072014e-308, 1.7976931348623157e308
SQRT2 = 1.4142135623730951
NAN, INF = float("nan"), float("inf")

EXP_EDGES = np.array([700.0, -700.0, math.nextafter(700.0, 0.0), math.nextafter(-700.0, 0.0), 0.0, -0.0, 1e-300, -1e-300,
                      699.9, -699.9,                                 # floor(x log2(e) + 0.5) = 1010, -1010
                      1009.5 / 1.4426950408889634 + 1e-9, -1009.5 / 1.4426950408889634 - 1e-9])   # the x nearest 0 of each
EXP_SPECIALS = [NAN, INF, -INF, math.nextafter(700.0, INF), math.nextafter(-700.0, -INF), -745.2, 709.79, 710.0, -746.0, 720.0]
LOG_EDGES = np.concatenate([[DBL_MIN, DBL_MAX, 1.0, math.nextafter(1.0, 0.0), math.nextafter(1.0, 2.0)],
                            P.around(SQRT2, 3), P.around(SQRT2, 3) * 2.0 ** -1022, P.around(SQRT2 / 2.0, 3) * 2.0 ** 1023])
LOG_SPECIALS = [NAN, INF, -INF, 0.0, -0.0, -1.0, -DBL_MIN, 5e-324, 1e-310, math.nextafter(DBL_MIN, 0.0)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _in_exp_domain(x):
    return np.abs(x) <= 700.0                    # (false for a NaN)


def _in_log_domain(x):
    return (x >= DBL_MIN) & (x <= DBL_MAX)       # positive, normal, finite (false for a NaN)


def _whole_wavefronts(x):
    """x, its last wavefront filled up with its own first points"""
    pad = -len(x) % W
    return np.concatenate([x, x[:pad]])


def _with_specials(base, specials):
    """the wavefronts of `base`, each once per (special, lane) with that one argument replaced"""
    waves = base.reshape(-1, W)
    out = []
    for s in specials:
        for lane in LANES:
            w = waves.copy()
            w[:, lane] = s
            out.append(w)
    return np.concatenate(out).reshape(-1)


class Case:
    def __init__(self, orc, fn, host_name, in_domain, points, edges, specials, extra=()):
        self.fn, self.in_domain = fn, in_domain
        pts = np.concatenate([edges] + [v for v in points.values()] + [P.all_arguments()] + list(extra))
        pts = pts[in_domain(pts)]
        self.inside = _whole_wavefronts(pts)
        # the specials go into the wavefronts that hold the edges and into two from the middle of the random sets
        n_waves = len(self.inside) // W
        pick = sorted({0, n_waves // 3, n_waves - 1})
        self.special = _with_specials(np.concatenate([self.inside[W * w:W * w + W] for w in pick]), specials)
        self.x = np.concatenate([self.inside, self.special])
        f = getattr(orc.lib, host_name)
        self.host = np.array([f(float(v)) for v in self.x])

    def check(self, force_full):
        n_in = len(self.inside)
        assert self.in_domain(self.inside).all() and n_in % W == 0 and len(self.special) % W == 0
        assert (~self.in_domain(self.special.reshape(-1, W))).sum(1).tolist() == [1] * (len(self.special) // W)
        dev, route = capi.selftest_detmath_routed(self.fn, self.x, force_full=force_full)
        want = np.full(len(self.x), capi.SELFTEST_ROUTE_FULL, np.int32)
        if not force_full:
            want[:n_in] = capi.SELFTEST_ROUTE_FAST
        wrong = np.flatnonzero(route != want)
        assert len(wrong) == 0, ("route", len(wrong), [(int(i), float(self.x[i]).hex(), int(route[i])) for i in wrong[:5]])
        nan = np.isnan(self.host)
        assert np.array_equal(np.isnan(dev), nan)
        bad = np.flatnonzero((_bits(dev) != _bits(self.host)) & ~nan)
        assert len(bad) == 0, ("bits", len(bad), [(float(self.x[i]).hex(), float(self.host[i]).hex(), float(dev[i]).hex())
                                                  for i in bad[:5]])


@pytest.fixture(scope="module")
def exp_case(orc):
    rng = np.random.default_rng(707)
    return Case(orc, capi.SELFTEST_EXP_R, "orc_det_exp", _in_exp_domain, P.exp_points(), EXP_EDGES, EXP_SPECIALS,
                extra=[rng.uniform(-700.0, 700.0, 100000)])


@pytest.fixture(scope="module")
def log_case(orc):
    return Case(orc, capi.SELFTEST_LOG_R, "orc_det_log", _in_log_domain, P.log_points(), LOG_EDGES, LOG_SPECIALS)


def test_edges_are_where_they_are_meant_to_be():
    log2e = 1.4426950408889634
    k = np.floor(EXP_EDGES * log2e + 0.5)
    assert k.max() == 1010 and k.min() == -1010 and _in_exp_domain(EXP_EDGES).all()
    assert not _in_exp_domain(np.array(EXP_SPECIALS)).any()
    assert _in_log_domain(LOG_EDGES).all() and not _in_log_domain(np.array(LOG_SPECIALS)).any()
    m = np.frexp(LOG_EDGES)[0] * 2.0             # mantissas in [1, 2): both sides of sqrt 2
    assert (m > SQRT2).any() and (m < SQRT2).any()


@pytest.mark.gpu
@pytest.mark.parametrize("force_full", [False, True])
def test_exp_routes_and_bits(exp_case, force_full):
    exp_case.check(force_full)


@pytest.mark.gpu
@pytest.mark.parametrize("force_full", [False, True])
def test_log_routes_and_bits(log_case, force_full):
    log_case.check(force_full)
