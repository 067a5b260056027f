"""CPU: the arithmetic contract (include/miso_detmath.h, as the checker compiles it: orc_det_exp / log / sqrt,
orc_qnorm_det) against mpmath at 200 bits, on the point sets of tests/_detmath_points.py -- random sets over each
routine's range plus the places where a routine changes behaviour.  tests/test_gpu_primitives.py shows the device
equal to the host, bit for bit, on the same sets: together, device against exact.

Error unit: ulps of the double nearest the exact value (the subnormal spacing for subnormal results); the normal
quantile as relative error against sqrt(2) erfinv(2p - 1) in the centre and against the root of ncdf(z) = p in the tails."""
import math

import mpmath
import numpy as np

import _detmath_points as P

mpmath.mp.prec = 200
mpf = mpmath.mpf


def _call(f, xs):
    return np.array([f(float(v)) for v in xs], dtype=np.float64)


def _ulp_error(got, exact):
    """|got - exact| in ulps of the double nearest `exact`; inf where one of the two overflows and the other does not"""
    near = float(exact)                       # mpmath rounds to nearest
    if math.isinf(near) or math.isinf(got):
        return 0.0 if near == got else math.inf
    return float(abs(mpf(got) - exact) / mpf(math.ulp(near)))


def _worst(f, exact_fn, sets):
    worst = (0.0, None, None)
    for name, xs in sets.items():
        got = _call(f, xs)
        for x, g in zip(xs, got):
            e = _ulp_error(float(g), exact_fn(mpf(float(x))))
            if e > worst[0]:
                worst = (e, name, float(x).hex())
    return worst


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def test_exp_within_two_ulp_of_mpmath(orc):
    """Measured against mpmath.exp: worst 0.867 ulp (a subnormal result, where the final scaling rounds a second time);
    0.863 ulp among normal results.  The bound is the header's own."""
    worst = _worst(orc.lib.orc_det_exp, mpmath.exp, P.exp_points(20000))
    print("miso_det_exp: worst %.4f ulp in set %s at %s" % worst)
    assert worst[0] <= 2.0, worst


def test_log_within_two_ulp_of_mpmath(orc):
    """Measured against mpmath.log: worst 0.834 ulp.  The bound is the header's own."""
    worst = _worst(orc.lib.orc_det_log, mpmath.log, P.log_points(20000))
    print("miso_det_log: worst %.4f ulp in set %s at %s" % worst)
    assert worst[0] <= 2.0, worst


def test_sqrt_is_correctly_rounded(orc):
    """Bit-equal to the IEEE square root on every point (numpy.sqrt, itself checked against mpmath here on a
    sample and on every perfect square's neighbours): worst error 0.5000 ulp, tighter than the header's 1 ulp."""
    sets = P.sqrt_points(20000)
    for name, xs in sets.items():
        want = np.sqrt(xs)
        step = 1 if name in ("squares", "exponent_ends", "below_four") else 10
        for x, w in zip(xs[::step], want[::step]):
            assert float(mpmath.sqrt(mpf(float(x)))) == w, (name, float(x).hex())
        got = _call(orc.lib.orc_det_sqrt, xs)
        bad = np.nonzero(_bits(got) != _bits(want))[0]
        assert len(bad) == 0, (name, [(float(xs[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:5]])


def test_special_values_bit_for_bit(orc):
    """The header's stated special cases."""
    inf, nan = math.inf, math.nan
    L = orc.lib
    cases = [
        (L.orc_det_exp, [(inf, inf), (-inf, 0.0), (0.0, 1.0), (-0.0, 1.0), (710.0, inf), (-746.0, 0.0), (-1.0, None),
                         (1.0, None), (5e-324, 1.0), (-5e-324, 1.0), (nan, nan)]),
        (L.orc_det_log, [(inf, inf), (-inf, nan), (0.0, -inf), (-0.0, -inf), (1.0, 0.0), (-1.0, nan), (-5e-324, nan),
                         (nan, nan)]),
        (L.orc_det_sqrt, [(inf, inf), (-inf, nan), (0.0, 0.0), (-0.0, -0.0), (1.0, 1.0), (4.0, 2.0), (-1.0, nan),
                          (-5e-324, nan), (nan, nan), (5e-324, 2.0 ** -537)]),
        (L.orc_det_qnorm, [(0.0, -inf), (-0.0, -inf), (1.0, inf), (0.5, 0.0), (-1.0, nan), (math.nextafter(1.0, 2.0), nan),
                           (-5e-324, nan), (inf, nan), (-inf, nan), (nan, nan)]),
        (L.orc_qnorm_det, [(0.0, -inf), (-0.0, -inf), (1.0, inf), (0.5, 0.0), (-1.0, nan), (math.nextafter(1.0, 2.0), nan),
                           (-5e-324, nan), (inf, nan), (-inf, nan), (nan, nan)]),
    ]
    for f, pairs in cases:
        for x, want in pairs:
            got = f(x)
            if want is None:
                continue
            if math.isnan(want):
                assert math.isnan(got), (f.__name__, x, got)
            else:
                assert _bits([got])[0] == _bits([want])[0], (f.__name__, x, got, want)
    # exp(+-1) are ordinary points: nearest or next to nearest
    assert abs(L.orc_det_exp(1.0) - math.e) <= math.ulp(math.e)
    assert abs(L.orc_det_exp(-1.0) - 1 / math.e) <= math.ulp(1 / math.e)


def _quantile(p):
    """the exact lower-tail normal quantile of the double p in (0, 1), as an mpf"""
    p = mpf(p)
    if abs(p - 0.5) <= mpf("0.425"):
        return mpmath.sqrt(2) * mpmath.erfinv(2 * p - 1)
    upper = p > 0.5
    q = 1 - p if upper else p                 # exact at 200 bits
    # root of ncdf(z) = q, z < 0: Newton on log ncdf(z) = log q from the asymptotic guess (ncdf written with erfc, which
    # keeps its relative accuracy in the far tail); stops at a relative step below 1e-50
    cdf = lambda t: mpmath.erfc(-t / mpmath.sqrt(2)) / 2
    z = -mpmath.sqrt(-2 * mpmath.log(q))
    for _ in range(60):
        c = cdf(z)
        dz = mpmath.log(c / q) * c / mpmath.npdf(z)
        z = z - dz
        if abs(dz) <= mpf("1e-50") * abs(z):
            break
    else:
        raise AssertionError("no root for p = %s" % p)
    assert abs(cdf(z) - q) <= mpf("1e-45") * q
    return -z if upper else z


def test_qnorm_against_the_exact_quantile(orc):
    """orc_qnorm_det (the checker's AS241 with miso_det_log / miso_det_sqrt; orc_det_qnorm, the header's routine, must be
    bit-equal to it) and orc_qnorm_libm (the same AS241 with
    libm's, the reference's routine) against the exact quantile on the same points.
    |p - 0.5| <= 0.425: no transcendental involved, the two must be bit-equal.
    Outside: r = sqrt(-log p) moves by about an ulp between the two and the tail's rational function is close to linear
    in r, so the bound is the libm routine's worst relative error measured HERE plus 2 ulp (2 * 2^-52 = 4.44e-16).
    Measured: orc_qnorm_libm worst 8.04e-16, orc_qnorm_det worst 8.04e-16 relative (the same point, p = 0x1.0b2b9c8473b2fp-590:
    AS241's own error in the far tail); for p >= 1e-30 both stay below 6.5e-16."""
    worst_det, worst_libm = (0.0, None, None), (0.0, None, None)
    for name, ps in P.qnorm_points().items():
        det = _call(orc.lib.orc_qnorm_det, ps)
        # include/miso_detmath.h's miso_det_qnorm (the kernels' routine, its own copy of the tables) is the same function
        assert np.array_equal(_bits(_call(orc.lib.orc_det_qnorm, ps)), _bits(det)), name
        libm = _call(orc.lib.orc_qnorm_libm, ps)
        central = np.abs(ps - 0.5) <= 0.425
        assert np.array_equal(_bits(det[central]), _bits(libm[central])), name
        for p, d, l in zip(ps, det, libm):
            z = _quantile(float(p))
            if z == 0:
                assert d == 0.0 and l == 0.0
                continue
            ed, el = float(abs(mpf(float(d)) - z) / abs(z)), float(abs(mpf(float(l)) - z) / abs(z))
            if ed > worst_det[0]:
                worst_det = (ed, name, float(p).hex())
            if el > worst_libm[0]:
                worst_libm = (el, name, float(p).hex())
    print("orc_qnorm_det:  worst relative error %.3e in set %s at %s" % worst_det)
    print("orc_qnorm_libm: worst relative error %.3e in set %s at %s" % worst_libm)
    assert worst_libm[0] < 2e-15, worst_libm            # the yardstick itself is AS241: "about 1 part in 10^16"
    assert worst_det[0] <= worst_libm[0] + 2 * 2.0 ** -52, (worst_det, worst_libm)


def test_logfact_table_within_one_ulp_of_loggamma(orc):
    """include/miso_binomial.h miso_logfact_fill (a compensated sum of <= 1-ulp logs) against mpmath.loggamma(k + 1),
    k = 0 .. 120 000: twice the largest event of tests/test_gpu_collapsed.py.  Measured: worst 0.755 ulp (k = 6)."""
    n = 120001
    t = orc.logfact(n)
    assert _bits(t[:2]).tolist() == [0, 0]
    worst, at = 0.0, -1
    for k in range(2, n):
        e = _ulp_error(float(t[k]), mpmath.loggamma(k + 1))
        if e > worst:
            worst, at = e, k
    print("miso_logfact_fill: worst %.4f ulp at k = %d" % (worst, at))
    assert worst <= 1.0, (worst, at)
