"""Deterministic point sets for include/miso_detmath.h's routines, shared by tests/test_detmath.py (host against mpmath)
and tests/test_gpu_primitives.py (device against host): random sets over each routine's range plus the places where a
routine changes behaviour.  Every function returns {set name: float64 array}; nothing here depends on the code under test."""
import numpy as np

N_RANDOM = 12000       # points per random set
LN2 = 0.6931471805599453
SQRT2 = 1.4142135623730951
SPECIALS = np.array([np.inf, -np.inf, np.nan, -1.0, 0.0, -0.0, 1.0])


def around(x, k):
    """the doubles within k ulps of each finite non-zero x (2 k + 1 per point, x itself included)"""
    b = np.atleast_1d(np.asarray(x, dtype=np.float64)).view(np.int64)
    return (b[:, None] + np.arange(-k, k + 1, dtype=np.int64)[None, :]).reshape(-1).view(np.float64).copy()


def _pow2(e):
    return np.ldexp(1.0, np.asarray(e, dtype=np.int32))


def exp_points(n=N_RANDOM):
    rng = np.random.default_rng(101)
    k = np.arange(-1076, 1025, dtype=np.float64)
    return {
        "uniform": rng.uniform(-745.0, 709.7, n),
        "normal3": rng.normal(0.0, 3.0, n),
        "subnormal_results": rng.uniform(-745.2, -708.0, n),
        "halfway": around((k + 0.5) * LN2, 3),              # where the range reduction's k changes, every k
        "pow2": np.concatenate([s * _pow2(np.arange(-60, 10)) for s in (1.0, -1.0)]),
        "overflow": np.concatenate([around(709.782712893384, 4), around(710.0, 2), around(-710.0, 2)]),
        "underflow": np.concatenate([around(-745.2, 4), around(-746.0, 2), around(-745.13321910194122, 4)]),
        "tiny": np.array([5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308, 1e-300, -1e-300, 1e-17, -1e-17]),
    }


def log_points(n=N_RANDOM):
    rng = np.random.default_rng(102)
    e = np.arange(-1022, 1024)
    first = _pow2(e)
    last = np.nextafter(_pow2(e[1:]), 0.0)
    spread = _pow2(np.arange(-1022, 1023, 31))
    sub = rng.integers(1, 1 << 52, n, dtype=np.int64).view(np.float64)
    return {
        "exp_uniform": np.exp(rng.uniform(-700.0, 700.0, n)),
        "unit": 1.0 - rng.uniform(0.0, 1.0, n),            # (0, 1]
        "near_one": np.concatenate([1.0 + 10.0 ** -rng.uniform(0.0, 16.0, n // 2),
                                    1.0 - 10.0 ** -rng.uniform(0.0, 16.0, n // 2)]),
        "mantissa_range": rng.uniform(0.70, 1.42, n),
        "subnormal": np.concatenate([sub, [5e-324, 1e-323, 2.225073858507201e-308], _pow2(np.arange(-1074, -1022))]),
        "switch": around([np.sqrt(0.5), 1.0, SQRT2, 2.0, 0.5], 6),
        "binade_ends": np.concatenate([first, last, [1.7976931348623157e308]]),
        "sqrt2_mantissa": (around(SQRT2, 6)[None, :] * spread[:, None]).reshape(-1),
    }


def sqrt_points(n=N_RANDOM):
    rng = np.random.default_rng(103)
    e = np.arange(-1022, 1024)
    r = np.floor(rng.uniform(1.0, 2.0 ** 26, n // 3))
    sq = r * r                                              # exact: r < 2^26
    sq = np.concatenate([sq, sq * _pow2(rng.integers(-400, 400, len(sq)) * 2)])
    return {
        "full_range": np.exp(rng.uniform(-708.0, 709.0, n)),
        "one_to_four": rng.uniform(1.0, 4.0, n),
        "subnormal": np.concatenate([rng.integers(1, 1 << 52, n, dtype=np.int64).view(np.float64), [5e-324, 1e-323],
                                     _pow2(np.arange(-1074, -1022))]),
        "squares": np.concatenate([sq, np.nextafter(sq, 0.0), np.nextafter(sq, np.inf)]),
        "exponent_ends": np.concatenate([_pow2(e), np.nextafter(_pow2(e[1:]), 0.0), [1.7976931348623157e308]]),
        "below_four": (around(np.nextafter(4.0, 0.0), 3)[None, :] * _pow2(np.arange(-1020, 1020, 20))[:, None]).reshape(-1),
    }


def sampler_grid(u1, u2):
    """the argument miso_det_norm_from_unif hands to miso_det_qnorm for two [0, 1) uniforms"""
    return (np.floor(134217728.0 * u1) + u2) / 134217728.0


def qnorm_points(n=2500):
    """{set: p}, every p in (0, 1)"""
    rng = np.random.default_rng(104)
    lo_tail = 10.0 ** -rng.uniform(1.2, 300.0, n)
    up_tail = 1.0 - 10.0 ** -rng.uniform(1.2, 15.9, n)
    r5 = np.exp(-25.0)
    w1 = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.float64) / 4294967296.0
    w2 = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.float64) / 4294967296.0
    grid = sampler_grid(w1, w2)
    # the grid's own tails: the first and last cells of floor(2^27 u1)
    edge = np.concatenate([sampler_grid(np.zeros(n // 5), w2[:n // 5]),
                           sampler_grid(np.full(n // 5, 1.0 - 2.0 ** -32), w2[:n // 5])])
    out = {
        "centre": rng.uniform(0.075, 0.925, n),
        "lower_tail": lo_tail,
        "upper_tail": up_tail[up_tail < 1.0],
        "near_half": np.concatenate([0.5 + s * 10.0 ** -rng.uniform(0.5, 16.0, n // 4) for s in (1.0, -1.0)] + [[0.5]]),
        "offset_grid": (rng.integers(0, 1 << 27, n).astype(np.float64) + 0.37) / 134217728.0,
        "central_switch": np.concatenate([around(0.075, 4), around(0.925, 4)]),
        "r5_switch": np.concatenate([around(r5, 4), around(1.0 - r5, 4)]),
        "ends": np.array([5e-324, 1e-310, 2.2250738585072014e-308, 1e-300, 1.0 - 2.0 ** -53, 1.0 - 2.0 ** -52, 2.0 ** -53]),
        "sampler_grid": np.concatenate([grid, edge]),
    }
    for k, v in out.items():
        out[k] = v[(v > 0.0) & (v < 1.0)]
    return out


def all_arguments():
    """every point of the four families and the special values, one array: what the device-against-host tests evaluate"""
    parts = [SPECIALS]
    for fam in (exp_points(), log_points(), sqrt_points(), qnorm_points()):
        parts.extend(fam.values())
    return np.concatenate(parts)
