"""CPU: the reference that tests/test_gpu_text_digits.py holds the device to does not rest on one formatter: Python's "%.4f"
against decimal.Decimal's exact expansion of the double, quantized half-even, on every point set of the device test."""
from fractions import Fraction

import numpy as np

import _text_points as P


def test_format_and_decimal_agree_on_every_point_set():
    for name, v in (("decimal ties", P.decimal_ties()), ("binary ties", P.binary_ties()), ("grid", P.grid()),
                    ("edges", P.edges()), ("random", P.random_unit(200000))):
        a, b = P.digits_by_format(v), P.digits_by_decimal(v)
        bad = np.nonzero(a != b)[0]
        assert len(bad) == 0, (name, [(float(v[i]).hex(), int(a[i]), int(b[i])) for i in bad[:5]])


def test_point_sets_hold_what_they_claim():
    t = P.decimal_ties()
    assert len(t) == 2 * 13 * 10001 and len(np.unique(t)) == len(t)
    for x in P.TIE_NEIGHBOURS:
        assert x in t and -x in t
    # a true tie: the exact product has fraction one half
    odd = [j / 32.0 for j in range(1, 65, 2)]
    assert all((Fraction(x) * 10000) % 1 == Fraction(1, 2) for x in odd)
    assert all(x in P.binary_ties() for x in odd)
    e = P.edges()
    assert np.abs(e).max() <= 2e5 + 1e-9 and (e == 0).sum() >= 2 and np.signbit(e[e == 0]).any()
    assert ((np.abs(e) > 0) & (np.abs(e) < 2.2250738585072014e-308)).any()            # subnormals


def test_the_rule_restated_with_the_exact_product_prints_what_format_prints():
    """csrc/text_digits.hpp in Python, the fma's error taken from the exact product: p = fl(10^4 v), e = 10^4 v - p,
    r = rint(p); only |p - r| = 1/2 needs e, and there its sign decides."""
    def rule(v):
        p = v * 10000.0
        e = Fraction(v) * 10000 - Fraction(p)
        r = float(np.rint(p))
        a = p - r
        if a == 0.5 and e > 0:
            r += 1.0
        elif a == -0.5 and e < 0:
            r -= 1.0
        return int(r)
    v = np.concatenate([P.decimal_ties(), P.binary_ties(), P.edges()[::7]])
    want = P.digits_by_format(v)
    bad = [(float(x).hex(), rule(x), int(w)) for x, w in zip(v.tolist(), want) if rule(x) != w]
    assert not bad, bad[:10]
