"""CPU: the law that include/miso_binomial.h's draws follow, counted over the 32-bit words they are functions of, against
the exact binomial probabilities -- every bin and every cumulative sum, at every k from 0 to n (tests/_binomial_law.py: the
method, the derived bound, the reference pmf -- scipy's, checked against mpmath on every call -- and the cases).

The kernels and the checker compile this one header, so every bit-for-bit test of the collapsed mode is silent about whether
its arithmetic is right; the chi-square of tests/test_collapsed.py sees a distortion of a probability from about one per cent.
This enumeration (every 4096th first word, the header's own routines reached one trial at a time through a preloaded
miso_ustream) sees 2e-6: a squeeze constant off in its third digit, a hat that fails to dominate at a few k, an off-by-one in m
or the table index.  tests/test_gpu_binomial_law.py runs the same enumeration on the device, down to every word."""
import pytest

import _binomial_law as L

STRIDE = 4096


@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_induced_law_is_the_binomial_law_within_the_derived_bound(orc, case):
    """|hist[k] / total - pmf(k)| <= (2 stride + 2) 2^-32 / accept + restarts / enumerated + 1e-12 at every k, the cumulative
    sums within twice that; the regime as info tells it; no restart; BTRS accepts at least 0.70 of its trials; k(U) does not
    decrease and the accepted second words are an initial segment (probed on one enumerated word in 2^8)."""
    n, p, regime = case
    hist, info = L.checker_law(orc, n, p, STRIDE)
    L.check_law(hist, info, n, p, STRIDE, regime)


def test_the_hook_refuses_what_miso_binomial_does_not_draw(orc):
    for n, p, stride in ((0, 0.5, 4096), (10, 0.0, 4096), (10, 1.0, 4096), (10, float("nan"), 4096), (10, 0.5, 0), (10, 0.5, 4095)):
        with pytest.raises(ValueError):
            orc.binomial_law(n, p, stride)

