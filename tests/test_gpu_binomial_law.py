"""GPU: the law that include/miso_binomial.h's draws follow, counted on the device over the 32-bit words they are functions of
(include/miso_amd.h miso_selftest_binomial_law: the header's own miso_binomial_btrs / miso_binomial_inversion compiled for
gfx950 and reached one trial at a time; tests/_binomial_law.py: the method, the derived bound, the reference, the cases).

(a) At every 4096th first word the device's counts equal the CPU checker's integers: the header's arithmetic on gfx950 is the
    host's at every enumerated word and every bisected second word, not only on the 256 Philox draws per point of
    tests/test_gpu_primitives.py.
(b) At stride 1 -- every first word -- the counts are held to the exact probabilities by the same derived bound as on the CPU
    (tests/test_binomial_law.py): 4 * 2^-32 / accept + 1e-12, 0.9e-9 to 1.3e-9."""
import numpy as np
import pytest

import _binomial_law as L
from miso_amd import capi

pytestmark = pytest.mark.gpu

PARITY_STRIDE = 4096
PARITY = [(20, 0.5), (1000, 0.0101), (1000, 0.0099), (688, 0.31), (60000, 0.97), (100000, 0.00011)]
SHARP_STRIDE = 1
SHARP = [(20, 0.5), (30, 1 / 3), (1000, 0.0101), (688, 0.31), (100000, 0.4), (1000, 0.0099), (100000, 0.000099)]
_REGIME = {(n, p): regime for n, p, regime in L.CASES}


def _id(c):
    return L.case_id(c)


@pytest.mark.parametrize("case", PARITY, ids=_id)
def test_device_counts_equal_the_checkers(orc, case):
    n, p = case
    want_hist, want_info = L.checker_law(orc, n, p, PARITY_STRIDE)
    hist, info, _ = capi.selftest_binomial_law(n, p, PARITY_STRIDE)
    assert info == want_info, (n, p, info, want_info)
    bad = np.nonzero(hist != want_hist)[0]
    assert len(bad) == 0, (n, p, len(bad), [(int(k), int(hist[k]), int(want_hist[k])) for k in bad[:5]])
    assert info["regime"] == _REGIME[case]


@pytest.mark.parametrize("case", SHARP, ids=_id)
def test_device_law_is_the_binomial_law_at_the_finest_stride(case):
    """The assertions of tests/test_binomial_law.py (L.check_law) on the device's counts at SHARP_STRIDE.

    How the stride was chosen: stride 16 timed first (79 - 105 ms per BTRS case, 4 - 5 ms per inversion case), which scales to
    1.3 - 1.7 s at stride 1, so every first word is enumerated.  Measured at stride 1 on an MI355X (kernel time by HIP events):

      n, p              routine  kernel     accept  worst bin error (k)   bound     worst cumulative error (k)  bound
      20, 0.5           BTRS     1386 ms    0.7091  1.53e-10 (9)          1.31e-09  1.45e-10 (11)               2.63e-09
      30, 1/3           BTRS     1385 ms    0.7244  1.42e-10 (16)         1.29e-09  1.51e-10 (14)               2.57e-09
      1000, 0.0101      BTRS     1394 ms    0.7429  2.07e-10 (7)          1.25e-09  1.61e-10 (11)               2.51e-09
      688, 0.31         BTRS     1061 ms    0.8386  2.34e-10 (193)        1.11e-09  1.57e-10 (227)              2.22e-09
      100000, 0.4       BTRS     1045 ms    0.8817  2.22e-10 (39880)      1.06e-09  1.31e-10 (40053)            2.11e-09
      1000, 0.0099      INV        41 ms    1       2.05e-10 (27)         9.32e-10  2.18e-10 (1)                1.86e-09
      100000, 0.000099  INV        41 ms    1       2.25e-10 (0)          9.32e-10  2.35e-10 (34)               1.86e-09

    No restart, no word whose k is below the word's before, no probe that contradicts the initial segment (1.6e7 words probed
    per BTRS case).  The errors are one word's weight, 2^-32 = 2.3e-10.  With the header's squeeze constant 0.92 raised to
    0.93, (100000, 0.4) misses by a factor 1800 (bin error 1.94e-06, cumulative 2.55e-05)."""
    n, p = case
    hist, info, ms = capi.selftest_binomial_law(n, p, SHARP_STRIDE)
    print("kernel %.1f ms" % ms)
    L.check_law(hist, info, n, p, SHARP_STRIDE, _REGIME[case])


def test_the_entry_point_refuses_what_miso_binomial_does_not_draw():
    for n, p, stride in ((0, 0.5, 4096), (10, 0.0, 4096), (10, 1.0, 4096), (10, float("nan"), 4096), (10, 0.5, 0), (10, 0.5, 4095),
                         ((1 << 24) + 1, 0.5, 4096)):
        with pytest.raises(capi.InternalError, match="n: 1|p: inside|stride: a power"):
            capi.selftest_binomial_law(n, p, stride)
