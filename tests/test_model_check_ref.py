"""The model check's yardstick (tests/_model_check_ref.py) against what it must be: its single binomials against the
checker's own (same word streams), and its law against exact enumeration.  No GPU."""
import numpy as np
import pytest
import _model_check_ref as ref
from _libs import OrcLib

from _model_check_ref import ENUM_M, ENUM_N, ENUM_PATTERN, ENUM_PSI, ENUM_ROWS, check_enum, enum_exact


@pytest.fixture(scope="module")
def orc():
    return OrcLib()


@pytest.mark.parametrize("n,p", [(6, 0.3), (40, 0.02), (9, 0.93), (200, 0.5), (1000, 0.3), (100000, 0.0001),
                                 (100000, 0.2), (5000, 0.999), (7, 0.0), (7, 1.0)])
def test_single_binomials_equal_the_checkers(orc, n, p):
    """the restated BINV / BTRS on the checker's addresses (site 3, chain 0, iteration i) give orc_binomial's draws"""
    M = ref.Math(orc)
    lf = orc.logfact(n + 1)
    want = orc.binomial(n, p, 24, seed=77, event_id=5)
    got = [ref.binomial(M, ref.Stream(orc, 77, 5, 0, i, 3), n, p, lf) for i in range(24)]
    assert got == list(want)


def test_enumerated_law(orc):
    """8192 constant rows, N = 6, C = 3: exceed / rows and every tail within 5 binomial standard errors of the exact value"""
    samples = np.tile(np.array(ENUM_PSI), (ENUM_ROWS, 1))
    r = ref.model_check(orc, ENUM_PATTERN, ENUM_M, ENUM_N, samples, event_id=11, seed=2024)
    assert r["status"] == "ok"
    check_enum(r)
    # the class probabilities do not depend on the row: expected = N p
    p = enum_exact()[0]
    assert np.allclose(r["expected"], 6 * p, rtol=1e-12)


def test_statuses_and_bad_rows(orc):
    rows = np.array([[0.5, 0.5], [0.0, 0.0], [np.nan, 0.5], [0.25, 0.75]])
    r = ref.model_check(orc, ENUM_PATTERN, ENUM_M, ENUM_N, rows, 0, 1)
    assert (r["status"], r["rows"], r["bad_rows"]) == ("ok", 2, 2)
    assert ref.model_check(orc, ENUM_PATTERN, ENUM_M, [0, 0, 0], rows, 0, 1)["status"] == "no_reads"
    assert ref.model_check(orc, ENUM_PATTERN, ENUM_M, ENUM_N, rows[1:3], 0, 1)["status"] == "no_rows"
    assert ref.model_check(orc, [1] * 65, [1] * 65, [1] * 65, rows, 0, 1)["status"] == "too_many_classes"
