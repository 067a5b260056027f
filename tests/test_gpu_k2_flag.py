"""GPU: the trip flag of the single-end two-isoform read loop (csrc/k2_flag.hpp k2_flag_note / k2_flag_read) on the device,
one lane per element, against the numpy restatement of its definition (tests/_k2_flag_ref.py): a lane's sequence of (running
minimum, stride position) pairs reads out as none / one flagged trip at its position / more than one.  Cases: none; one at
position 0 and at the largest position; low half only, high half only; both halves of one word; two trips; 300, 65 536 and
70 000 flagged trips (no accumulator wraps to "none"); the words 0x00010001, 0xFFFF0000, 0x0000FFFF, 0; a few thousand
random sequences with about 1 % zero halves."""
import numpy as np
import pytest

import _k2_flag_ref as R
from miso_amd import capi

pytestmark = pytest.mark.gpu


def test_flag_read_out_matches_the_definition():
    m, k, start = R.flag_cases(np.random.default_rng(211), 3000)
    want_code, want_pos = R.flag_expected(m, k, start)
    assert {R.NONE, R.ONE, R.MANY} <= set(want_code.tolist())
    code, pos = capi.selftest_k2_flag(m, k, start)
    bad = np.nonzero(code != want_code)[0]
    assert len(bad) == 0, [(int(i), int(code[i]), int(want_code[i]), [hex(v) for v in m[start[i]:start[i + 1]][:8]]) for i in bad[:5]]
    one = want_code == R.ONE
    bad = np.nonzero(pos[one].astype(np.int64) != want_pos[one])[0]
    assert len(bad) == 0, [(int(pos[one][i]), int(want_pos[one][i])) for i in bad[:5]]

