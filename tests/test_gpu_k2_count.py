"""GPU: the assembly statements of the single-end two-isoform read loop's per-word arithmetic (csrc/k2_count.hpp
k2_count_pair, the steady trips' form, and k2_count_pair_masked, the tail's) on the device, one lane per element, against the
same header's plain functions compiled for the host (tools/k2_count_host.cpp) and the numpy restatement of the definition
(tests/_k2_count_ref.py): every threshold against the halves next to it and at both ends of the range, every half against
the thresholds at the ends, and 3000 random sequences with about 1 % of halves on or next to the threshold."""
import numpy as np
import pytest

import _k2_count_ref as R
from miso_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return R.build_host(tmp_path_factory.mktemp("k2_count"))


def _check(prog, tmp_path, th, start, u, inv, masked):
    n = len(th)
    out = R.run_host(prog, "seq", [[n, len(u)], start, th, u, inv], tmp_path)
    acc, o = capi.selftest_k2_count(th, start, u, inv, masked)
    want_acc, want_o = R.seq_expected(th, start, u, inv)
    assert np.array_equal(out[:n], want_acc) and np.array_equal(out[n:], want_o)      # host functions == definition
    bad = np.nonzero((acc != out[:n]) | (o != out[n:]))[0]                            # assembly == host functions
    assert len(bad) == 0, [(int(i), int(th[i]), hex(int(acc[i])), hex(int(out[i])), hex(int(o[i])), hex(int(out[n + i])))
                           for i in bad[:5]]


def test_steady_and_masked_statements_on_the_edge_cases(prog, tmp_path):
    rng = np.random.default_rng(51)
    th, start, u, inv = R.edge_sequences(rng)
    n = len(th)
    _check(prog, tmp_path, th, start, u, inv, np.zeros(n, np.int32))                  # the steady form
    _check(prog, tmp_path, th, start, u, inv, np.ones(n, np.int32))                   # the masked form, nothing masked
    inv = R.INVS[rng.integers(0, 4, len(u))]
    _check(prog, tmp_path, th, start, u, inv, np.ones(n, np.int32))                   # ... and with masks


def test_random_sequences(prog, tmp_path):
    rng = np.random.default_rng(52)
    th, start, u, inv = R.random_sequences(rng, 3000)
    thw = np.repeat(th.astype(np.int64), np.diff(start))
    near = (np.abs((u & 0xFFFF).astype(np.int64) - thw) <= 1) | (np.abs((u >> 16).astype(np.int64) - thw) <= 1)
    assert 0.005 < near.mean() < 0.05, near.mean()
    _check(prog, tmp_path, th, start, u, inv, np.ones(len(th), np.int32))
    _check(prog, tmp_path, th, start, u, np.zeros(len(u), np.uint32), np.zeros(len(th), np.int32))
