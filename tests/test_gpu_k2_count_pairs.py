"""GPU: the word PAIR of the single-end two-isoform read loop (csrc/k2_count.hpp k2_count_pair / k2_count_pair_masked: two
words' classes go into the packed counters with ONE three-input add and into the trip's flag word with ONE three-input or)
through miso_selftest_k2_count, one lane per element, against the same header's plain functions compiled for the host
(tools/k2_count_host.cpp) and the numpy restatement of the definition (tests/_k2_count_ref.py).

* every combination of classes over the four halves of a pair -- above the threshold, on it, one below (d = 2: the cap's
  first value) and far below: 256 -- as the trip's first pair (o = c_a | c_b) and as a later pair (o |= c_a | c_b, behind
  another combination), in the steady form and in the masked form with every inv of {0, 0x0000FFFF, 0xFFFF0000, 0xFFFFFFFF}
  on either word, at th 0, 1, 0x7FFF, 0xFFFE, 0xFFFF (at the ends of the range some classes do not exist: their halves are
  kept inside the range and fall into a neighbouring class);
* a lane of 8190 blocks' words all far below: both counters end at 65 520 = 8190 x 8 and the three-input add carries nothing
  from the low counter into the high one; the same with the last pair's four halves on the threshold;
* 2000 random sequences of even length."""
import numpy as np
import pytest

import _k2_count_ref as R
from miso_amd import capi

pytestmark = pytest.mark.gpu

TH = (0, 1, 0x7FFF, 0xFFFE, 0xFFFF)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return R.build_host(tmp_path_factory.mktemp("k2_count_pairs"))


def _check(prog, tmp_path, th, start, u, inv, masked):
    n = len(th)
    out = R.run_host(prog, "seq", [[n, len(u)], start, th, u, inv], tmp_path)
    acc, o = capi.selftest_k2_count(th, start, u, inv, masked)
    want_acc, want_o = R.seq_expected(th, start, u, inv)
    assert np.array_equal(out[:n], want_acc) and np.array_equal(out[n:], want_o)      # host functions == definition
    bad = np.nonzero((acc != out[:n]) | (o != out[n:]))[0]                            # assembly == host functions
    assert len(bad) == 0, [(int(i), int(th[i]), hex(int(acc[i])), hex(int(out[i])), hex(int(o[i])), hex(int(out[n + i])))
                           for i in bad[:5]]
    return acc, o


def _class_halves(th):
    """the four halves that stand for above, on, one below, far below at th"""
    return np.array([min(th + 1, 0xFFFF), th, max(th - 1, 0), th // 3], np.uint32)


def _pairs(th):
    """[256, 2]: the word pair of every combination of classes over (a.lo, a.hi, b.lo, b.hi)"""
    v = _class_halves(th)
    k = np.arange(256)
    a = v[k & 3] | (v[(k >> 2) & 3] << np.uint32(16))
    b = v[(k >> 4) & 3] | (v[(k >> 6) & 3] << np.uint32(16))
    return np.stack([a, b], axis=1).astype(np.uint32)


def _combination_sequences(inva, invb):
    """(th, start, u, inv): per th the 256 pairs alone (the trip's first pair) and each behind another combination's pair (a
    later pair); inva / invb: the masks of the pair under test's two words (the pair ahead of it is not masked)"""
    ths, us, invs, lens = [], [], [], []
    for th in TH:
        p = _pairs(th)
        ahead = p[(np.arange(256) * 7 + 3) % 256]
        ths += [np.full(512, th)]
        us += [p.ravel(), np.concatenate([ahead, p], axis=1).ravel()]
        invs += [np.tile([inva, invb], 256), np.tile([0, 0, inva, invb], 256)]
        lens += [np.full(256, 2), np.full(256, 4)]
    start = np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.int64)
    return np.concatenate(ths).astype(np.uint32), start, np.concatenate(us).astype(np.uint32), np.concatenate(invs).astype(np.uint32)


def test_class_values_cover_the_four_classes_where_they_exist():
    c = R.half_class(0x7FFF, _class_halves(0x7FFF))
    assert list(c) == [0, 1, 2, 2] and 0x7FFF + 1 - int(_class_halves(0x7FFF)[2]) == 2      # d = 2 exactly, and d far above it
    assert len(np.unique(_pairs(0x7FFF), axis=0)) == 256


def test_every_class_combination_steady(prog, tmp_path):
    th, start, u, inv = _combination_sequences(0, 0)
    acc, o = _check(prog, tmp_path, th, start, u, inv, np.zeros(len(th), np.int32))
    # the all-far-below pair at th = 0x7FFF, alone: every half counts 2, no read on the threshold
    i = 2 * 512 + 255
    assert acc[i] == 0x00040004 and o[i] == 0x00020002


@pytest.mark.parametrize("inva", [int(x) for x in R.INVS])
def test_every_class_combination_masked(prog, tmp_path, inva):
    for invb in R.INVS:
        th, start, u, inv = _combination_sequences(inva, int(invb))
        _check(prog, tmp_path, th, start, u, inv, np.ones(len(th), np.int32))


def test_full_counters_do_not_carry_between_the_halves(prog, tmp_path):
    th, words = 0x7FFF, 4 * 8190
    assert 8190 <= R.MAX_BLOCKS
    far = np.uint32(_class_halves(th)[3])
    u_far = np.full(words, far | (far << np.uint32(16)), np.uint32)
    u_on = u_far.copy()
    u_on[-2:] = np.uint32(th | (th << 16))
    u = np.concatenate([u_far, u_on])
    start = np.array([0, words, 2 * words], np.int64)
    ths = np.full(2, th, np.uint32)
    for masked in (0, 1):
        acc, o = _check(prog, tmp_path, ths, start, u, np.zeros(len(u), np.uint32), np.full(2, masked, np.int32))
        assert acc[0] == (65520 | (65520 << 16)) and o[0] == 0x00020002
        assert acc[1] == (65518 | (65518 << 16)) and o[1] == 0x00030003


def test_random_sequences_of_even_length(prog, tmp_path):
    rng = np.random.default_rng(53)
    th, start, u, inv = R.random_sequences(rng, 2000)
    assert np.all(np.diff(start) % 2 == 0)
    _check(prog, tmp_path, th, start, u, inv, np.ones(len(th), np.int32))
    _check(prog, tmp_path, th, start, u, np.zeros(len(u), np.uint32), np.zeros(len(th), np.int32))
