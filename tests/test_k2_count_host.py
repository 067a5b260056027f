"""CPU: the read loop's per-word arithmetic and finishing expression (csrc/k2_count.hpp) compiled for the host
(tools/k2_count_host.cpp) against the numpy restatement of the definition (tests/_k2_count_ref.py): below is x < th, on the
threshold is x == th, a read picks isoform 0 iff hi 2^16 + lo < th 2^16 + tl."""
import numpy as np
import pytest

import _k2_count_ref as R


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return R.build_host(tmp_path_factory.mktemp("k2_count"))


def test_every_threshold_against_its_neighbours_and_every_half_against_the_edge_thresholds(prog, tmp_path):
    th, start, u, inv = R.edge_sequences(np.random.default_rng(41))
    thw = np.repeat(th, np.diff(start))
    # every th 0 .. 0xFFFF meets th - 2 .. th + 2, 0, 1, 0xFFFE, 0xFFFF in both halves; every x meets the edge thresholds
    assert set(np.unique(th[:65536])) == set(range(65536)) and len(u) == 65536 * 12 + len(R.EDGE_TH) * 65536
    got = R.run_host(prog, "word", [[len(u)], thw, u], tmp_path)
    want = R.word_class(thw, u)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(int(thw[i]), hex(int(u[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:5]]
    # the definition itself at the ends: nothing is below th = 0 and a half of 0 is on it; th = 0xFFFF runs as 0xFFFE
    assert R.half_class(0, 0) == 1 and R.half_class(0, 1) == 0 and R.half_class(0xFFFE, 0xFFFE) == 1
    assert R.half_class(0xFFFF, 0xFFFF) == 0 and R.half_class(0xFFFF, 0xFFFE) == 1 and R.half_class(0xFFFF, 0xFFFD) == 2
    # the sums and the flag word of the same words as sequences, and of masked random ones
    for th, start, u, inv in ((th, start, u, inv), R.random_sequences(np.random.default_rng(42), 3000)):
        n = len(th)
        out = R.run_host(prog, "seq", [[n, len(u)], start, th, u, inv], tmp_path)
        acc, o = R.seq_expected(th, start, u, inv)
        assert np.array_equal(out[:n], acc) and np.array_equal(out[n:], o)


def _lane(rng, th, tl, n_reads, n_on):
    """(hi, lo) of a lane's reads: exactly n_on high halves on th, about 1 % next to it"""
    hi = rng.integers(0, 65536, n_reads)
    hi = np.where(rng.random(n_reads) < 0.01, np.clip(th + rng.choice([-1, 1], n_reads), 0, 0xFFFF), hi)
    hi = np.where(hi == th, (th + 7) % 65536, hi)
    hi[rng.choice(n_reads, n_on, replace=False)] = th
    lo = rng.integers(0, 65536, n_reads)
    lo[rng.random(n_reads) < 0.05] = tl                      # a low half ON tl is not below it
    return hi, lo


def test_finishing_expression(prog, tmp_path):
    """d0 = (A - E) / 2 + more is the number of reads with u < t, for E = 0, 1, 2, 8 reads on the threshold, tl zero or not"""
    rng = np.random.default_rng(43)
    ths, us, starts, want, Es, mores = [], [], [0], [], [], []
    for E in (0, 1, 2, 8):
        for tl in (0, 1, 0x8000, 0xFFFF):
            for th in (0, 1, 2, 0x1234, 0x8000, 0xFFFD, 0xFFFE):     # (th = 0xFFFF: the rule of the test below)
                hi, lo = _lane(rng, th, tl, 64, E)
                ths.append(th)
                us.append((hi[0::2] | (hi[1::2] << 16)).astype(np.uint32))
                starts.append(starts[-1] + 32)
                want.append(int(np.sum((hi.astype(np.int64) << 16 | lo) < (th << 16 | tl))))
                Es.append(int(np.sum(hi == th)))
                mores.append(int(np.sum((hi == th) & (lo < tl))))
    assert sorted(set(Es)) == [0, 1, 2, 8] and any(m > 0 for m in mores) and any(m < e for m, e in zip(mores, Es))
    n, u = len(ths), np.concatenate(us)
    out = R.run_host(prog, "seq", [[n, len(u)], starts, ths, u, np.zeros(len(u), np.uint32)], tmp_path)
    A = (out[:n] & 0xFFFF) + (out[:n] >> 16)
    flagged = (out[n:] & 0x00010001) != 0
    assert np.array_equal(flagged, np.array(Es) > 0)                 # a lane enters the settle path iff it has a read on th
    assert np.array_equal(A, 2 * (np.array(want) - np.array(mores)) + np.array(Es))
    got = R.run_host(prog, "finish", [[n], A, Es, mores], tmp_path).astype(np.int32)
    assert np.array_equal(got, want), (got, want)
    # with tl == 0 nothing on the threshold is below t, and leaving E = 2 or 8 out of the expression would miscount
    tl0 = [i for i in range(n) if mores[i] == 0 and Es[i] >= 2]
    assert tl0 and all((int(A[i]) >> 1) != want[i] for i in tl0)


def test_threshold_ffff_rule(prog, tmp_path):
    """th = 0xFFFF: a lane is unflagged with A == 2 N if and only if none of its halves is 0xFFFE or 0xFFFF"""
    rng = np.random.default_rng(44)
    us, starts, clean = [], [0], []
    for case in range(400):
        hi = rng.integers(0, 0xFFFE, 32)
        kind = case % 8                                              # 0, 1: clean; then 0xFFFE, 0xFFFF, both, several
        if kind in (2, 4, 6):
            hi[rng.choice(32, 1 + (kind == 6) * 3, replace=False)] = 0xFFFE
        if kind in (3, 4, 7):
            hi[rng.choice(32, 1 + (kind == 7) * 3, replace=False)] = 0xFFFF
        if kind == 5:
            hi[:] = 0xFFFF
        us.append((hi[0::2] | (hi[1::2] << 16)).astype(np.uint32))
        starts.append(starts[-1] + 16)
        clean.append(not np.any(hi >= 0xFFFE))
    n, u = len(clean), np.concatenate(us)
    out = R.run_host(prog, "seq", [[n, len(u)], starts, np.full(n, 0xFFFF), u, np.zeros(len(u), np.uint32)], tmp_path)
    A = (out[:n] & 0xFFFF) + (out[:n] >> 16)
    flagged = np.array([bin(int(z)).count("1") for z in out[n:] & 0x00010001])
    got = R.run_host(prog, "top", [[n], A, flagged, np.full(n, 32)], tmp_path)
    assert np.array_equal(got.astype(bool), np.array(clean)) and 0 < sum(clean) < n


def test_counters_do_not_carry_within_the_capacity_bound(prog, tmp_path):
    """8191 blocks of all-below words: 8 per block and half, 65 528 -- the low counter does not reach the high one"""
    words = 4 * R.MAX_BLOCKS
    u = np.zeros(words, np.uint32)
    out = R.run_host(prog, "seq", [[1, words], [0, words], [0x8000], u, np.zeros(words, np.uint32)], tmp_path)
    assert out[0] == (8 * R.MAX_BLOCKS) * 0x00010001 and 8 * R.MAX_BLOCKS < 65536 and out[1] == 0x00020002
    # ... and one block more would
    assert 8 * (R.MAX_BLOCKS + 1) >= 65536
