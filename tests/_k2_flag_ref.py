"""numpy restatement of csrc/k2_flag.hpp from its definitions, and the cases tests/test_gpu_k2_flag.py (device) and
tests/test_k2_flag_host.py (the same functions compiled for the host) share.

A trip is flagged iff a 16-bit half of its running minimum m is zero.  A lane's trips read out as NONE (no flagged trip),
ONE at the flagged trip's position, or MANY (two or more flagged trips).  MANY is also allowed -- the caller's rescan is
always correct -- for a single flagged trip that sets two bits of (m - 0x00010001) & ~m & 0x80008000: both halves zero, or
a zero low half whose borrow runs into a high half equal to 1."""
import numpy as np

NONE, ONE, MANY = 0, 1, 2
MAX_POS = (1 << 24) - 1          # k2_flag.hpp K2_FLAG_MAX_POS - 1: the largest position the 24-bit multiply carries


def flag_expected(m, k, start):
    """(code, pos or -1 where the code is not ONE) per sequence; start: n + 1 offsets into m, k"""
    m = np.asarray(m, np.uint32)
    k = np.asarray(k, np.uint32)
    start = np.asarray(start, np.int64)
    lo, hi = m & np.uint32(0xFFFF), m >> np.uint32(16)
    zero = (lo == 0) | (hi == 0)
    two = ((lo == 0) & (hi == 0)) | ((lo == 0) & (hi == 1))
    n = len(start) - 1
    code = np.zeros(n, np.int32)
    pos = np.full(n, -1, np.int64)
    csum = np.concatenate([[0], np.cumsum(zero)])
    nflag = csum[start[1:]] - csum[start[:-1]]
    code[nflag >= 2] = MANY
    first = np.searchsorted(csum, csum[start[:-1]] + 1, side="left") - 1    # index of the sequence's first flagged trip
    one = np.nonzero(nflag == 1)[0]
    idx = first[one]
    assert zero[idx].all() and (idx >= start[one]).all() and (idx < start[one + 1]).all()
    code[one] = np.where(two[idx], MANY, ONE)
    pos[one] = np.where(two[idx], -1, k[idx].astype(np.int64))
    return code, pos


def flag_cases(rng, n_random):
    """sequences of (m, k): the named cases, then n_random random sequences of 1 .. 40 trips with about 1 % zero halves"""
    seqs = []
    clean = [0x12345678, 0x00010001, 0xFFFFFFFF, 0x80008000, 0x00020001, 0x7FFF8000]

    def seq(ms, ks):
        seqs.append((np.array(ms, np.uint64).astype(np.uint32), np.array(ks, np.uint64).astype(np.uint32)))

    seq(clean, range(0, 12, 2))                                              # no flagged trip
    seq([0x00010001], [5])
    for word in (0xFFFF0000, 0x0000FFFF, 0x12340000, 0x00001234, 0x00020000, 0x80000000, 0x00008000):   # one half only
        for at in (0, 7, MAX_POS):                                           # at k = 0 and at the largest position
            seq(clean[:3] + [word] + clean[3:], [1, 2, 3, at, 4, 6, 8])
    seq([0xFFFF0000], [0])
    seq([0x0000FFFF], [MAX_POS])
    seq([0], [9])                                                            # both halves of one word
    seq(clean + [0], list(range(6)) + [MAX_POS])
    seq([0x00010000], [3])                                                   # a low half under a high half of 1
    seq([0x00000001], [3])                                                   # a high half over a low half of 1: one bit
    seq([0xFFFF0000, 0x12345678, 0x0000FFFF], [2, 4, 6])                     # two different trips
    seq([0xFFFF0000, 0xFFFF0000], [MAX_POS, MAX_POS])
    seq([0x0000FFFF, 0], [0, 0])
    for count in (300, 70000):                                               # no accumulator may wrap to "none"
        seq([0xABCD0000] * count, np.arange(count) * 2)
        seq([0] * count, np.full(count, MAX_POS))
        seq([0x00010000] * count, np.arange(count) % 65536 * 256)
    seq([0] * 65536, [MAX_POS] * 65536)                                      # 2 x 65536 bits: a 16-bit count would wrap here
    for _ in range(n_random):
        ln = int(rng.integers(1, 41))
        m = rng.integers(0, 1 << 32, ln, dtype=np.uint64)
        z = rng.random((ln, 2)) < 0.01
        m = np.where(z[:, 0], m & 0xFFFF0000, m)
        m = np.where(z[:, 1], m & 0x0000FFFF, m)
        near = rng.random(ln) < 0.02                                         # halves of 1 next to the zeros
        m = np.where(near, (m & 0x0000FFFF) | 0x00010000, m)
        k = rng.integers(0, MAX_POS + 1, ln, dtype=np.uint64)
        seq(m, k)
    start = np.concatenate([[0], np.cumsum([len(s[0]) for s in seqs])]).astype(np.int32)
    return np.concatenate([s[0] for s in seqs]), np.concatenate([s[1] for s in seqs]), start


def part_inv_expected(rem, w):
    """halves 2 w and 2 w + 1 of the partial block are not reads iff their number is >= rem"""
    rem, w = np.asarray(rem, np.int64), np.asarray(w, np.int64)
    lo = np.where(2 * w >= rem, 0xFFFF, 0)
    hi = np.where(2 * w + 1 >= rem, 0xFFFF0000, 0)
    return (lo | hi).astype(np.uint32)
