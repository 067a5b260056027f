"""GPU: what a lane of the single-end two-isoform read loop does BEHIND the loop (miso_amd/csrc/kernels_k2.inl k2_finish_lane:
the settle path, d0 = (A - E) / 2 + more, the th = 0xFFFF rule and recount, the t = 2^32 closed form) with thresholds the
test chooses -- among them the ones a sampled chain meets once in 10^8 steps: tl == 0 with TWO AND MORE reads of one lane on
the threshold, which the old `tl != 0 &&` guard in front of the settle path would get wrong by E / 2.

`miso_selftest_k2_finish` runs one single-lane chain per element: the sum and flag from csrc/k2_count.hpp's functions over
the chain's generator blocks, then the kernel's own k2_finish_lane.  The expected count is the definition: the number of the
chain's reads whose 32-bit uniform (high half-word from site 2, low from site 4, include/miso_philox.h) is below t; the
uniforms come from the checker's generator."""
import numpy as np
import pytest

from miso_amd import capi

pytestmark = pytest.mark.gpu

SEED, EVENT, CHAIN = 93, 4100, 1
SIZES = (2003, 1501, 24, 16, 7, 1, 0)       # two blocks = one trip; three = a trip and a single step; partial blocks; none
SCAN = 8192 + 3                             # lanes searched for a half of 0xFFFF or 0xFFFE (one iteration in nine holds one)


def _uniforms(orc, iteration, n_draw):
    """the 32-bit uniforms of the chain's drawing reads at this iteration (half h of block r / 8 = bits 16 (h & 1) .. of word
    h / 2)"""
    out = []
    for site in (2, 4):
        halves = []
        for q in range((n_draw + 7) >> 3):
            w = orc.philox((q, iteration, site | (CHAIN << 8), EVENT), (SEED & 0xFFFFFFFF, SEED >> 32)).astype(np.uint64)
            halves.append(np.stack([w & 0xFFFF, w >> 16], axis=1).ravel())
        out.append(np.concatenate(halves)[:n_draw] if halves else np.zeros(0, np.uint64))
    return (out[0] << np.uint64(16)) | out[1]


@pytest.fixture(scope="module")
def cases(orc):
    """[(iteration, n_draw, t, expected, label)]"""
    assert int(_uniforms(orc, 5, 9)[8]) == orc.split_word(SEED, EVENT, CHAIN, 5, 8)      # the address restated here is the checker's
    rng = np.random.default_rng(61)
    out = []
    top_seen = set()
    for it, n in [(i, SIZES[i % len(SIZES)]) for i in range(14)] + [(100 + i, SCAN) for i in range(120)]:
        if it >= 100 and all(sum(1 for s in top_seen if s[0] == v) >= 3 for v in (0xFFFF, 0xFFFE)):
            break
        u = _uniforms(orc, it, n)
        hi, lo = (u >> np.uint64(16)).astype(np.int64), (u & np.uint64(0xFFFF)).astype(np.int64)
        ts = []
        if it < 14:
            ts += [(0, "th=0"), (1, "th=0"), (0xFFFF, "th=0"), (0xFFFE0000, "th=0xFFFE"), (0xFFFEFFFF, "th=0xFFFE"),
                   (0xFFFF0000, "th=0xFFFF"), (0xFFFF8000, "th=0xFFFF"), (0xFFFFFFFF, "th=0xFFFF"), (1 << 32, "closed")]
            ts += [(int(x), "random") for x in rng.integers(0, 1 << 32, 6, dtype=np.uint64)]
            vals, cnt = np.unique(hi, return_counts=True)
            for v in vals[cnt >= 2][:6]:                    # two and more reads of the lane ON the threshold
                los = np.sort(lo[hi == v])
                ts += [(int(v) << 16, "tl=0,E>=2"), ((int(v) << 16) | int(los[0]), "E>=2"), ((int(v) << 16) | (int(los[0]) + 1), "E>=2"),
                       ((int(v) << 16) | int(los[-1]), "E>=2"), ((int(v) << 16) | 0xFFFF, "E>=2")]
            for v in vals[cnt == 1][:4]:                    # one
                l1 = int(lo[hi == v][0])
                ts += [(int(v) << 16, "tl=0,E=1"), ((int(v) << 16) | l1, "E=1"), ((int(v) << 16) | min(l1 + 1, 0xFFFF), "E=1")]
        else:                                               # lanes that hold a half of 0xFFFF or of 0xFFFE, at th = 0xFFFF
            for v in (0xFFFF, 0xFFFE):
                if np.any(hi == v) and sum(1 for s in top_seen if s[0] == v) < 3:
                    top_seen.add((v, it))
                    l1 = int(lo[hi == v][0])
                    ts += [(0xFFFF0000, "0x%X at th=0xFFFF" % v), (0xFFFF0000 | l1, "0x%X at th=0xFFFF" % v),
                           (0xFFFF0000 | min(l1 + 1, 0xFFFF), "0x%X at th=0xFFFF" % v), (1 << 32, "closed")]
        for t, label in ts:
            out.append((it, n, t, int(np.sum(u < np.uint64(t))) if t < (1 << 32) else n, label))
    return out


@pytest.mark.parametrize("settle_all", [False, True])
def test_finish_equals_the_definition(cases, settle_all):
    labels = [c[4] for c in cases]
    for want, least in (("tl=0,E>=2", 10), ("E>=2", 10), ("tl=0,E=1", 10), ("0xFFFF at th=0xFFFF", 3), ("0xFFFE at th=0xFFFF", 3),
                        ("th=0", 10), ("th=0xFFFE", 10), ("th=0xFFFF", 10), ("closed", 10)):
        assert labels.count(want) >= least, (want, labels.count(want))
    it, n, t, want, _ = (np.array(x) for x in zip(*[c[:4] + (0,) for c in cases]))
    got = capi.selftest_k2_finish(SEED, np.full(len(cases), EVENT), np.full(len(cases), CHAIN), it, n, t.astype(np.uint64), settle_all)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(cases[i], int(got[i])) for i in bad[:8]]
    # the cases do tell the old guard apart: leaving E out at tl == 0 moves the count by E / 2 >= 1
    assert any(c[4] == "tl=0,E>=2" and c[1] >= 1500 for c in cases)
