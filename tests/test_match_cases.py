"""Read x isoform matching on reads and genes the simulators never make (tests/_match_cases.py): the golden from the
real reference is not vacuous, and the CPU checker, the library's host path and -- where it is built -- the reference
library all equal it.  The device's match_kernel meets the same golden in tests/test_gpu_match_adversarial.py.
Integer work: every comparison is exact."""
import os

import numpy as np
import pytest

import _match_cases as mc
from _problems import flat
from miso_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match", "adversarial.npz")
GRID = [(ov, rl) for ov in mc.OVERHANGS for rl in mc.READ_LENS]


@pytest.fixture(scope="module")
def gold():
    return mc.Golden(GOLDEN)


@pytest.fixture(scope="module")
def single():
    return mc.single_reads()


def test_generator_still_makes_the_goldens_inputs(gold):
    assert mc.inputs_digest() == gold.digest


def test_wide_genes_put_tangled_on_both_sides_of_every_word_boundary():
    for K in mc.WIDE_K:
        slots = mc.tangled_slots(K)
        assert len(set(slots)) == 7 and max(slots) < K
        assert {0, 31, 32, K - 2, K - 1} <= set(slots)
        exons, isoforms = mc.wide(K)
        assert len(isoforms) == K and len({tuple(i) for i in isoforms}) == K
        assert all(exons[e][0] > 700 for k, iso in enumerate(isoforms) if k not in slots for e in iso)
    assert {63, 64} <= set(mc.tangled_slots(65)) and {63, 64, 254, 255} <= set(mc.tangled_slots(256))


@pytest.mark.parametrize("ov,rl", GRID)
def test_golden_is_not_vacuous_single_end(gold, single, ov, rl):
    m = gold.se("tangled", ov, rl)
    pos, cig, where = single
    assert m.shape == (len(pos), 7)
    hit = m.any(axis=1)
    assert 0.25 <= hit.mean() <= 0.75
    assert len({tuple(r) for r in m[hit]}) >= 10
    for k in range(7):
        assert m[:, k].any() and (hit & (m[:, k] == 0)).any()
    for name, _, cigar, row36, row30 in mc.corner_reads():
        want = mc.corner_expected(row36, row30, cigar, rl, ov)
        assert np.array_equal(m[where[name]], want), (name, m[where[name]], want)


@pytest.mark.parametrize("K", mc.WIDE_K)
def test_golden_fillers_matched_and_unmatched(gold, K):
    """some filler isoforms are matched and some are not; the bits on both sides of the word boundaries the tangled
    isoforms sit at (31 | 32 and 63 | 64) are set and cleared independently of each other"""
    m = gold.se("wide%d" % K, 1, 36)
    rest = np.setdiff1d(np.arange(K), mc.tangled_slots(K))
    cols = m[:, rest].any(axis=0)
    assert cols.any() and not cols.all()
    for b in (b for b in (32, 64) if b < K):   # a read with bit b - 1 set and b clear, and one the other way round
        assert ((m[:, b - 1] == 1) & (m[:, b] == 0)).any() and ((m[:, b - 1] == 0) & (m[:, b] == 1)).any(), b


@pytest.mark.parametrize("mean,var", mc.MEAN_VARS)
@pytest.mark.parametrize("ov,rl", GRID)
def test_golden_is_not_vacuous_paired_end(gold, ov, rl, mean, var):
    m, fl = gold.pe("tangled", ov, rl, mean, var)
    pos, cig, where = mc.paired_reads(mean, var, rl)
    assert fl.shape == (len(pos) // 2, 7) and np.array_equal(m != 0, fl >= 0)
    assert (fl >= 0).any(axis=1).sum() >= 100
    differing = sum(1 for r in fl if len(set(r[r >= 0])) > 1)
    assert differing >= (20 if (mean, var) != (60.0, 100.0) else 4)
    start, il = mc.normal_fragment(mean, var, rl)
    k = mc.window_isoform()
    assert [int(fl[where[n], k]) for n in ("window_below", "window_first", "window_last", "window_above")] \
        == [-1, start, start + il - 1, -1]
    assert fl[fl >= 0].min() == start and fl.max() == start + il - 1
    for n in ("swapped", "one_unusable", "disjoint_sets"):
        assert (fl[where[n]] == -1).all(), n
    same = rl if start == rl else -1        # fragment == read length: inside the window only where start was clamped
    assert (fl[where["same_place"]] == same).all()
    if (mean, var) == (120.0, 400.0) and rl == 36 and ov == 1:
        assert fl[where["split_lengths"]].tolist() == [77, 107, 97, 77, 177, -1, 177]


def _se_all(match, names, single, shift_of):
    pos, cig, _ = single
    for name in names:
        exons, isoforms = mc.gene(name)
        for ov, rl in GRID:
            yield name, ov, rl, match(exons, isoforms, pos + shift_of(name), cig, rl, ov)


def _shift(name):
    return mc.SHIFT if name == "shifted" else 0


def _check_lib(L, gold, single):
    """one checker library (CPU checker or reference) against the golden, every gene and every grid point"""
    def se(exons, isoforms, pos, cig, rl, ov):
        rc, m = L.match_iso(L.gene(flat(exons), isoforms), pos, cig, rl, overhang=ov)
        assert rc == 0
        return m
    for name, ov, rl, m in _se_all(se, mc.gene_names(False), single, _shift):
        assert np.array_equal(m, gold.se(name, ov, rl)), (name, ov, rl)
    for mean, var in mc.MEAN_VARS:
        for rl in mc.READ_LENS:
            pos, cig, _ = mc.paired_reads(mean, var, rl)
            for name in mc.gene_names(True):
                exons, isoforms = mc.gene(name)
                g = L.gene(flat(exons), isoforms)
                for ov in mc.OVERHANGS:
                    rc, m, fl = L.match_iso_paired(g, pos + _shift(name), cig, rl, mean, var, overhang=ov)
                    wm, wfl = gold.pe(name, ov, rl, mean, var)
                    assert rc == 0 and np.array_equal(m != 0, wm) and np.array_equal(fl, wfl), (name, ov, rl, mean, var)


def test_checker_equals_golden(orc, gold, single):
    _check_lib(orc, gold, single)


def test_reference_equals_golden(ref, gold, single):
    """also the two equalities the golden file relies on: "shifted" is "tangled", and a wide gene's tangled columns
    are "tangled" (mc.Golden rebuilds those matrices from them)"""
    _check_lib(ref, gold, single)


def test_host_library_equals_golden(gold, single):
    def se(exons, isoforms, pos, cig, rl, ov):
        return capi.Gene(exons, isoforms).match_iso(pos, cig, rl, overhang=ov)
    for name, ov, rl, m in _se_all(se, mc.gene_names(False), single, _shift):
        assert np.array_equal(m, gold.se(name, ov, rl)), (name, ov, rl)
    for mean, var in mc.MEAN_VARS:
        for rl in mc.READ_LENS:
            pos, cig, _ = mc.paired_reads(mean, var, rl)
            for name in mc.gene_names(True):
                G = capi.Gene(*mc.gene(name))
                for ov in mc.OVERHANGS:
                    m, fl = G.match_iso_paired(pos + _shift(name), cig, rl, mean, var, overhang=ov)
                    wm, wfl = gold.pe(name, ov, rl, mean, var)
                    assert np.array_equal(m != 0, wm) and np.array_equal(fl, wfl), (name, ov, rl, mean, var)


def test_model_equals_golden(gold, single):
    """the plain-Python restatement the generator plants its reads with"""
    pos, cig, _ = single
    exons, isoforms = mc.tangled()
    for ov, rl in GRID:
        assert np.array_equal(mc.model_match(exons, isoforms, pos, cig, rl, ov), gold.se("tangled", ov, rl))
    mean, var = mc.MEAN_VARS[1]
    pos, cig, _ = mc.paired_reads(mean, var, 36)
    assert np.array_equal(mc.model_match_paired(exons, isoforms, pos, cig, 36, 4, mean, var),
                          gold.pe("tangled", 4, 36, mean, var)[1])


# ---- the fragment index is a uint16_t and 0xFFFF means "none" ----
# mean 40000, numDevs 4: sd = 8191.75 gives the window 7233 .. 72767 = 65535 lengths (indices 0 .. 65534, the most
# that stay below 0xFFFF), sd = 8191.875 gives 7232 .. 72767 = 65536 lengths (index 65535 would read as "none").
# Both sd and their squares are exact in binary, so sqrt(var) gives them back exactly.
WIDEST_SD, TOO_WIDE_SD = 8191.75, 8191.875


def test_fragment_window_limit():
    assert mc.normal_fragment(40000.0, WIDEST_SD ** 2, 36) == (7233, 65535)
    assert mc.normal_fragment(40000.0, TOO_WIDE_SD ** 2, 36) == (7232, 65536)
    for device_match in (False, True):
        kw = dict(iters=100, burn=10, lag=1, chains=1, paired=True, mean=40000.0, device_match=device_match)
        b = capi.Batch(36, var=WIDEST_SD ** 2, **kw)
        assert len(b) == 0
        with pytest.raises(NotImplementedError, match="65535"):
            capi.Batch(36, var=TOO_WIDE_SD ** 2, **kw)
