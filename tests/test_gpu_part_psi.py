"""GPU: the isoform-group passes (miso_batch_summarize_isoform_groups, miso_batch_compare_pairs_isoform_groups;
miso_amd/csrc/kernels_groups.hip) against their restatement (tests/_part_psi_ref.py): every double by its bits,
every count as an integer.  Columns are placed with SamplesBatch (miso_batch_from_samples).

Shapes: K in {2, 3, 20, 64} (one member, an odd count, several words of a row, the mask's full width) and S in {60, 257,
8192} (the smallest S the strict ranks accept and fewer rows than threads; one more than the workgroup; the limit).  Masks: a
single bit, all bits, bit 63 alone, alternating bits.  Values: unrounded draws (what as_text changes), ties on a dyadic grid
with -0.0 among the zeros, a NaN and an infinity in member columns, a NaN in a column outside the mask."""
import ctypes as C
import math

import numpy as np
import pytest

import _pairs_ref as PR
import _part_psi_ref as GR
from miso_amd import capi

pytestmark = pytest.mark.gpu

TAUS4 = (0.05, 0.2, 0.25, 0.5)


def masks_of(K):
    """single bits (the first, the second, the last: bit 63 at K = 64), all bits, the two alternating patterns"""
    full = (1 << K) - 1
    ms = [1, 1 << (K - 1), full, 0x5555555555555555 & full, 0xAAAAAAAAAAAAAAAA & full]
    if K >= 3:
        ms.append(2)
    return sorted(set(ms))


def planted(K, S, seed):
    """three events [S, K] and what a `.miso` file would hand on of them: unrounded draws; a dyadic grid with ties and -0.0;
    the first again with a NaN in column 0 and an infinity in the last column"""
    rng = np.random.default_rng([seed, K, S])
    e0 = rng.dirichlet(np.ones(K), S)
    e0[1] = e0[0]                                       # a tied row
    e1 = rng.integers(0, 5, (S, K)) / 16.0
    e1[(e1 == 0) & (rng.random((S, K)) < 0.5)] = -0.0
    e2 = e0.copy()
    e2[S // 2, 0] = np.nan
    e2[3, K - 1] = np.inf
    r0 = GR.as_read(e0)
    r2 = r0.copy()
    r2[S // 2, 0] = np.nan
    r2[3, K - 1] = np.inf
    return [e0, e1, e2], [r0, e1, r2]                   # (the grid prints exactly; "-0.0000" adds like 0.0)


def finite_expected(K, e, mask):
    return e != 2 or not (mask & 1 or mask >> (K - 1) & 1)


@pytest.mark.parametrize("S", [60, 257, 8192])
@pytest.mark.parametrize("K", [2, 3, 20, 64])
def test_summary_bit_for_bit(K, S):
    evs, read = planted(K, S, 1)
    b = capi.SamplesBatch(evs)
    groups = [(e, m) for e in range(3) for m in masks_of(K)]
    for as_text in (False, True):
        got = b.summarize_isoform_groups(groups, 0.95, as_text=as_text)
        assert len(got) == len(groups) and got.kernel_ms > 0
        for g, (e, m) in enumerate(groups):
            want = GR.summarize((read if as_text else evs)[e], m, 0.95)
            assert GR.same3(got.summary(g), want), (as_text, e, hex(m), got.summary(g), want)
            assert math.isnan(want[0]) == (not finite_expected(K, e, m)), (e, hex(m))
    assert "summarize_groups" in b.last_kernels().split(",")
    if K >= 3:      # the NaN in column 0 is outside the mask {1}: the group is finite, its numbers those of the clean event
        clean = b.summarize_isoform_groups([(0, 2), (2, 2)], 0.95)
        assert GR.same3(clean.summary(0), clean.summary(1)) and not math.isnan(clean.mean[1])


def test_summary_levels_and_the_sign_of_zero():
    """other ranks; a column of -0.0 and 0.0 only comes back as +0.0 in all three numbers"""
    S = 257
    rng = np.random.default_rng(3)
    x = rng.dirichlet(np.ones(5), S)
    z = np.where(rng.random((S, 3)) < 0.5, -0.0, 0.0)
    b = capi.SamplesBatch([x, z])
    for level in (0.5, 0.9, 0.98):
        got = b.summarize_isoform_groups([(0, 0b10110), (1, 0b101), (1, 0b010)], level)
        assert GR.same3(got.summary(0), GR.summarize(x, 0b10110, level))
        for g in (1, 2):
            assert PR.bits(got.summary(g)).tolist() == [0, 0, 0]


@pytest.mark.parametrize("n_tau", [0, 4])
@pytest.mark.parametrize("K", [2, 3, 20, 64])
def test_comparison_bit_for_bit(K, n_tau):
    S1, S2 = 60, 97
    taus = TAUS4[:n_tau]
    ev1, read1 = planted(K, S1, 11)
    ev2, read2 = planted(K, S2, 12)
    ev2[2], read2[2] = ev2[0].copy(), read2[0].copy()    # event 2: not finite in sample 1 only
    b1, b2 = capi.SamplesBatch(ev1), capi.SamplesBatch(ev2)
    groups = [(e, m) for e in range(3) for m in masks_of(K)]
    for as_text in (False, True):
        got = capi.compare_pairs_isoform_groups(b1, b2, groups, 0.95, taus, as_text=as_text)
        assert len(got) == len(groups) and got.n_pairs == S1 * S2 and got.n_tau == n_tau
        for g, (e, m) in enumerate(groups):
            want = GR.compare((read1 if as_text else ev1)[e], (read2 if as_text else ev2)[e], m, 0.95, taus)
            assert PR.same(got.pair_comparison(g), want), (as_text, e, hex(m), got.pair_comparison(g), want)
            assert want[6] == finite_expected(K, e, m)
        # the samples swapped
        back = capi.compare_pairs_isoform_groups(b2, b1, groups, 0.95, taus, as_text=as_text)
        for g, (e, m) in enumerate(groups):
            want = GR.compare((read2 if as_text else ev2)[e], (read1 if as_text else ev1)[e], m, 0.95, taus)
            assert PR.same(back.pair_comparison(g), want), ("swapped", as_text, e, hex(m))
    assert "compare_pairs_groups_iso" in b1.last_kernels().split(",")
    # the pairwise pass after the group pass is still named
    b1.compare_pairs(b2, 0.95, taus)
    assert b1.last_kernels().split(",")[-1] == "compare_pairs"


def test_comparison_at_larger_columns():
    """more draws than threads on both sides, a chunk of several draws per thread: M = 1000 x 450"""
    rng = np.random.default_rng(17)
    ev1 = [np.round(rng.dirichlet(np.ones(4), 1000), 4)]
    ev2 = [np.round(rng.dirichlet(np.ones(4), 450), 4)]
    b1, b2 = capi.SamplesBatch(ev1), capi.SamplesBatch(ev2)
    groups = [(0, 0b0110), (0, 0b1111), (0, 0b1001)]
    got = capi.compare_pairs_isoform_groups(b1, b2, groups, 0.9, (0.1, 0.2))
    for g, (_, m) in enumerate(groups):
        assert PR.same(got.pair_comparison(g), GR.compare(ev1[0], ev2[0], m, 0.9, (0.1, 0.2))), hex(m)


@pytest.mark.parametrize("S", [60, 257, 8192])
def test_a_single_bit_is_the_isoform_itself(S):
    """a group of one isoform against summarize / summarize_as_text and compare_pairs / compare_pairs_as_text of that isoform
    (columns without -0.0, which the group's 0.0 + x turns into 0.0 and the summary hands on as it is).

    Bit for bit: everything of the plain summary, both bounds of the text summary, everything of both comparisons.  The text
    summary's MEAN is not the same number by definition: miso_batch_summarize_as_text divides the exact integer sum of the
    printed digits by S * 10^4 (one rounding), the group pass folds the doubles k / 10^4 as its contract states.
    Both approximate the same exact mean of non-negative terms; the fold rounds each term once (k / 10^4), every term passes
    through at most ceil(S / 256) + 8 additions, then one division, the digit sum rounds once: the two differ by at most
    (ceil(S / 256) + 8 + 1 + 1 + 1) * 2^-53 relative to the mean, to first order; asserted with that bound and one unit of
    slack for the second-order terms.  The group mean itself is asserted bit for bit against the restatement above."""
    rng = np.random.default_rng([5, S])
    K = 3
    x1 = rng.dirichlet(np.ones(K), S)
    x2 = np.round(rng.dirichlet(np.ones(K), S), 2)       # ties
    y1, y2 = rng.dirichlet(np.ones(K), 97), np.round(rng.dirichlet(np.ones(K), 97), 2)
    b, c = capi.SamplesBatch([x1, x2]), capi.SamplesBatch([y1, y2])
    groups = [(e, 1 << k) for e in range(2) for k in range(K)]
    for as_text in (False, True):
        b.summarize(0.95, as_text=as_text)
        got = b.summarize_isoform_groups(groups, 0.95, as_text=as_text)
        for g, (e, m) in enumerate(groups):
            k = m.bit_length() - 1
            mean, lo, hi = (v[k] for v in b.summary(e))
            gm, glo, ghi = got.summary(g)
            assert PR.bits([glo, ghi]).tolist() == PR.bits([lo, hi]).tolist(), (as_text, e, k)
            if not as_text:
                assert PR.bits(gm) == PR.bits(mean), (e, k, gm, mean)
            else:
                bound = (math.ceil(S / 256) + 12) * 2.0 ** -53 * abs(mean)
                print("text mean, S=%d event %d isoform %d: group %r summary %r bound %.3g" % (S, e, k, gm, mean, bound))
                assert abs(gm - mean) <= bound, (e, k, gm, mean, bound)
    if S == 8192:
        return                                           # (the pairwise pass at the limit has its own test)
    for as_text in (False, True):
        b.compare_pairs(c, 0.95, TAUS4, as_text=as_text)
        got = capi.compare_pairs_isoform_groups(b, c, groups, 0.95, TAUS4, as_text=as_text)
        for g, (e, m) in enumerate(groups):
            k = m.bit_length() - 1
            med, lo, hi, gt, lt, ge, fin, M = b.pair_comparison(e)
            want = (med[k], lo[k], hi[k], int(gt[k]), int(lt[k]), [int(v) for v in ge[k]], bool(fin[k]), M)
            assert PR.same(got.pair_comparison(g), want), (as_text, e, k)


def test_the_limit_both_columns_in_lds():
    """S1 = S2 = 8192: 128 KB of columns; two masks against the restatement that forms no difference (_pairs_ref.bisect)"""
    S = 8192
    rng = np.random.default_rng(23)
    x1, x2 = np.round(rng.dirichlet(np.ones(3), S), 4), np.round(rng.dirichlet(np.ones(3), S), 4)
    b1, b2 = capi.SamplesBatch([x1]), capi.SamplesBatch([x2])
    got = capi.compare_pairs_isoform_groups(b1, b2, [(0, 0b011), (0, 0b100)], 0.95, (0.1, 0.2))
    for g, m in enumerate((0b011, 0b100)):
        want = PR.bisect(GR.group_column(x1, m), GR.group_column(x2, m), 0.95, (0.1, 0.2))
        assert PR.same(got.pair_comparison(g), want), hex(m)


def test_undecoded_events_are_not_finite():
    """columns decoded from `.miso` text; an event outside the fast grammar, in either sample: as miso_batch_compare_pairs"""
    rng = np.random.default_rng(9)
    S1, S2, Ks = 120, 75, [2, 4, 3]

    def sample(S, spoil):
        evs = [np.round(rng.dirichlet(np.ones(K), S), 4) for K in Ks]
        bodies = []
        for e, x in enumerate(evs):
            rows = [",".join("%.4f" % v for v in r) + "\t-12.5\n" for r in x]
            if e == spoil:
                rows[3] = rows[3].replace("\t", "e0\t")       # an exponent
            bodies.append("".join(rows).encode())
        offs = np.concatenate([[0], np.cumsum([len(t) for t in bodies])]).astype(np.int64)
        return evs, capi.SamplesBatch.from_text(b"".join(bodies), offs, Ks, S)
    ev1, b1 = sample(S1, 1)
    ev2, b2 = sample(S2, 2)
    assert [int(s != 0) for s in b1.status] == [0, 1, 0] and [int(s != 0) for s in b2.status] == [0, 0, 1]
    groups = [(0, 0b11), (1, 0b0110), (2, 0b101)]
    got = capi.compare_pairs_isoform_groups(b1, b2, groups, 0.95, (0.2,))
    assert PR.same(got.pair_comparison(0), GR.compare(ev1[0], ev2[0], 0b11, 0.95, (0.2,)))
    for g in (1, 2):
        med, lo, hi, gt, lt, ge, fin, M = got.pair_comparison(g)
        assert not fin and math.isnan(med) and math.isnan(lo) and math.isnan(hi) and (gt, lt, ge, M) == (0, 0, [0], S1 * S2)
    s1 = b1.summarize_isoform_groups(groups, 0.95)
    assert GR.same3(s1.summary(0), GR.summarize(ev1[0], 0b11)) and GR.same3(s1.summary(2), GR.summarize(ev1[2], 0b101))
    assert all(math.isnan(v) for v in s1.summary(1))


# ---- refusals: MISO_EINVAL before any launch, earlier results untouched
def _raw_summarize(b, ev, mask, level=0.95, out_len=None):
    L = capi.lib()
    ev, mask = np.asarray(ev, np.int32), np.asarray(mask, np.uint64)
    out = np.full(3 * max(len(ev), 1), 7.0)
    L.miso_batch_summarize_isoform_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int,
                                                      C.c_void_p, C.c_int64, C.POINTER(C.c_float)]
    rc = L.miso_batch_summarize_isoform_groups(b.handle, capi._p(ev), capi._p(mask), len(ev), level, 0, capi._p(out),
                                               3 * len(ev) if out_len is None else out_len, None)
    return rc, L.miso_last_error().decode(), out


def _raw_compare(b1, b2, ev, mask, level=0.95, taus=(0.2,), out_len=None):
    L = capi.lib()
    ev, mask, tt = np.asarray(ev, np.int32), np.asarray(mask, np.uint64), np.asarray(taus, np.float64)
    W = 6 + len(tt)
    out = np.full(W * max(len(ev), 1), 7, np.uint64)
    L.miso_batch_compare_pairs_isoform_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double,
                                                          C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                                          C.POINTER(C.c_int64), C.POINTER(C.c_float)]
    rc = L.miso_batch_compare_pairs_isoform_groups(b1.handle, b2.handle, capi._p(ev), capi._p(mask), len(ev), level, capi._p(tt),
                                                   len(tt), 0, capi._p(out), W * len(ev) if out_len is None else out_len, None,
                                                   None)
    return rc, L.miso_last_error().decode(), out


def test_refusals_launch_nothing_and_leave_earlier_results():
    rng = np.random.default_rng(2)
    Ks = [2, 3, 65, 64]
    ev1 = [rng.dirichlet(np.ones(K), 80) for K in Ks]
    ev2 = [rng.dirichlet(np.ones(K), 61) for K in Ks]
    b1, b2 = capi.SamplesBatch(ev1), capi.SamplesBatch(ev2)
    b1.summarize(0.95)
    b1.compare_pairs(b2, 0.95, (0.2,))
    names = b1.last_kernels()

    def stored():
        return [np.concatenate([PR.bits(np.concatenate(b1.summary(i))),
                                PR.bits(np.concatenate([np.asarray(v, np.float64).ravel() for v in b1.pair_comparison(i)[:6]]))])
                for i in range(len(Ks))]
    before = stored()
    cases = [([0], [0], "group 0: empty"), ([0, 1], [1, 0b1000], "group 1: the mask names"), ([0], [0b100], "group 0: the mask names"),
             ([1, 2], [1, 1], "group 1: event 2 has 65 isoforms"), ([4], [1], "group 0: event index"), ([-1], [1], "group 0: event index")]
    for ev, mask, msg in cases:
        for rc, err, out in (_raw_summarize(b1, ev, mask), _raw_compare(b1, b2, ev, mask)):
            assert rc == capi.MISO_EINVAL and msg in err, (ev, mask, rc, err)
            assert (out == 7).all()
    for rc, err, out in (_raw_summarize(b1, [0, 1], [1, 1], out_len=5), _raw_compare(b1, b2, [0, 1], [1, 1], out_len=13)):
        assert rc == capi.MISO_EINVAL and "out is too short" in err and (out == 7).all()
    big = capi.SamplesBatch([np.full((8193, 2), 0.5)])
    rc, err, _ = _raw_summarize(big, [0], [1])
    assert rc == capi.MISO_EINVAL and "Too many samples" in err
    one = capi.SamplesBatch([rng.random((80, 2))])
    for x, y in ((big, one), (one, big)):
        rc, err, _ = _raw_compare(x, y, [0], [1])
        assert rc == capi.MISO_EINVAL and PR.refusal(8193, 80, 0.95, (0.2,)) in err
    few = capi.SamplesBatch([rng.random((59, 2))])
    rc, err, _ = _raw_summarize(few, [0], [1])
    assert rc == capi.MISO_EINVAL and "Too few samples for a credible interval" in err
    with pytest.raises(capi.InternalError, match="Too few samples"):
        few.summarize(0.95)                               # (the summary's own refusal)
    rc, err, _ = _raw_compare(b1, b2, [0], [1], taus=(0.2, 1.5))
    assert rc == capi.MISO_EINVAL and "Invalid delta psi threshold" in err
    rc, err, _ = _raw_compare(b1, one, [0], [1])
    assert rc == capi.MISO_EINVAL and "differ in events" in err
    with pytest.raises(capi.InternalError, match="empty isoform mask"):
        b1.summarize_isoform_groups([(0, 0)])
    with pytest.raises(capi.InternalError, match="empty isoform mask"):
        capi.compare_pairs_isoform_groups(b1, b2, [(0, 0)])
    # nothing ran, nothing moved
    assert b1.last_kernels() == names and "groups" not in names
    for x, y in zip(before, stored()):
        assert x.tolist() == y.tolist()
    # no groups: valid, nothing launched
    assert _raw_summarize(b1, [], [])[0] == 0 and _raw_compare(b1, b2, [], [])[0] == 0
    assert len(b1.summarize_isoform_groups([])) == 0 and len(capi.compare_pairs_isoform_groups(b1, b2, [])) == 0
    assert b1.last_kernels() == names
    # ... and after all that the calls still work, bit 63 of the 64-isoform event included, and store nothing
    got = b1.summarize_isoform_groups([(3, 1 << 63), (1, 0b110)], 0.95)
    assert GR.same3(got.summary(0), GR.summarize(ev1[3], 1 << 63)) and GR.same3(got.summary(1), GR.summarize(ev1[1], 0b110))
    cmp_ = capi.compare_pairs_isoform_groups(b1, b2, [(3, 1 << 63)], 0.95, (0.2,))
    assert PR.same(cmp_.pair_comparison(0), GR.compare(ev1[3], ev2[3], 1 << 63, 0.95, (0.2,)))
    for x, y in zip(before, stored()):
        assert x.tolist() == y.tolist()


def test_sampler_batches_not_yet_synced():
    """resident samples of two launched runs (other seeds, other lengths), neither synced: the passes wait for both"""
    from miso_amd import workload
    n, K = 6, 3
    b1 = workload.build_batch(100, n, K=K, n_reads=60, iters=200, burn=50, lag=1, chains=2, paired=True)
    b2 = workload.build_batch(100, n, K=K, n_reads=60, iters=170, burn=50, lag=1, chains=2, paired=True)
    for s, b in enumerate((b1, b2)):
        b.upload(0)
        b.launch(seed=5 + s, first_event_id=0)
    groups = [(i, 0b011) for i in range(n)] + [(i, 0b110) for i in range(n)]
    cmp_ = capi.compare_pairs_isoform_groups(b1, b2, groups, 0.95, (0.1, 0.2), as_text=True)
    summ = b1.summarize_isoform_groups(groups, 0.95, as_text=True)
    for b in (b1, b2):
        b.sync()
        b.download()
    for g, (i, m) in enumerate(groups):
        s1, s2 = GR.as_read(b1.result(i).samples), GR.as_read(b2.result(i).samples)
        assert s1.shape == (300, K) and s2.shape == (240, K)
        assert PR.same(cmp_.pair_comparison(g), GR.compare(s1, s2, m, 0.95, (0.1, 0.2))), (i, hex(m))
        assert GR.same3(summ.summary(g), GR.summarize(s1, m, 0.95)), (i, hex(m))
