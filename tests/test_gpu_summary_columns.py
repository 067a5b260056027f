"""GPU: summarize_kernel on columns chosen to break a radix select or a rounding rule, through capi.SamplesBatch(arrays)
(miso_batch_from_samples, the entry samples_utils uses for every host-parsed file) and, where a column can be written in
four decimals, through SamplesBatch.from_text as well.  Bit-exact against a plain reference on the same doubles:

  plain    bounds = np.sort(col)[rank] (credible_intervals.py:31-55), mean = _summary_ref.tree_mean(col)
  as_text  bounds = credible_interval over float("%.4f" % v); mean = the exact integer sum of the printed digits over
           S x 10^4; when the column holds a value that is printed and read back unchanged and has no four digits to sum
           (nan, +-inf, |v| >= 2^38), tree_mean of the values as read

Zeros compare by value: np.sort does not order -0.0 against 0.0.  NaN: np.sort (and the reference's `samples.sort()`,
credible_intervals.py:53) puts every NaN behind +inf whatever its sign bit, and float("%.4f" % nan) is a plain nan; the
device is pinned to that: a bound whose rank lies among the NaNs is NaN, and a sign-bit NaN does not move in front of
-inf (kernels_summary.hip order_key maps every NaN to the largest key).

What the sampler's own output never reaches, and these columns do: the negative half of order_key, ties (the early exit,
the per-thread and per-wavefront merging of histogram adds), keys that differ in their first byte or only in their last,
the 256-thread stride (S = 255, 256, 257, 511), the register cache's limit (8191, 8192, 8193), the smallest admitted S,
blocks with blockIdx.y >= K beside working ones."""
import numpy as np
import pytest

from _summary_ref import credible_interval, tree_mean
from miso_amd import capi, summary

pytestmark = pytest.mark.gpu

LEVELS = (0.95, 0.9, 0.5, 0.0)
TEXT_EXACT_BELOW = 2.0 ** 38        # kernels_summary.hip: |v| below this is rounded as "%.4f" does, the rest stays as it is


def smallest_admitted(level=0.95):
    S = 2
    while summary.credible_interval_ranks(S, level)[0] <= 0:
        S += 1
    return S


S_MIN = smallest_admitted()
SAMPLE_COUNTS = (S_MIN, 255, 256, 257, 511, 8191, 8192, 8193, 20000)


def test_smallest_admitted_is_sixty():
    assert S_MIN == 60 and summary.credible_interval_ranks(59, 0.95)[0] == 0


# ---- orders ----
def thread_major(S):
    """positions ordered by (s % 256, s // 256): a sorted column written along it hands thread t of summarize_column
    (samples t, t + 256, ...) consecutive sorted values -- with ties, runs of one bin: a sawtooth of period 256"""
    return np.argsort(np.arange(S) % 256, kind="stable")


def orders(sorted_col, rng):
    S = len(sorted_col)
    saw = np.empty(S)
    saw[thread_major(S)] = sorted_col
    return np.stack([sorted_col, sorted_col[::-1], sorted_col[rng.permutation(S)], saw], axis=1)      # [S, 4]


# ---- columns ----
def _from_bits(b):
    return np.asarray(b, dtype=np.uint64).view(np.float64)


def column_families(S, rng):
    """name -> S values (any order)"""
    fam = {}
    fam["constant"] = np.full(S, 0.3137)
    fam["two valued"] = np.where(rng.random(S) < 0.3, 0.25, 0.7501)
    fam["grid ties"] = rng.integers(0, 40, S) / 1e4 + 0.42
    base = np.array([0.61803398875]).view(np.uint64)[0] & ~np.uint64(0xFFFF)
    fam["low bytes only"] = _from_bits(base + np.arange(S, dtype=np.uint64))           # distinct; S <= 256: seven bytes shared
    fam["last byte only"] = _from_bits(base + (np.arange(S, dtype=np.uint64) % np.uint64(256)))
    z = rng.normal(0.0, 0.01, S)
    z[rng.random(S) < 0.15] = 0.0
    z[rng.random(S) < 0.15] = -0.0
    z[rng.random(S) < 0.1] = 5e-324
    z[rng.random(S) < 0.1] = -5e-324
    fam["signs around zero"] = z
    # subnormal to 1e300, either sign (as_text: not in [2^38, 2^52), where "%.4f" rounds and the device does not)
    ex = np.where(rng.random(S) < 0.7, rng.uniform(-322, 5, S), rng.uniform(16, 300, S))
    fam["magnitudes"] = np.where(rng.random(S) < 0.4, -1.0, 1.0) * 10.0 ** ex
    v = rng.random(S)
    v[:2] = -np.inf
    v[2:5] = np.inf
    fam["inf at the ends"] = v
    v = rng.random(S) * 2 - 1
    v[:3] = np.inf
    fam["inf at the top"] = v
    v = rng.random(S) * 2 - 1
    v[0] = np.nan
    v[1] = -np.nan
    v[2] = _from_bits([0xFFF0000000000001])[0]           # a signalling-pattern NaN with the sign bit
    v[3] = -np.inf
    fam["a few nan"] = v
    # enough NaN that the upper 0.95 rank lies among them, half of them with the sign bit
    n_nan = S - summary.credible_interval_ranks(S, 0.95)[1] + 1
    v = rng.random(S) - 0.5
    v[:n_nan] = np.nan
    v[:n_nan:2] = -np.nan
    fam["nan up to the rank"] = v
    # tie runs placed by the ranks of each level: distinct values everywhere else, so a rank one off gives another value
    for level in LEVELS:
        lo, hi = summary.credible_interval_ranks(S, level)
        asc = (np.arange(S) - S // 3) / 1024.0 + rng.random(S) / 4096.0            # strictly increasing, both signs
        assert np.all(np.diff(asc) > 0)
        w = min(5, lo, S - 1 - hi)
        if w < 1:
            continue
        for name, runs in (("run starts at the ranks", [(lo, lo + w), (hi, hi + w)]),
                           ("run ends at the ranks", [(lo - w, lo), (hi - w, hi)]),
                           ("both ranks in one run", [(lo - w, hi + w)])):
            if name != "both ranks in one run" and hi - lo <= w:
                continue
            c = asc.copy()
            for a, b in runs:
                c[a:b + 1] = asc[a]
            fam["%s, level %g" % (name, level)] = c
    return fam


def as_read(col):
    """what float() makes of "%.4f" % v"""
    return np.array([float("%.4f" % v) for v in col.tolist()])


def text_mean(col, read):
    plain = np.isfinite(col) & (np.abs(col) < TEXT_EXACT_BELOW)
    if not plain.all():
        return tree_mean(read)
    digits = sum(int(("%.4f" % v).replace(".", "")) for v in col.tolist())
    return digits / (len(col) * 10000.0)


def same(a, b):
    """equal doubles: by value (so -0.0 is 0.0; for every other pair that is bit for bit), NaN equal to NaN"""
    a, b = float(a), float(b)
    return a == b or (a != a and b != b)


@pytest.mark.parametrize("as_text", [False, True], ids=["plain", "as_text"])
@pytest.mark.parametrize("S", SAMPLE_COUNTS)
def test_adversarial_columns_at_every_order_and_level(S, as_text):
    rng = np.random.default_rng(1000 + S)
    fam = column_families(S, rng)
    names = list(fam)
    events = []
    for n in names:
        col = fam[n]
        nan = np.isnan(col)
        srt = np.concatenate([np.sort(col[~nan]), col[nan]])             # ascending, the NaNs (of either sign) last
        events.append(orders(srt, rng))
    b = capi.SamplesBatch(events)
    # NaN placement of the reference, written down: np.sort puts NaN last whatever its sign bit
    assert np.isnan(np.sort(np.array([-np.nan, 1.0, np.inf, -np.inf]))[-1])
    refs = []
    with np.errstate(invalid="ignore", over="ignore"):           # (inf - inf, NaN and 1e300 + 1e300 are among the columns)
        for ev in events:
            per_col = []
            for k in range(ev.shape[1]):
                col = ev[:, k]
                vals = as_read(col) if as_text else col
                per_col.append((text_mean(col, vals) if as_text else tree_mean(col), vals))
            refs.append(per_col)
    bad = []
    for level in LEVELS:
        lo_rank, hi_rank = summary.credible_interval_ranks(S, level)
        assert 0 < lo_rank <= hi_rank < S and (level != 0.0 or lo_rank == hi_rank)
        b.summarize(level, as_text=as_text)
        for i, n in enumerate(names):
            m, lo, hi = b.summary(i)
            for k in range(4):
                mean, vals = refs[i][k]
                elo, ehi = credible_interval(vals, level)                 # np.sort(vals)[rank]
                if not (same(m[k], mean) and same(lo[k], elo) and same(hi[k], ehi)):
                    bad.append((n, "order %d" % k, level, (m[k], lo[k], hi[k]), (mean, elo, ehi)))
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("S", SAMPLE_COUNTS)
def test_one_level_past_the_limit_raises_and_one_before_it_does_not(S):
    """lo = round(alpha / 2 S) - 1 must be > 0 (credible_intervals.py:49-50): alpha / 2 S = 1.45 raises, 1.55 does not"""
    raises, works = 1.0 - 2.9 / S, 1.0 - 3.1 / S
    assert summary.credible_interval_ranks(S, raises)[0] == 0 and summary.credible_interval_ranks(S, works)[0] == 1
    col = np.random.default_rng(S).random((S, 1))
    b = capi.SamplesBatch([col])
    with pytest.raises(capi.InternalError, match="Too few samples"):
        b.summarize(raises)
    with pytest.raises(capi.InternalError, match="Too few samples"):
        b.summarize(raises, as_text=True)
    b.summarize(works)
    m, lo, hi = b.summary(0)
    srt = np.sort(col[:, 0])
    lo_rank, hi_rank = summary.credible_interval_ranks(S, works)
    assert lo[0] == srt[lo_rank] and hi[0] == srt[hi_rank] and m[0] == tree_mean(col[:, 0])


def test_one_sample_fewer_than_the_smallest_admitted_raises():
    b = capi.SamplesBatch([np.random.default_rng(5).random((S_MIN - 1, 2))])
    with pytest.raises(capi.InternalError, match="Too few samples"):
        b.summarize(0.95)


@pytest.mark.parametrize("S", [257, 8193])
def test_mixed_isoform_counts_in_one_batch(S):
    """K = 1, 2, 7 and 20 in one batch: the grid is n x 20, so blocks with blockIdx.y >= K exist beside working ones.
    Column k of event i is a dyadic column + i + k / 32 (exact sums): every column's mean and bounds differ from every
    other's, so an indexing slip cannot pass.  x 10^4 the values end in .0, .25, .5 and .75: true ties among them."""
    rng = np.random.default_rng(S)
    Ks = [1, 20, 2, 7, 20, 1, 7, 2, 2]
    events = []
    for i, K in enumerate(Ks):
        base = rng.integers(0, 64, (S, K)) / 2048.0                     # < 1 / 32: the columns' ranges do not overlap
        events.append(base + i + np.arange(K) / 32.0)
    b = capi.SamplesBatch(events)
    for as_text in (False, True):
        for level in (0.95, 0.5):
            b.summarize(level, as_text=as_text)
            seen = set()
            for i, ev in enumerate(events):
                m, lo, hi = b.summary(i)
                assert len(m) == Ks[i]
                for k in range(Ks[i]):
                    col = ev[:, k]
                    vals = as_read(col) if as_text else col
                    elo, ehi = credible_interval(vals, level)
                    mean = text_mean(col, vals) if as_text else tree_mean(col)
                    assert (m[k], lo[k], hi[k]) == (mean, elo, ehi), (as_text, level, i, k)
                    if not as_text:
                        assert i + k / 32.0 <= lo[k] <= m[k] <= hi[k] < i + (k + 1) / 32.0
                    seen.add((m[k], lo[k], hi[k]))
            assert len(seen) == sum(Ks)


@pytest.mark.parametrize("S", [S_MIN, 257, 8193])
def test_four_decimal_columns_through_the_text_decoder_take_the_same_route(S):
    """Columns that four decimals express exactly, as `.miso` rows through SamplesBatch.from_text: the decoded pool and
    the parsed doubles give the same summaries, and both the reference's."""
    rng = np.random.default_rng(3000 + S)
    cols = {"constant": np.full(S, 0.3137), "two valued": np.where(rng.random(S) < 0.3, 0.25, 0.7501),
            "grid ties": rng.integers(0, 40, S) / 1e4 + 0.42, "signs": rng.integers(-30, 31, S) / 1e4,
            "up to 2e5": rng.integers(-2 * 10 ** 9, 2 * 10 ** 9, S) / 1e4}
    events, bodies = [], []
    for n, c in cols.items():
        srt = np.sort(c)
        rows = [["%.4f" % v for v in row] for row in orders(srt, rng)]
        bodies.append("".join("%s\t%.2f\n" % (",".join(r), -1.5 - j) for j, r in enumerate(rows)).encode())
        events.append(np.array([[float(f) for f in r] for r in rows]))
    offs = np.concatenate([[0], np.cumsum([len(x) for x in bodies])]).astype(np.int64)
    bt = capi.SamplesBatch.from_text(b"".join(bodies), offs, [4] * len(bodies), S)
    assert bt.status.tolist() == [0] * len(bodies)
    bs = capi.SamplesBatch(events)
    for level in LEVELS:
        for as_text in (False, True):
            bt.summarize(level, as_text=as_text)
            bs.summarize(level, as_text=as_text)
            for i, ev in enumerate(events):
                for got in (bt.summary(i), bs.summary(i)):
                    for k in range(4):
                        col = ev[:, k]
                        elo, ehi = credible_interval(col, level)
                        # (the values are what "%.4f" prints already: as_text rounds nothing, its mean is the digit sum)
                        mean = text_mean(col, col) if as_text else tree_mean(col)
                        assert same(got[0][k], mean) and same(got[1][k], elo) and same(got[2][k], ehi), (level, as_text, i, k)
