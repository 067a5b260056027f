"""GPU: the device functions the samplers are built from, each against an independent statement of what it computes
(include/miso_amd.h miso_selftest_*; csrc/kernels_selftest.hip calls the routines of the samplers' own .inl files).

* detmath: device miso_det_* and every csrc/detmath_n.hpp variant bit-equal to the host's routines on the point sets that
  tests/test_detmath.py ties to mpmath -- device against exact follows.
* draw thresholds (k2_threshold, k2_threshold_exact, flat_threshold / flat_threshold_fast as sampler_flat chooses between
  them, draw_threshold<LE>) against the DEFINITION: the number of 32-bit words u for which the reference's per-read test
  holds, counted by bisection in numpy float64 with no estimate involved.  An off-by-one threshold changes a count only when
  a Philox word lands on it (2^-32 per read): trajectory parity cannot see it, this can.
* count_below, the paired-end compare-and-count (pe_all_tests, pe_pick_exact) with ties built on purpose, binomial_coop<G>.

Not covered here (compares written inside loop bodies rather than as functions of their own): the two-isoform paired-end
loop's v_cmp_lt_f64 (kernels_k2.inl), and the packed 16-bit compare of the two-isoform single-end loop beyond what
test_gpu_k2's high-half tests force.  The MI_SLOW route of sampler_flat (a non-final threshold of 2^32) has no trajectory
test either: no input reaches it without a given starting psi."""
import numpy as np
import pytest

import _binomial_law as L
import _detmath_points as P
from miso_amd import capi

pytestmark = pytest.mark.gpu

TWO32 = 4294967296


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_same_doubles(dev, host, what):
    dev, host = np.asarray(dev), np.asarray(host)
    nan = np.isnan(host)
    assert np.array_equal(np.isnan(dev), nan), what
    bad = np.nonzero(_bits(dev)[~nan] != _bits(host)[~nan])[0]
    assert len(bad) == 0, (what, len(bad), [(float(host[~nan][i]).hex(), float(dev[~nan][i]).hex()) for i in bad[:5]])


@pytest.fixture(scope="module")
def points(orc):
    x = P.all_arguments()
    host = {name: np.array([getattr(orc.lib, fn)(float(v)) for v in x])
            for name, fn in (("exp", "orc_det_exp"), ("log", "orc_det_log"), ("sqrt", "orc_det_sqrt"), ("qnorm", "orc_qnorm_det"))}
    return x, host


def test_detmath_device_equals_host_on_the_mpmath_point_sets(points):
    x, host = points
    e, l, s, q = capi.selftest_detmath(x)
    for name, dev in (("exp", e), ("log", l), ("sqrt", s), ("qnorm", q)):
        _assert_same_doubles(dev, host[name], name)


@pytest.mark.parametrize("fn,name,widths", [(capi.SELFTEST_EXP_N, "exp", (1, 2, 3, 5)), (capi.SELFTEST_LOG_N, "log", (1, 2, 3, 5))])
def test_detmath_n_equals_host_for_every_width(points, fn, name, widths):
    """det_exp_n<N> / det_log_n<N>, coefficient tables in registers as the kernels load them; argument j of element i is
    point (i + j stride) mod n, so the N interleaved chains of one call carry different arguments."""
    x, host = points
    n = len(x)
    for width in widths:
        stride = 7919 * width + 1
        dev = capi.selftest_detmath_n(fn, x, width, stride)
        for j in range(width):
            idx = (np.arange(n) + j * stride) % n
            _assert_same_doubles(dev[:, j], host[name][idx], (name, width, j))


def test_detmath_t_and_sqrt_pos_equal_host(points):
    x, host = points
    _assert_same_doubles(capi.selftest_detmath_n(capi.SELFTEST_EXP_T, x)[:, 0], host["exp"], "det_exp_t")
    _assert_same_doubles(capi.selftest_detmath_n(capi.SELFTEST_LOG_T, x)[:, 0], host["log"], "det_log_t")
    ok = np.isfinite(x) & (x >= 2.2250738585072014e-308)       # det_sqrt_pos's stated domain: positive, normal, finite
    _assert_same_doubles(capi.selftest_detmath_n(capi.SELFTEST_SQRT_POS, x[ok])[:, 0], host["sqrt"][ok], "det_sqrt_pos")


# ---- draw thresholds ----
def threshold_by_definition(le, c, T):
    """#{u in [0, 2^32) : pred(u)}, pred(u) = (u 2^-32) T < c  resp.  !((u 2^-32) T > c), by bisection on u: the test is
    monotone in u (u 2^-32 is exact, a correctly rounded product with T >= 0 is monotone)."""
    c, T = np.asarray(c, np.float64), np.asarray(T, np.float64)
    lo = np.zeros(len(c), np.int64)                  # every u < lo passes
    hi = np.full(len(c), TWO32, np.int64)            # hi does not pass (u >= 2^32: false by definition)
    for _ in range(34):
        mid = (lo + hi) >> 1
        rnd = (mid.astype(np.float64) * 2.0 ** -32) * T
        p = ~(rnd > c) if le else (rnd < c)
        p &= mid < hi                                 # (lo == hi: settled)
        lo = np.where(p, mid + 1, lo)
        hi = np.where(p | (lo >= hi), hi, mid)
    assert np.array_equal(lo, hi)
    return lo.astype(np.uint64)


def _ulp_neighbours(c):
    return np.concatenate([c, np.nextafter(c, np.inf), np.nextafter(c, -np.inf).clip(min=0.0)])


def threshold_sets(n=1 << 20):
    """{name: (c, T)}: the kinds of input the samplers produce, the ties an off-by-one routine gets wrong, and what the
    two-test route refuses"""
    rng = np.random.default_rng(77)
    psi = rng.uniform(0, 1, n)
    a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    la, lb = 10.0 ** rng.uniform(-12, 0, n), 10.0 ** rng.uniform(-12, 0, n)
    sets = {"psi": (psi, psi + (1.0 - psi)), "two_uniform": (a, a + b), "log_uniform": (la, la + lb)}
    m = n // 3
    k = np.concatenate([rng.integers(0, TWO32, m - 4004), np.arange(0, 2002), np.arange(TWO32 - 2002, TWO32)]).astype(np.float64)
    # exact ties: a 20-bit T, so that k 2^-32 T is exact (32 + 20 bits) -- c IS the boundary, and c +- 1 ulp
    T20 = rng.integers(1 << 19, 1 << 20, m).astype(np.float64) * 2.0 ** rng.integers(-30, 10, m)
    sets["exact_ties"] = (_ulp_neighbours(k * 2.0 ** -32 * T20), np.tile(T20, 3))
    # c = fl(k 2^-32 T) for a 53-bit T: c is word k's rnd itself
    T53 = rng.uniform(0.5, 2.0, m)
    for name, scale in (("rnd_ties", 1.0), ("rnd_ties_1e279", 1e279), ("rnd_ties_1e-279", 1e-279)):
        Ts = T53 * scale
        sets[name] = (_ulp_neighbours(k * 2.0 ** -32 * Ts), np.tile(Ts, 3))
    ks = np.tile(np.arange(2, 2002, dtype=np.float64), n // 2000)
    Tk = rng.uniform(0.5, 2.0, len(ks))
    sets["small_k"] = (_ulp_neighbours(ks * 2.0 ** -32 * Tk), np.tile(Tk, 3))
    # what the two-test route refuses
    r = 4096
    Tr = rng.uniform(0.5, 2.0, r)
    sub = rng.integers(1, 1 << 52, r, dtype=np.int64).view(np.float64)
    big, small = 10.0 ** rng.uniform(280, 307, r), 10.0 ** rng.uniform(-307, -280, r)
    u = rng.uniform(0, 1, r)
    refused = {
        "est_below_2": (Tr * rng.uniform(0, 2.0 ** -31, r), Tr),
        "est_near_2^32": (Tr * (1.0 - rng.uniform(0, 4, r) * 2.0 ** -32), Tr),
        "c_equals_T": (Tr, Tr),
        "c_above_T": (Tr * (1.0 + u), Tr),
        "c_zero": (np.zeros(r), Tr),
        "T_huge": (u * big, big),
        "T_tiny": (u * small, small),
        "T_tiny_ties": (np.floor(u * TWO32) * 2.0 ** -32 * small, small),
        "T_subnormal": (np.floor(u * sub.view(np.int64)).astype(np.int64).view(np.float64), sub),
        "T_subnormal_c_normal": (u, sub),
        "T_5e-324": (np.where(u < 0.5, 0.0, 5e-324), np.full(r, 5e-324)),
        "both_zero": (np.zeros(r), np.zeros(r)),
        "T_zero": (u, np.zeros(r)),
        "c_subnormal": (sub, Tr),
        "T_largest": (u * 1.7976931348623157e308, np.full(r, 1.7976931348623157e308)),
    }
    sets.update(refused)
    return sets, list(refused)


ROUTINES = [("k2_threshold", capi.SELFTEST_K2_THRESHOLD, False), ("k2_threshold_exact", capi.SELFTEST_K2_THRESHOLD_EXACT, False),
            ("flat lt", capi.SELFTEST_FLAT_LT, False), ("flat le", capi.SELFTEST_FLAT_LE, True),
            ("flat_threshold lt", capi.SELFTEST_FLAT_GENERAL_LT, False), ("flat_threshold le", capi.SELFTEST_FLAT_GENERAL_LE, True),
            ("draw_threshold<false>", capi.SELFTEST_DRAW_LT, False), ("draw_threshold<true>", capi.SELFTEST_DRAW_LE, True)]


def _report(name, routine, c, T, got, want):
    bad = np.nonzero(got != want)[0]
    return (routine, name, "%d of %d differ" % (len(bad), len(c)),
            [("c", float(c[i]).hex(), "T", float(T[i]).hex(), "got", int(got[i]), "wanted", int(want[i])) for i in bad[:6]])


@pytest.fixture(scope="module")
def thresholds():
    sets, refused = threshold_sets()
    want = {(name, le): threshold_by_definition(le, c, T) for name, (c, T) in sets.items() for le in (False, True)}
    return sets, refused, want


def test_thresholds_equal_the_definition_for_every_finite_input(thresholds):
    """Every routine, every set, both rules: device == the count by definition.  No excluded region: the general routines
    fall back to a bisection on u, exact for every finite c >= 0, T >= 0 (subnormal T, T below 2^32 / DBL_MAX where the
    estimate 2^32 / T overflows, c == T == 0 included).
    (One arm no input can reach: k2_threshold's `t0 + 2`.  Its second test holds at t0 + 1 only if (t0 + 1) 2^-32 < p0 / T in
    the reals; rounding the quotient is monotone and (t0 + 1) 2^-32 is a double, so est = fl(p0 / T) 2^32 >= t0 + 1, against
    t0 = floor(est).  flat_threshold_fast's estimate c (2^32 / T) rounds twice and does reach it.)"""
    sets, _, want = thresholds
    for name, (c, T) in sets.items():
        for routine, code, le in ROUTINES:
            got = capi.selftest_threshold(code, c, T)
            assert np.array_equal(got, want[name, le]), _report(name, routine, c, T, got, want[name, le])


def test_fast_and_general_threshold_routines_agree_where_the_fast_one_applies(thresholds):
    sets, _, want = thresholds
    for name, (c, T) in sets.items():
        with np.errstate(all="ignore"):
            est = c * (4294967296.0 / T)
            ok = (T >= 1e-280) & (T <= 1e280) & (est >= 2.0) & (est <= 4294967293.0)
        if not ok.any():
            continue
        for le, fast, general in ((False, capi.SELFTEST_FLAT_FAST_LT, capi.SELFTEST_FLAT_GENERAL_LT),
                                  (True, capi.SELFTEST_FLAT_FAST_LE, capi.SELFTEST_FLAT_GENERAL_LE)):
            f = capi.selftest_threshold(fast, c[ok], T[ok])
            g = capi.selftest_threshold(general, c[ok], T[ok])
            assert np.array_equal(f, g), _report(name, "fast vs general, le=%s" % le, c[ok], T[ok], f, g)
            assert np.array_equal(f, want[name, le][ok]), _report(name, "flat_threshold_fast le=%s" % le, c[ok], T[ok], f, want[name, le][ok])


def test_threshold_route_is_chosen_per_wavefront(thresholds):
    """k2_threshold takes the two-test route only when ALL 64 lanes of the wavefront may (sampler_flat: when none needs the
    general one).  Wavefronts of 64 accepted inputs, of 64 refused ones, and of one refused lane -- at every lane position --
    among 63 accepted ones: every lane's count is the definition's, whichever route its wavefront took."""
    sets, refused, _ = thresholds
    rng = np.random.default_rng(78)
    sc, sT = sets["rnd_ties"]
    pick = rng.integers(0, len(sc), 64 * 200)
    with np.errstate(all="ignore"):
        est = sc[pick] / sT[pick] * 4294967296.0
    pick = pick[(est >= 2.0) & (est <= 4294967293.0)][:64 * 130]
    assert len(pick) == 64 * 130
    c, T = sc[pick].copy(), sT[pick].copy()                       # wavefronts 0 .. 129: all accepted
    rc = np.concatenate([sets[n][0][:64] for n in refused])
    rT = np.concatenate([sets[n][1][:64] for n in refused])
    for w in range(64):                                            # wavefronts 0 .. 63: one refused lane, at lane w
        c[64 * w + w], T[64 * w + w] = rc[(7 * w) % len(rc)], rT[(7 * w) % len(rc)]
    c, T = np.concatenate([c, rc]), np.concatenate([T, rT])        # behind them: wavefronts of refused inputs only
    for routine, code, le in ROUTINES:
        want = threshold_by_definition(le, c, T)
        got = capi.selftest_threshold(code, c, T)
        assert np.array_equal(got, want), _report("mixed wavefronts", routine, c, T, got, want)


def test_thresholds_of_non_finite_inputs_stay_in_range():
    """nan / inf weights are outside the contract: the call returns, with a count in [0, 2^32]"""
    v = np.array([np.nan, np.inf, -np.inf, 0.0, 1.0, -1.0])
    c, T = np.repeat(v, len(v)), np.tile(v, len(v))
    for routine, code, le in ROUTINES:
        got = capi.selftest_threshold(code, c, T)
        assert (got <= TWO32).all(), routine


def test_count_below_in_every_word_position():
    rng = np.random.default_rng(79)
    thr = np.concatenate([[0, 1, 0x80000000, 0xFFFFFFFF], rng.integers(2, 0xFFFFFFFF, 60)]).astype(np.uint64)
    rows, Ts = [], []
    for t in thr.tolist():
        words = np.array([0, 1, (t - 1) % TWO32, t, (t + 1) % TWO32, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000], np.uint64)
        for pos in range(4):
            for w in words:
                row = rng.integers(0, TWO32, 4).astype(np.uint64)
                row[pos] = w
                rows.append(row)
                Ts.append(t)
        g = np.array(np.meshgrid(words, words, words, words)).reshape(4, -1).T      # all of them in all positions at once
        rows.extend(g)
        Ts.extend([t] * len(g))
    w = np.array(rows, np.uint64).astype(np.uint32)
    T = np.array(Ts, np.uint64).astype(np.uint32)
    D = rng.integers(-1000, 1 << 30, len(T)).astype(np.int32)
    want = (D + (w < T[:, None]).sum(1)).astype(np.int32)
    got = capi.selftest_count_below(D, w, T)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(w[i].tolist(), int(T[i]), int(D[i]), int(got[i]), int(want[i])) for i in bad[:5]]


# ---- the paired-end draw ----
def pe_scan(frag, psi, fp, le, word):
    """the reference's scan (miso_paired.c:11-22, 64-75) as pe_pick_exact words it; weights summed over ascending isoforms"""
    zero = len(fp) - 2
    valid = [k for k in range(len(frag)) if frag[k] != zero]
    T = np.float64(0.0)
    for k in valid:
        T = T + np.float64(psi[k]) * np.float64(fp[frag[k]])
    rnd = np.float64(word) * 2.0 ** -32 * T
    cum = np.float64(0.0)
    for seen, k in enumerate(valid):
        cum = cum + np.float64(psi[k]) * np.float64(fp[frag[k]])
        stop = (not rnd > cum) if le else (rnd < cum if seen == 0 else True)
        if stop or seen == len(valid) - 1:
            return k, bool(rnd < T)
    raise AssertionError("no compatible isoform")


def _check_pe(frag, psi, fp, le, words, what):
    frag, psi = np.asarray(frag, np.uint8), np.asarray(psi, np.float64)
    le, words = np.asarray(le, np.uint32), np.asarray(words, np.uint32)
    dense, over, exact = capi.selftest_pe_pick(frag, psi, fp, le, words)
    n, K = frag.shape
    zero = len(fp) - 2
    for i in range(n):
        want, fast_ok = pe_scan(frag[i], psi[i], fp, bool(le[i]), int(words[i]))
        ctx = (what, i, frag[i].tolist(), [float(v).hex() for v in psi[i]], int(le[i]), hex(int(words[i])))
        assert exact[i] == want, ("pe_pick_exact", ctx, int(exact[i]), want)
        if fast_ok:                                   # rnd < T: the dense loop decides the read itself
            assert dense[i] == want, ("pe_all_tests pick", ctx, int(dense[i]), want)
            assert over[i].tolist() == [1 if k < want else 0 for k in range(K - 1)], ("over[]", ctx, over[i].tolist(), want)
        else:                                         # handed to pe_pick_exact; the tests passed over the leading incompatible isoforms
            assert dense[i] == -1, ("should leave the read to pe_pick_exact", ctx)
            lead = 0
            while lead < K - 1 and frag[i, lead] == zero:
                lead += 1
            assert over[i].tolist() == [1 if k < lead else 0 for k in range(K - 1)], ("over[] of a read left to pe_pick_exact", ctx)


def _fp_table(rng, il2=40):
    fp = rng.uniform(1e-4, 0.05, il2)
    fp[il2 - 2], fp[il2 - 1] = -0.0, 1.0              # incompatible; "probability one"
    return fp


def test_pe_draw_random_reads_every_mask():
    rng = np.random.default_rng(80)
    fp = _fp_table(rng)
    il2 = len(fp)
    for K in range(2, 9):
        masks = range(1, 1 << K) if K <= 5 else rng.integers(1, 1 << K, 40)
        frag, psi, le, words = [], [], [], []
        for m in masks:
            for _ in range(12 if K <= 5 else 30):
                f = rng.integers(0, il2 - 2, K)
                f[[k for k in range(K) if not (m >> k) & 1]] = il2 - 2
                p = rng.dirichlet(np.ones(K))
                frag.append(f); psi.append(p)
                le.append(0 if bin(int(m)).count("1") == 2 else 1)
                words.append(rng.choice([0, 1, 0xFFFFFFFF, 0x80000000, int(rng.integers(0, TWO32))], p=[.05, .05, .05, .05, .8]))
        _check_pe(frag, psi, fp, le, words, "random K=%d" % K)


def test_pe_draw_ties_built_on_purpose():
    """rnd == c_k exactly, for each k, under both rules (the two differ ONLY there), with the words next to the tie;
    rnd == +0 (word 0); incompatible isoforms in front, between and behind; a compatible isoform of weight +0.0.
    psi and the fragment probabilities are small dyadic rationals, and the last compatible isoform tops the total up to a
    power of two, so that every product and sum is exact and word = (c_k / T) 2^32 is an integer: rnd IS c_k."""
    il2 = 12
    fp = np.array([0.5, 0.25, 0.125, 0.75, 0.375, 1.0, 0.0, 0.0625, 0.625, 0.875, -0.0, 1.0])
    rng = np.random.default_rng(81)
    for K in range(2, 9):
        frag, psi, le, words, n_ties = [], [], [], [], 0
        for trial in range(80):
            ncomp = 2 if trial % 3 == 0 else int(rng.integers(2, K + 1))
            comp = sorted(rng.choice(K, ncomp, replace=False).tolist())
            f = np.full(K, il2 - 2)
            f[comp] = rng.integers(0, 10, ncomp)
            p = rng.integers(1, 16, K) / 64.0
            if trial % 5 == 0 and ncomp > 2:
                p[comp[int(rng.integers(0, ncomp - 1))]] = 0.0      # a compatible isoform of weight +0.0
            f[comp[-1]] = 5                                        # fp = 1.0: its psi is its weight
            partial = sum(p[k] * fp[f[k]] for k in comp[:-1])      # exact: a multiple of 2^-10
            T = 2.0 ** np.floor(np.log2(partial) + 1) if partial > 0 else 0.25
            p[comp[-1]] = T - partial
            cum = np.cumsum([p[k] * fp[f[k]] for k in comp])
            assert cum[-1] == T and p[comp[-1]] > 0
            rule = 0 if ncomp == 2 else 1
            for ck in cum[:-1]:
                tie = int(ck / T * TWO32)
                assert tie * 2.0 ** -32 * T == ck                   # the word whose rnd is c_k
                n_ties += 1
                for wd in (0, tie - 1, tie, tie + 1):
                    if 0 <= wd < TWO32:
                        frag.append(f.copy()); psi.append(p.copy()); le.append(rule); words.append(wd)
        assert n_ties >= 80
        _check_pe(frag, psi, fp, le, words, "ties K=%d" % K)
        # the reads with two compatible isoforms under the other rule too: what a kernel that mixed the rules up would
        # compute (the reference never asks; the routines take the rule as an input, so the question is valid)
        two = [i for i in range(len(le)) if le[i] == 0]
        _check_pe([frag[i] for i in two], [psi[i] for i in two], fp, [1] * len(two), [words[i] for i in two], "ties, `!(rnd > c)` on two, K=%d" % K)


def test_pe_draw_total_weight_zero_goes_to_the_exact_scan():
    fp = np.array([0.5, 0.0, -0.0, 1.0])
    frag = [[0, 1, 2], [1, 1, 2], [2, 1, 0], [1, 2, 1]]
    psi = [[0.0, 0.5, 0.5], [0.25, 0.5, 0.25], [0.5, 0.5, 0.0], [0.3, 0.3, 0.4]]
    for word in (0, 12345, 0xFFFFFFFF):
        _check_pe(frag, psi, fp, [0, 0, 0, 0], [word] * 4, "T == 0, two compatible")
    _check_pe([[0, 1, 1], [1, 1, 1]], [[0.0, 0.5, 0.5], [0.2, 0.3, 0.5]], fp, [1, 1], [0, 99], "T == 0, three compatible")


# ---- the collapsed step's binomial ----
@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_binomial_coop_equals_the_sequential_routine(orc, G):
    ps = [0.0, 1e-12, 0.01, 0.2, 0.5, 0.8, 1 - 1e-12, 1.0]
    for n in (0, 1, 9, 10, 11, 50, 1000, 60000):
        sw = []
        if n >= 20:                                    # n min(p, q) just either side of 10: inversion / BTRS
            r = 10.0 / n
            sw = [np.nextafter(r, 0), r, np.nextafter(r, 1), 1 - r, np.nextafter(1 - r, 0), np.nextafter(1 - r, 1), r * 0.999, r * 1.001]
        for p in ps + sw:
            want = orc.binomial(n, float(p), 256, seed=5, event_id=n)
            got = capi.selftest_binomial(G, n, float(p), 256, seed=5, event_id=n)
            assert np.array_equal(got, want), (G, n, float(p).hex(), got[:8], want[:8])
    # ... and at the points where the sequential routine is tied to the exact law (tests/test_binomial_law.py)
    for n, p, _ in L.CASES:
        if (n, p) in L.DEGENERATE:
            continue
        want = orc.binomial(n, p, 256, seed=5, event_id=n)
        got = capi.selftest_binomial(G, n, p, 256, seed=5, event_id=n)
        assert np.array_equal(got, want), (G, n, float(p).hex(), got[:8], want[:8])
