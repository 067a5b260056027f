"""GPU: compare_kernel through capi.SamplesBatch(arrays) against an EXACT reference (_compare_ref.exact_comparison: mpmath at
50 digits on the double differences fl(u - v)), with a derived tolerance.  tests/test_gpu_compare.py holds the kernel
to 1e-9 against a double-precision restatement on the sampler's own output; here the columns are chosen: S = 2, 3, 257,
8192, 8193 (the register cache's limit) and 20000, mixed isoform counts in one batch (blocks with k >= K return early
beside working ones), all differences 0.25, all but one, mean|delta| just under and just over 0.009, a density in the
subnormals, a density of 0, 1 / density just under and just over the 1e12 cap, smoothing 0.3, 0.5 and 0.05, NaN.

Means: bit for bit _summary_ref.tree_mean.  Branch (null peaked or not): equal to `mean|delta| <= 0.009 or all equal`
with mean|delta| summed in the device's order (_compare_ref.device_mean_abs), bit for bit; the threshold cases are built
so that the exact rational mean|delta| is at least 1e-12 from 0.009 on the intended side, which
tests/test_compare_exact_ref.py checks on the CPU, so that the numpy restatement, the exact one and the device agree.

The tolerance for density and Bayes factor, first order in u = 2^-53, D = ceil(S / 256) + 8 the additions a term
passes through in the fixed summation order (its thread's strided sum, then eight tree levels):

  cov    dev_i = d_i - mean (u; the mean's own error enters sum dev_i^2 only at second order, sum (d_i - m) = 0),
         squared (2u + u), summed (D u), / (n - 1) (u), smoothing^2 (u), their product (u):       d_cov = (D + 7) u
  x_i    = -(d_i d_i) (1 / (2 cov)): d_cov + 3u.  e^{x (1 + r)} = e^x (1 + x r): in the sum that is
         A (d_cov + 3u), A = sum |x_i| e^{x_i} / sum e^{x_i}, which the reference computes per case
  sum    miso_det_exp within 1 ulp (tests/test_detmath.py): 2u; D additions of positive terms: D u
  denom  n sqrt(2 pi cov): the constant (u), x cov (u), half of (d_cov + 2u) under the root, miso_det_sqrt within
         1 ulp (2u), x n (u), the division (u)
  total  A (d_cov + 3u) + (2 + D) u + (d_cov + 2u) / 2 + 4u            (_compare_ref.density_error_bound)
  plus   S 2^-1074 / density: terms and results in the subnormals carry an absolute error: each of the S terms up to
         2^-1074 before the division by n sqrt(2 pi cov), the quotient's own rounding 2^-1075, together
         (1 / sqrt(2 pi cov) + 1/2) 2^-1074, which S 2^-1074 covers unless the kernel is narrower than 1 / S (S = 2, 3
         at smoothing 0.05): there the derived factor stands in for S
  Bayes factor = 1 / density: + u.
2 x that is allowed, for the second-order terms.  Nothing here was tuned to what the device returns; the worst
observed error / bound per case family is printed (run with -s)."""
import mpmath
import numpy as np
import pytest

from _compare_columns import SAMPLE_COUNTS, columns
from _compare_ref import (bayes_factor, density_error_bound, device_mean_abs, exact_comparison)
from _summary_ref import tree_mean
from miso_amd import capi

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SMOOTHINGS = (0.3, 0.5, 0.05)


def _layout(names, Ks):
    """column j of the batch -> (event, isoform): the events' isoform counts in turn"""
    where, i = [], 0
    while len(where) < len(names):
        for k in range(Ks[i % len(Ks)]):
            where.append((i, k))
        i += 1
    return where[:len(names)], i


@pytest.mark.parametrize("S", SAMPLE_COUNTS)
def test_compare_against_the_exact_reference(S):
    rng = np.random.default_rng(S)
    col = columns(S, rng)
    names = list(col)
    # mixed isoform counts in one batch; the columns behind the last case are filled with distinguishable psi
    Ks = [1, 3, 2, 7]
    where, n_events = _layout(names, Ks)
    ev1 = [np.empty((S, Ks[i % len(Ks)])) for i in range(n_events)]
    ev2 = [np.empty((S, Ks[i % len(Ks)])) for i in range(n_events)]
    cases = {}
    for i in range(n_events):
        for k in range(ev1[i].shape[1]):
            ev1[i][:, k] = rng.random(S) + i + k / 32.0
            ev2[i][:, k] = rng.random(S)
    for n, (i, k) in zip(names, where):
        ev1[i][:, k], ev2[i][:, k] = col[n]
    for i in range(n_events):
        for k in range(ev1[i].shape[1]):
            cases[i, k] = next((n for n, w in zip(names, where) if w == (i, k)), "filler")
    b1, b2 = capi.SamplesBatch(ev1), capi.SamplesBatch(ev2)
    failures, worst = [], {}                 # worst: (case, smoothing) -> worst error / (2 x bound) seen
    for factor in SMOOTHINGS:
        b1.compare(b2, factor)
        for i in range(n_events):
            m1, m2, bf, dens = b1.comparison(i)
            assert len(bf) == ev1[i].shape[1]
            for k in range(ev1[i].shape[1]):
                name = cases[i, k]
                u, v = ev1[i][:, k], ev2[i][:, k]
                e1, e2 = tree_mean(u), tree_mean(v)
                assert (m1[k] == e1 or (e1 != e1 and m1[k] != m1[k])) and (m2[k] == e2 or (e2 != e2 and m2[k] != m2[k])), (name, i, k)
                d = u - v
                if name == "nan in one column":                         # pinned to the numpy restatement
                    ebf, edens = bayes_factor(u, v, factor)
                    assert np.isnan(ebf) and np.isnan(edens) and np.isnan(bf[k]) and np.isnan(dens[k]), (bf[k], dens[k])
                    continue
                null = device_mean_abs(d) <= 0.009 or bool(np.all(d - d[0] == 0))
                got_null = bf[k] == 0.0 and np.isposinf(dens[k])
                assert got_null == null, (name, factor, bf[k], dens[k])
                ex = exact_comparison(d, factor)
                assert bool(ex["null_peaked"]) == null, (name, "the exact branch and the device-order branch differ")
                if null:
                    assert name in ("all 0.25", "mad just under") or S <= 3, name
                    continue
                post = ex["post"]
                rel = density_error_bound(S, ex["amplification"])
                # relative: S 2^-1074 / density -- or, with few samples under a narrow kernel, the factor it derives from
                absolute = max(S, float(1 / ex["sqrt_2pi_cov"]) + 0.5) * 2.0 ** -1074
                err = abs(float(dens[k] - post))
                tol = 2 * (rel * float(post) + absolute)
                ratio = err / tol
                worst[name, factor] = max(worst.get((name, factor), 0.0), ratio)
                if not err <= tol:
                    failures.append((name, factor, "density", dens[k], float(post), ratio))
                # the Bayes factor: 1 / density, capped at 1e12, 1e12 when the density is 0
                rel_bf = 2 * (rel + U + absolute / float(post)) if post > mpmath.mpf(2) ** -1080 else np.inf
                if ex["bf"] * (1 - min(rel_bf, 0.5)) > 1e12:
                    if bf[k] != 1e12:
                        failures.append((name, factor, "cap", bf[k], float(ex["bf"]), np.inf))
                elif ex["bf"] * (1 + rel_bf) < 1e12:
                    r = abs(float(bf[k] - ex["bf"])) / (rel_bf * float(ex["bf"]))
                    worst[name + " (bf)", factor] = max(worst.get((name + " (bf)", factor), 0.0), r)
                    if not r <= 1:
                        failures.append((name, factor, "bf", bf[k], float(ex["bf"]), r))
                else:
                    failures.append((name, factor, "the case is too close to the cap to say which side", bf[k], float(ex["bf"]), 0))
                # what the case claims to be, at the smoothing it was built for
                if factor == 0.3:
                    if name == "density subnormal":
                        assert 2.0 ** -1060 < post < 2.0 ** -1022 and 0 < dens[k] < 2.2250738585072014e-308 and bf[k] == 1e12
                    elif name == "density zero":
                        assert post < mpmath.mpf(2) ** -1100 and dens[k] == 0.0 and bf[k] == 1e12
                    elif name == "just under the cap":
                        assert 1e12 * (1 - 1e-8) < ex["bf"] < 1e12 and bf[k] < 1e12
                    elif name == "just over the cap":
                        assert 1e12 < ex["bf"] < 1e12 * (1 + 1e-8) and bf[k] == 1e12
                    elif name == "all 0.25 but one":
                        assert not null
    print("S = %d: worst error / allowed (2 x bound) per case and smoothing" % S)
    for (name, factor), r in sorted(worst.items()):
        print("  %-28s smoothing %-5g %.4f" % (name, factor, r))
    assert not failures, failures


def test_all_equal_differences_and_sample_count_errors():
    S = 257
    dy = np.random.default_rng(1).integers(16, 64, (S, 3)) / 64.0
    b1, b2 = capi.SamplesBatch([dy]), capi.SamplesBatch([dy - 0.25])
    b1.compare(b2)
    m1, m2, bf, dens = b1.comparison(0)
    assert bf.tolist() == [0.0] * 3 and np.all(np.isposinf(dens))          # Bayes factor 0, density inf
    one = capi.SamplesBatch([dy[:1]])
    with pytest.raises(capi.InternalError, match="Too few samples"):
        one.compare(capi.SamplesBatch([dy[:1] - 0.25]))
    with pytest.raises(capi.InternalError, match="differ"):
        b1.compare(capi.SamplesBatch([dy[:200]]))
    with pytest.raises(capi.InternalError, match="isoforms"):
        b1.compare(capi.SamplesBatch([dy[:, :2]]))


@pytest.mark.parametrize("S", [3, 257, 8193])
def test_decimal_columns_through_the_text_decoder_compare_the_same(S):
    """Columns that 15 digits express exactly, as `.miso` rows through SamplesBatch.from_text on both sides: the decoded
    pools give the comparison of the parsed doubles bit for bit (and that one is held to the exact reference above)."""
    rng = np.random.default_rng(40 + S)
    dy = rng.integers(16, 64, S) / 64.0
    one = dy - 0.25
    one[S // 2] = dy[S // 2] - 0.5
    step = (1 + np.arange(S) % 3) * 1e-12                       # 0.009 -+ 1, 2, 3 x 10^-12: thirteen decimals
    sign = np.where(np.arange(S) % 2 == 0, 1, -1)
    fmt = "%.13f"
    sides = []
    for cols in ([dy, dy, np.round(rng.random(S), 4), 0.5 + sign * (0.009 - step), 0.5 + sign * (0.009 + step)],
                 [dy - 0.25, one, np.round(rng.random(S), 4), np.full(S, 0.5), np.full(S, 0.5)]):
        rows = [[fmt % v for v in row] for row in np.stack(cols, axis=1)]
        assert all(len(f.replace(".", "").replace("-", "").lstrip("0")) <= 15 for r in rows for f in r)
        body = "".join("%s\t%.2f\n" % (",".join(r), -2.0 - j) for j, r in enumerate(rows)).encode()
        parsed = np.array([[float(f) for f in r] for r in rows])
        bt = capi.SamplesBatch.from_text(body, np.array([0, len(body)], np.int64), [5], S)
        assert bt.status.tolist() == [0]
        sides.append((bt, capi.SamplesBatch([parsed]), parsed))
    for factor in SMOOTHINGS:
        sides[0][0].compare(sides[1][0], factor)
        sides[0][1].compare(sides[1][1], factor)
        text, arrays = sides[0][0].comparison(0), sides[0][1].comparison(0)
        for a, b in zip(text, arrays):
            assert a.view(np.uint64).tolist() == b.view(np.uint64).tolist(), factor
        m1, m2, bf, dens = arrays
        d = sides[0][2] - sides[1][2]
        for k in range(5):
            null = device_mean_abs(d[:, k]) <= 0.009 or bool(np.all(d[:, k] - d[0, k] == 0))
            assert (bf[k] == 0.0 and np.isposinf(dens[k])) == null, (factor, k)
            assert m1[k] == tree_mean(sides[0][2][:, k]) and m2[k] == tree_mean(sides[1][2][:, k])
        assert bf[0] == 0.0 and bf[3] == 0.0 and (S <= 3 or (bf[1] > 0 and bf[4] > 0))
