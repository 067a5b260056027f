"""CPU checker for the device Bayes factors: numpy restatement of
misopy/hypothesis_test.py:89-179 (delta densities) and :348-380 (Bayes factor), with the Gaussian
KDE of scipy.stats.gaussian_kde (third-party, outside /root/reference; the reference subclasses it
with a constant covariance factor, hypothesis_test.py:41-59) written out:
    cov = var(delta, ddof=1) * factor^2;  f(0) = sum exp(-delta^2 / (2 cov)) / (n sqrt(2 pi cov)).
Test infrastructure only."""
import numpy as np

MAX_BF = 1e12


def kde_at_zero(delta, factor=0.3):
    n = len(delta)
    cov = np.cov(delta, rowvar=1, bias=False) * factor ** 2
    return float(np.sum(np.exp(-(delta * delta) / (2 * cov))) / (n * np.sqrt(2 * np.pi * cov)))


def bayes_factor(x1, x2, factor=0.3):
    """-> (bayes_factor, posterior density at 0) for one isoform column pair."""
    d = np.asarray(x1, dtype=np.float64) - np.asarray(x2, dtype=np.float64)
    mad = np.mean(np.abs(d))
    all_same = bool(np.all(d - d[0] == 0))
    if mad <= .009 or all_same:           # NullPeakedDensity -> inf at 0 -> BF 0
        return 0.0, np.inf
    post = kde_at_zero(d, factor)
    if post == 0:
        return MAX_BF, post
    return min(1.0 / post, MAX_BF), post


# ---- the same at 50 digits (mpmath), on the double differences fl(u - v) as the reference program has them ----
def summation_depth(n):
    """additions one term passes through in the device's fixed order: ceil(n / 256) in its thread, 8 in the tree"""
    return -(-n // 256) + 8


def device_mean_abs(d):
    """mean|delta| in the device's summation order (compare_column: 256 strided partial sums, binary tree, / n)"""
    from _summary_ref import tree_mean
    return tree_mean(np.abs(np.asarray(d, dtype=np.float64)))


def exact_comparison(d, factor=0.3, digits=50):
    """d: the double differences.  Every quantity from the exact values of those doubles, `digits` decimal digits:
    {mad, all_same, null_peaked, var, cov, post, bf (uncapped 1 / post), amplification, sqrt_2pi_cov}.
    amplification = sum |x_i| e^{x_i} / sum e^{x_i}, x_i = -d_i^2 / (2 cov): what a relative error of the exponents
    (of cov, that is) becomes in the sum.  factor enters as the double it is, squared exactly."""
    import mpmath
    d = np.asarray(d, dtype=np.float64)
    n = len(d)
    with mpmath.workdps(digits):
        md = [mpmath.mpf(float(x)) for x in d]
        mad = mpmath.fsum(abs(x) for x in md) / n
        all_same = bool(np.all(d == d[0]))
        out = {"mad": mad, "all_same": all_same, "null_peaked": bool(mad <= mpmath.mpf(0.009)) or all_same}
        if all_same:
            return out
        mean = mpmath.fsum(md) / n
        var = mpmath.fsum((x - mean) ** 2 for x in md) / (n - 1)
        cov = var * mpmath.mpf(float(factor)) ** 2
        xs = [-(x * x) / (2 * cov) for x in md]
        es = [mpmath.exp(x) for x in xs]
        se = mpmath.fsum(es)
        root = mpmath.sqrt(2 * mpmath.pi * cov)
        post = se / (n * root)
        out.update(var=var, cov=cov, post=post, bf=1 / post, sqrt_2pi_cov=root,
                   amplification=mpmath.fsum(-x * e for x, e in zip(xs, es)) / se)
        return out


def density_error_bound(n, amplification):
    """First-order forward bound of the device's relative error in the density (tests/test_gpu_compare_exact.py derives
    it), without the absolute term for subnormal results.  u = 2^-53, D = summation_depth(n)."""
    u = 2.0 ** -53
    D = summation_depth(n)
    d_cov = (D + 7) * u
    return float(amplification) * (d_cov + 3 * u) + (2 + D) * u + (d_cov + 2 * u) / 2 + 4 * u
