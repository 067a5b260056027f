"""CPU references for the rank-normalised chain diagnostics (miso_batch_diagnose_rank,
miso_amd/csrc/kernels_diagnose_rank.hip).

* ``rank_fixed``  the definitions restated operation for operation: ranks from integer counts, the normal scores through
                  the `qnorm` it is given (the tests hand it the checker library's orc_det_qnorm, which
                  tests/test_detmath.py pins bit-equal to the kernels' miso_det_qnorm), and each transformed column,
                  placed at the used positions of a column of S values, through _diag_ref.diag_fixed -- the restatement
                  of the moments-and-Geyer stage.  Equal to the kernel's outputs bit for bit
                  (tests/test_gpu_diagnostics_rank.py).
* ``rank_plain``  the same definitions written independently with scipy.stats.rankdata(method="average") and
                  scipy.special.ndtri, and numpy's sort for the order statistics.
* ``refusal``     the message with which the pass refuses a shape (S, C, L), or None.
"""
import math

import numpy as np

import _diag_ref as R

OUTPUTS = ("rhat_bulk", "rhat_fold", "ess_bulk", "ess_ci_low", "ess_ci_high", "distinct")
MAX_DRAWS, MAX_CHAINS = 8192, 512


def bounds(N, level):
    """(lo, hi): summarize()'s order statistics, over N draws."""
    alpha = 1 - level
    return int(math.floor((alpha / 2) * N + 0.5)) - 1, int(math.floor((1 - alpha / 2) * N + 0.5)) - 1


def refusal(S, C, level):
    _, h, _, N = R.shape(S, C)
    if h < 4:
        return "Too few samples per chain for diagnostics"
    lo, hi = bounds(N, level)
    if not (lo > 0 and hi > 0 and hi < N):
        return "Too few samples for a credible interval"
    if N > MAX_DRAWS:
        return "Too many samples for rank diagnostics"
    if C > MAX_CHAINS:
        return "Too many chains for rank diagnostics"
    return None


def used_index(S, C):
    """Sample index of every used draw, at its flat index e = j h + i."""
    n, h, M, _ = R.shape(S, C)
    idx = np.empty((M, h), dtype=np.int64)
    i = np.arange(h)
    for c in range(C):
        idx[2 * c] = i * C + c
        idx[2 * c + 1] = (n - h + i) * C + c
    return idx.reshape(-1)


def r2_counts(v):
    """r2 = 2 less + equal + 1 of every element, from integer counts (the positions of a value in the sorted array)."""
    srt = np.sort(v)
    less = np.searchsorted(srt, v, side="left")
    equal = np.searchsorted(srt, v, side="right") - less
    return 2 * less + equal + 1


def normal_scores(r2, N, qnorm):
    return np.array([qnorm((0.5 * float(r) - 0.375) / (float(N) + 0.25)) for r in r2])


def rank_fixed(x, C, level, qnorm):
    """dict: the six outputs (OUTPUTS) of one column, and what they were made of: r2, z (bulk), r2_fold, lo, hi, thr_lo,
    thr_hi, med."""
    x = np.asarray(x, dtype=np.float64)
    S = len(x)
    why = refusal(S, C, level)
    if why:
        raise ValueError(why)
    _, _, _, N = R.shape(S, C)
    used = used_index(S, C)
    v = x[used]
    nan = math.nan
    if not np.isfinite(v).all():
        return dict(zip(OUTPUTS, (nan, nan, nan, nan, nan, 0)))
    with np.errstate(all="ignore"):
        srt = np.sort(v)
        lo, hi = bounds(N, level)
        med = 0.5 * srt[N // 2 - 1] + 0.5 * srt[N // 2]
        fold = np.abs(v - med)
        r2, r2_fold = r2_counts(v), r2_counts(fold)
        columns = {"bulk": normal_scores(r2, N, qnorm), "fold": normal_scores(r2_fold, N, qnorm),
                   "low": np.where(v <= srt[lo], 1.0, 0.0), "high": np.where(v >= srt[hi], 1.0, 0.0)}
    d = {}
    for name, t in columns.items():
        placed = np.zeros(S)
        placed[used] = t
        d[name] = R.diag_fixed(placed, C)
    return {"rhat_bulk": d["bulk"][0], "rhat_fold": d["fold"][0], "ess_bulk": d["bulk"][1], "ess_ci_low": d["low"][1],
            "ess_ci_high": d["high"][1], "distinct": int(1 + np.count_nonzero(srt[1:] != srt[:-1])),
            "r2": r2, "z": columns["bulk"], "r2_fold": r2_fold, "lo": lo, "hi": hi, "thr_lo": float(srt[lo]),
            "thr_hi": float(srt[hi]), "med": float(med)}


def _split_stats(seq):
    """(rhat, ess) of sequences [M, h] by the textbook formulas (numpy means and variances, Geyer's initial monotone
    sequence over pairs, the 1 / log10 N floor)."""
    M, h = seq.shape
    N = M * h
    means = seq.mean(axis=1)
    W = seq.var(axis=1, ddof=1).mean()
    V = W * (h - 1) / h + means.var(ddof=1)
    if not (W > 0 and math.isfinite(V)):
        return math.nan, math.nan
    d = seq - means[:, None]

    def rho(t):
        return 1.0 - (W - (d[:, :h - t] * d[:, t:]).sum(axis=1).mean() / h) / V

    total, prev, k = 0.0, None, 0
    while 2 * k + 1 <= h - 1:
        P = (1.0 if k == 0 else rho(2 * k)) + rho(2 * k + 1)
        if k >= 1:
            if not P > 0:
                break
            P = min(P, prev)
        total += P
        prev = P
        k += 1
    tau = max(-1.0 + 2.0 * total, 1.0 / math.log10(N))
    return math.sqrt(V / W), N / tau


def rank_plain(x, C, level):
    """The six outputs by an independent route: scipy's average ranks and ndtri."""
    from scipy import special, stats
    x = np.asarray(x, dtype=np.float64)
    seq = R.sequences(x, C)
    M, h = seq.shape
    N = M * h
    v = seq.reshape(-1)
    if not np.isfinite(v).all():
        return dict(zip(OUTPUTS, (math.nan,) * 5 + (0,)))

    def z(values):
        return special.ndtri((stats.rankdata(values, method="average") - 0.375) / (N + 0.25)).reshape(M, h)

    srt = np.sort(v)
    lo, hi = bounds(N, level)
    bulk = _split_stats(z(v))
    fold = _split_stats(z(np.abs(v - np.median(v))))
    low = _split_stats((v <= srt[lo]).astype(float).reshape(M, h))
    high = _split_stats((v >= srt[hi]).astype(float).reshape(M, h))
    return {"rhat_bulk": bulk[0], "rhat_fold": fold[0], "ess_bulk": bulk[1], "ess_ci_low": low[1], "ess_ci_high": high[1],
            "distinct": len(np.unique(v))}


def four_decimal_repeats(rng, C, draws, repeat=0.6):
    """A sample column of C chains as `--diagnose-samples` reads it: AR(1) around 0.5, printed to four decimals, and a
    share `repeat` of the draws repeating their chain's previous one (a rejected Metropolis-Hastings proposal)."""
    x = np.round(R.ar1(rng, 0.3, C, draws, mean=0.5, sd=0.04), 4).reshape(draws, C)
    stay = rng.random((draws, C)) < repeat
    for i in range(1, draws):
        x[i] = np.where(stay[i], x[i - 1], x[i])
    return x.reshape(-1)
