"""Two-sample comparison output -- the `.miso_bf` side of `compare_miso`
(misopy/hypothesis_test.py:186-345), fed from the Bayes factors, means and credible intervals the
device computes (`miso_batch_compare`, `miso_batch_summarize`).
"""
from decimal import Decimal

import numpy as np

HEADER_FIELDS = ["event_name", "sample1_posterior_mean", "sample1_ci_low", "sample1_ci_high",
                 "sample2_posterior_mean", "sample2_ci_low", "sample2_ci_high", "diff",
                 "bayes_factor", "isoforms", "sample1_counts", "sample1_assigned_counts",
                 "sample2_counts", "sample2_assigned_counts", "chrom", "strand", "mRNA_starts",
                 "mRNA_ends"]

MAX_BF = 1e12           # hypothesis_test.py:352


def _py2_str(x):
    """str(float) of Python 2 (12 significant digits) -- what the reference feeds to Decimal."""
    return "%.12g" % x


def comparison_fields(event_name, summary1, summary2, bayes_factors):
    """summaryN = (means, ci_low, ci_high) of sample N.  hypothesis_test.py:283-311: two isoforms ->
    means quantised to 2 decimals (Decimal, half-even) and their difference; more -> comma lists of
    "%.2f", diff from the raw means, negative Bayes factors clipped to 0."""
    m1, lo1, hi1 = summary1
    m2, lo2, hi2 = summary2
    K = len(m1)
    if K == 2:
        q = Decimal("0.01")
        d1 = Decimal(_py2_str(m1[0])).quantize(q)
        d2 = Decimal(_py2_str(m2[0])).quantize(q)
        return [event_name, "%s" % d1, "%.2f" % lo1[0], "%.2f" % hi1[0],
                "%s" % d2, "%.2f" % lo2[0], "%.2f" % hi2[0],
                "%.2f" % (d1 - d2), "%.2f" % bayes_factors[0]]
    join = lambda v: ",".join("%.2f" % x for x in v)  # noqa: E731
    return [event_name, join(m1), join(lo1), join(hi1), join(m2), join(lo2), join(hi2),
            join([a - b for a, b in zip(m1, m2)]), join([max(v, 0) for v in bayes_factors])]


def comparison_line(event_name, summary1, summary2, bayes_factors, header1, header2):
    f = comparison_fields(event_name, summary1, summary2, bayes_factors)
    f.append(header1["isoforms"])
    f += [header1["counts"], header1["assigned_counts"], header2["counts"], header2["assigned_counts"]]
    for key in ("chrom", "strand", "mRNA_starts", "mRNA_ends"):
        f.append(header1.get(key, "NA"))
    return "\t".join(f)


def write_comparison(filename, rows):
    """rows: iterable of (event_name, summary1, summary2, bayes_factors, header1, header2)."""
    n = 0
    with open(filename, "w") as f:
        f.write("\t".join(HEADER_FIELDS) + "\n")
        for row in rows:
            f.write(comparison_line(*row) + "\n")
            n += 1
    return n


# ---- the exact comparison's table, `<label1>_vs_<label2>.miso_bf_exact` beside the `.miso_bf` ----
DEFAULT_DELTA_THRESHOLDS = (0.1, 0.2)
MAX_DELTA_THRESHOLDS = 4            # two points of the CDF each, miso_batch_compare_exact takes eight


def check_delta_thresholds(thresholds):
    """the thresholds as floats; ValueError unless there are 1 .. 4 of them, each inside (0, 1)"""
    t = [float(x) for x in thresholds]
    if not 1 <= len(t) <= MAX_DELTA_THRESHOLDS:
        raise ValueError("Error: between 1 and %d delta psi thresholds, got %d" % (MAX_DELTA_THRESHOLDS, len(t)))
    for x in t:
        if not 0.0 < x < 1.0:
            raise ValueError("Error: delta psi threshold %r outside (0, 1)" % x)
    return t


def delta_points(thresholds):
    """where the exact comparison evaluates the CDF of psi_1 - psi_2: (t, -t) of every threshold"""
    return tuple(z for t in check_delta_thresholds(thresholds) for z in (t, -t))


def exact_header_fields(thresholds):
    return HEADER_FIELDS + ["exact", "log10_bayes_factor"] + ["prob_abs_diff_ge_%g" % t for t in thresholds]


def exact_comparison_line(event_name, summary1, summary2, bayes_factors, header1, header2, exact, thresholds):
    """exact = None: the event's `.miso_bf` line, then exact = 0 and NA.  Otherwise (mean1, mean2, log_density_at_0,
    bayes_factor, log10_bayes_factor, cdf at delta_points(thresholds), grid summary of sample 1, of sample 2) as
    pysplicing.MISOCompareBatch(exact_compare=) returns it: means, bounds and difference from the grid as %.4f, the capped
    Bayes factor as %.2f, P(|psi_1 - psi_2| >= t) = 1 - H(t) + H(-t) per threshold."""
    if exact is None:
        return "\t".join([comparison_line(event_name, summary1, summary2, bayes_factors, header1, header2), "0", "NA"]
                         + ["NA"] * len(thresholds))
    return "\t".join(exact_head_fields(event_name, header1, header2, exact) + ["1", "%.4f" % exact[4]]
                     + exact_prob_fields(exact[5], thresholds))


def exact_head_fields(event_name, header1, header2, exact):
    """the HEADER_FIELDS part of an exact-comparable event's row: the summaries from the grid"""
    mean1, mean2, _, bf, _, _, (m1, lo1, hi1), (m2, lo2, hi2) = exact
    f = [event_name, "%.4f" % m1[0], "%.4f" % lo1[0], "%.4f" % hi1[0], "%.4f" % m2[0], "%.4f" % lo2[0], "%.4f" % hi2[0],
         "%.4f" % (mean1 - mean2), "%.2f" % min(bf, MAX_BF), header1["isoforms"],
         header1["counts"], header1["assigned_counts"], header2["counts"], header2["assigned_counts"]]
    for key in ("chrom", "strand", "mRNA_starts", "mRNA_ends"):
        f.append(header1.get(key, "NA"))
    return f


def exact_prob_fields(cdf, thresholds):
    """P(|psi_1 - psi_2| >= t) = 1 - H(t) + H(-t) per threshold, cdf at delta_points(thresholds)"""
    return ["%.4f" % ((1.0 - cdf[2 * j]) + cdf[2 * j + 1]) for j in range(len(thresholds))]


def write_exact_comparison(filename, rows, thresholds):
    """rows: iterable of (event_name, summary1, summary2, bayes_factors, header1, header2, exact) -- write_comparison's
    row and the event's exact comparison, or None where the pair was not exact-comparable."""
    thresholds = check_delta_thresholds(thresholds)
    n = 0
    with open(filename, "w") as f:
        f.write("\t".join(exact_header_fields(thresholds)) + "\n")
        for row in rows:
            f.write(exact_comparison_line(*row, thresholds=thresholds) + "\n")
            n += 1
    return n


# ---- the all-pairs table, `<label1>_vs_<label2>.miso_dpsi` beside the `.miso_bf` ----
DPSI_FIELDS = ["delta_psi_median", "delta_psi_ci_low", "delta_psi_ci_high", "prob_diff_gt_0", "prob_diff_lt_0"]


def dpsi_header_fields(thresholds):
    return HEADER_FIELDS + DPSI_FIELDS + ["prob_abs_diff_ge_%g" % t for t in thresholds]


def dpsi_fields(pairs, n_thresholds):
    """pairs = (median[K], ci_low[K], ci_high[K], n_gt0[K], n_lt0[K], n_abs_ge[K, n_tau], finite[K], n_pairs) as
    capi.Batch.pair_comparison(i) returns it: the three doubles and the probabilities count / n_pairs as %.4f; two isoforms
    -> isoform 0, more -> comma lists over the isoforms (as comparison_fields); a column that is not finite prints NA.
    pairs = None (the pass did not take the event: too many draws): NA in every field."""
    if pairs is None:
        return ["NA"] * (len(DPSI_FIELDS) + n_thresholds)
    med, lo, hi, gt, lt, ge, fin, M = pairs
    ks = [0] if len(med) == 2 else range(len(med))
    M = float(M)

    def col(value):
        return ",".join(("%.4f" % value(k)) if fin[k] else "NA" for k in ks)
    f = [col(lambda k: med[k]), col(lambda k: lo[k]), col(lambda k: hi[k]), col(lambda k: gt[k] / M), col(lambda k: lt[k] / M)]
    f += [col(lambda k, j=j: ge[k][j] / M) for j in range(n_thresholds)]
    return f


def dpsi_line(bf_line, pairs, n_thresholds):
    """bf_line: the event's `.miso_bf` line, verbatim (comparison_line)"""
    return "\t".join([bf_line] + dpsi_fields(pairs, n_thresholds))


def write_dpsi(filename, rows, thresholds):
    """rows: iterable of (event_name, summary1, summary2, bayes_factors, header1, header2, pairs) -- write_comparison's row
    and the event's all-pairs results.  The quantities are those of the doubles the device holds: a pair of four-decimal
    draws whose decimal difference equals a threshold exactly may fall on either side of it (0.3 - 0.1 < 0.2)."""
    thresholds = check_delta_thresholds(thresholds)
    n = 0
    with open(filename, "w") as f:
        f.write("\t".join(dpsi_header_fields(thresholds)) + "\n")
        for row in rows:
            f.write(dpsi_line(comparison_line(*row[:6]), row[6], len(thresholds)) + "\n")
            n += 1
    return n


# ---- the exact comparison's delta psi table, `<label1>_vs_<label2>.miso_dpsi_exact` ----
EXACT_DPSI_PROBS = (0.5, 0.025, 0.975)      # median and the 95 % credible interval, as `.miso_dpsi`'s confidence level


def exact_dpsi_header_fields(thresholds):
    return HEADER_FIELDS + ["exact"] + DPSI_FIELDS + ["prob_abs_diff_ge_%g" % t for t in thresholds]


def exact_dpsi_line(event_name, summary1, summary2, bayes_factors, header1, header2, exact, delta, thresholds):
    """exact: as exact_comparison_line's; delta = (quantiles of psi_1 - psi_2 at EXACT_DPSI_PROBS, H(0)) as
    capi.Batch.exact_delta(i) returns it.  Either None: the event's `.miso_bf` line, then exact = 0 and NA.  Otherwise the
    `.miso_bf_exact` row's leading fields, 1, median and interval as %.4f, P(diff > 0) = 1 - H(0) and P(diff < 0) = H(0) (the
    law has no atom at 0), and `.miso_bf_exact`'s P(|psi_1 - psi_2| >= t)."""
    if exact is None or delta is None:
        return "\t".join([comparison_line(event_name, summary1, summary2, bayes_factors, header1, header2), "0"]
                         + ["NA"] * (len(DPSI_FIELDS) + len(thresholds)))
    q, h0 = delta
    f = exact_head_fields(event_name, header1, header2, exact) + ["1"]
    f += ["%.4f" % q[0], "%.4f" % q[1], "%.4f" % q[2], "%.4f" % (1.0 - h0), "%.4f" % h0]
    return "\t".join(f + exact_prob_fields(exact[5], thresholds))


def write_exact_dpsi(filename, rows, thresholds):
    """rows: iterable of (event_name, summary1, summary2, bayes_factors, header1, header2, exact, delta) --
    write_exact_comparison's row and the event's exact quantiles of delta psi."""
    thresholds = check_delta_thresholds(thresholds)
    n = 0
    with open(filename, "w") as f:
        f.write("\t".join(exact_dpsi_header_fields(thresholds)) + "\n")
        for row in rows:
            f.write(exact_dpsi_line(*row, thresholds=thresholds) + "\n")
            n += 1
    return n


# ---- the pooled table of two replicate groups, `<A>_vs_<B>/delta-psi/<A>_vs_<B>.miso_group_dpsi` ----
GROUP_DPSI_HEAD = ["event_name", "group1_replicates", "group2_replicates", "group1_posterior_mean", "group2_posterior_mean",
                   "diff"]
GROUP_DPSI_TAIL = ["isoforms", "chrom", "strand", "mRNA_starts", "mRNA_ends"]


def group_dpsi_header_fields(thresholds):
    return GROUP_DPSI_HEAD + DPSI_FIELDS + ["prob_abs_diff_ge_%g" % t for t in thresholds] + GROUP_DPSI_TAIL


def group_mean(means):
    """means: per replicate, in replicate order, the K double means of its summary -> their mean per isoform, summed in that
    order and divided once"""
    K = len(means[0])
    out = []
    for k in range(K):
        acc = 0.0
        for m in means:
            acc += float(m[k])
        out.append(acc / len(means))
    return out


def group_dpsi_line(event_name, n1, n2, means1, means2, pairs, header, n_thresholds):
    """n1, n2: the samples of either group that were pooled (that have the event).  means1, means2: group_mean's input per
    group, or None: NA in both means and their difference.  pairs: dpsi_fields' -- capi.GroupPairComparison.pair_comparison's
    tuple, or None: NA in every pooled field.  header: the header fields of the first pooled group-1 sample."""
    f = [event_name, "%d" % n1, "%d" % n2]
    if means1 is None or means2 is None:
        f += ["NA"] * 3
    else:
        m1, m2 = group_mean(means1), group_mean(means2)
        ks = [0] if len(m1) == 2 else range(len(m1))
        join = lambda v: ",".join("%.4f" % v[k] for k in ks)  # noqa: E731
        f += [join(m1), join(m2), join([a - b for a, b in zip(m1, m2)])]
    f += dpsi_fields(pairs, n_thresholds)
    f.append(header.get("isoforms", "NA"))
    for key in ("chrom", "strand", "mRNA_starts", "mRNA_ends"):
        f.append(header.get(key, "NA"))
    return "\t".join(f)


def write_group_dpsi(filename, rows, thresholds):
    """rows: iterable of (event_name, n1, n2, means1, means2, pairs, header) -- group_dpsi_line's arguments."""
    thresholds = check_delta_thresholds(thresholds)
    n = 0
    with open(filename, "w") as f:
        f.write("\t".join(group_dpsi_header_fields(thresholds)) + "\n")
        for row in rows:
            f.write(group_dpsi_line(*row, n_thresholds=len(thresholds)) + "\n")
            n += 1
    return n


# ---- the pooled table from the exact posteriors, `<A>_vs_<B>.miso_group_dpsi_exact` beside it ----
def group_dpsi_exact_header_fields(thresholds):
    return (GROUP_DPSI_HEAD + ["exact"] + DPSI_FIELDS + ["prob_abs_diff_ge_%g" % t for t in thresholds] + GROUP_DPSI_TAIL)


def group_dpsi_exact_line(event_name, n1, n2, result, header, thresholds):
    """n1, n2: the replicates of either group that were pooled (that have the event with exact = 1).  result = (mean1, mean2,
    quantiles at EXACT_DPSI_PROBS, H(0), cdf at delta_points(thresholds)) as capi.ExactGroupDelta.row returns it, or None (the
    event is not comparable): the replicate counts, exact = 0 and NA.  Otherwise exact = 1, the means, the median and bounds as
    %.4f, P(diff > 0) = 1 - H(0) and P(diff < 0) = H(0), and `.miso_bf_exact`'s P(|diff| >= t) = 1 - H(t) + H(-t).  header:
    whatever of isoforms, chrom, strand, mRNA_starts, mRNA_ends the caller knows."""
    f = [event_name, "%d" % n1, "%d" % n2]
    if result is None:
        f += ["NA"] * 3 + ["0"] + ["NA"] * (len(DPSI_FIELDS) + len(thresholds))
    else:
        m1, m2, q, h0, cdf = result
        f += ["%.4f" % m1, "%.4f" % m2, "%.4f" % (m1 - m2), "1"]
        f += ["%.4f" % q[0], "%.4f" % q[1], "%.4f" % q[2], "%.4f" % (1.0 - h0), "%.4f" % h0]
        f += exact_prob_fields(cdf, thresholds)
    f.append(header.get("isoforms", "NA"))
    for key in ("chrom", "strand", "mRNA_starts", "mRNA_ends"):
        f.append(header.get(key, "NA"))
    return "\t".join(f)


def write_group_dpsi_exact(filename, rows, thresholds):
    """rows: iterable of (event_name, n1, n2, result, header) -- group_dpsi_exact_line's arguments."""
    thresholds = check_delta_thresholds(thresholds)
    n = 0
    with open(filename, "w") as f:
        f.write("\t".join(group_dpsi_exact_header_fields(thresholds)) + "\n")
        for row in rows:
            f.write(group_dpsi_exact_line(*row, thresholds=thresholds) + "\n")
            n += 1
    return n


# ---- the statistics an exact posterior is made of, `<sample>.miso_exact_stats` ----
EXACT_STATS_FIELDS = ["event_name", "exact", "n10", "n01", "n", "e0", "e1", "h0", "h1"]


def write_exact_stats(filename, rows):
    """rows: iterable of (event_name, was_exact, stats7).  The statistics are printed with repr, so that they read back to
    the same doubles."""
    n = 0
    with open(filename, "w") as f:
        f.write("\t".join(EXACT_STATS_FIELDS) + "\n")
        for name, was, st in rows:
            f.write("\t".join([name, "1" if was else "0"] + [repr(float(v)) for v in st]) + "\n")
            n += 1
    return n


def read_exact_stats(filename):
    """{event_name: (was_exact, [7 floats])} of a `.miso_exact_stats` table, in the file's order"""
    out = {}
    with open(filename) as f:
        head = f.readline().rstrip("\n").split("\t")
        if head != EXACT_STATS_FIELDS:
            raise ValueError("Error: %s is no .miso_exact_stats table" % filename)
        for line in f:
            v = line.rstrip("\n").split("\t")
            if len(v) != len(EXACT_STATS_FIELDS):
                raise ValueError("Error: %s: malformed line %r" % (filename, line))
            out[v[0]] = (v[1] == "1", [float(x) for x in v[2:]])
    return out


# ---- what a paired-end exact posterior is made of, `<sample>.miso_exact_pairs` ----
EXACT_PAIRS_FIELDS = ["event_name", "exact", "n10", "n01", "A0", "A1", "h0", "h1", "n_pairs", "pair_probs", "pairs"]


def write_exact_pairs(filename, rows):
    """rows: iterable of (event_name, was_exact, stats6, m [n_pairs, 2]).  One header line; every row stands alone: the six
    statistics as repr, the number of drawing pairs, the event's distinct pair probabilities as repr in order of first use
    (comma-separated), and the pairs in record order as `i:j` index pairs into that list -- so the table reads back to the
    same doubles in the same order.  It grows with the drawing pairs, in the order of 10 bytes a pair."""
    n = 0
    with open(filename, "w") as f:
        f.write("\t".join(EXACT_PAIRS_FIELDS) + "\n")
        for name, was, st, m in rows:
            index, pairs = {}, []
            for m0, m1 in np.asarray(m, np.float64).reshape(-1, 2).tolist():
                pairs.append("%d:%d" % (index.setdefault(m0, len(index)), index.setdefault(m1, len(index))))
            f.write("\t".join([name, "1" if was else "0"] + [repr(float(v)) for v in st] +
                              [str(len(pairs)), ",".join(repr(v) for v in index) or "NA", ",".join(pairs) or "NA"]) + "\n")
            n += 1
    return n


def read_exact_pairs(filename):
    """{event_name: (was_exact, [6 floats], m [n_pairs, 2])} of a `.miso_exact_pairs` table, in the file's order"""
    out = {}
    with open(filename) as f:
        head = f.readline().rstrip("\n").split("\t")
        if head != EXACT_PAIRS_FIELDS:
            raise ValueError("Error: %s is no .miso_exact_pairs table" % filename)
        for line in f:
            v = line.rstrip("\n").split("\t")
            if len(v) != len(EXACT_PAIRS_FIELDS):
                raise ValueError("Error: %s: malformed line %r" % (filename, line))
            probs = np.array([float(x) for x in v[9].split(",")] if v[9] != "NA" else [], np.float64)
            idx = np.array([[int(i) for i in p.split(":")] for p in v[10].split(",")] if v[10] != "NA" else [], np.int64).reshape(-1, 2)
            if len(idx) != int(v[8]):
                raise ValueError("Error: %s: event %s has %d pairs, not %s" % (filename, v[0], len(idx), v[8]))
            out[v[0]] = (v[1] == "1", [float(x) for x in v[2:8]], probs[idx].reshape(-1, 2))
    return out
