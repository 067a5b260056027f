"""Chain diagnostics of sampled events -- the table `<label>.miso_diag`, fed from the numbers the device computes
(`miso_batch_diagnose`, csrc/kernels_diagnose.hip): per event and isoform the split R-hat of its chains,
the effective sample size and Monte-Carlo standard error of the psi mean, and the lag at which Geyer's initial monotone
sequence was cut.  No reference counterpart: the reference reports none of these.

One row per event, in the order of the summary table (summary.py), tab-separated:

    event_name  rhat  ess  mcse  lag  num_samples  num_chains

Two-isoform events print the first isoform's scalars, more isoforms comma lists, as summary.format_credible_intervals
does.  A degenerate column (constant, or holding a NaN or an infinity) prints `nan` and lag 0.

With rank=True (`--rank-diagnostics`) six more columns follow, from the rank-normalised pass (`miso_batch_diagnose_rank`,
csrc/kernels_diagnose_rank.hip), at the 95 % interval the summary prints:

    rhat_rank  ess_bulk  ess_tail  ess_ci_low  ess_ci_high  num_distinct

rhat_rank is the larger of the bulk and the folded R-hat, ess_tail the smaller of the two bounds' effective sample
sizes, each `nan` if either is.  An event whose group of events the rank pass refused prints `nan` in all six.
"""
import math

HEADER_FIELDS = ["event_name", "rhat", "ess", "mcse", "lag", "num_samples", "num_chains"]
RANK_FIELDS = ["rhat_rank", "ess_bulk", "ess_tail", "ess_ci_low", "ess_ci_high", "num_distinct"]
RANK_CONFIDENCE_LEVEL = 0.95


def _fmt(fmt, v):
    return "nan" if math.isnan(v) else fmt % v


def format_diagnostics(event_name, rhat, ess, mcse, lag):
    """Two isoforms -> the first isoform's scalars, more -> comma lists."""
    cols = ((rhat, "%.3f"), (ess, "%.1f"), (mcse, "%.4f"))
    if len(rhat) > 2:
        return [event_name] + [",".join(_fmt(f, float(v)) for v in col) for col, f in cols] \
            + [",".join("%d" % int(v) for v in lag)]
    return [event_name] + [_fmt(f, float(col[0])) for col, f in cols] + ["%d" % int(lag[0])]


def diagnostics_line(event_name, rhat, ess, mcse, lag, num_samples, num_chains):
    return "\t".join(format_diagnostics(event_name, rhat, ess, mcse, lag) + ["%d" % num_samples, "%d" % num_chains])


def _worse(a, b, pick):
    """pick(a, b), or NaN if either is."""
    return math.nan if math.isnan(a) or math.isnan(b) else pick(a, b)


def format_rank_diagnostics(rank):
    """The six rank columns of one event from (rhat_bulk, rhat_fold, ess_bulk, ess_ci_low, ess_ci_high, distinct), arrays
    over its isoforms; None (the pass refused the event's group): `nan` six times."""
    if rank is None:
        return ["nan"] * 6
    rb, rf, eb, lo, hi, distinct = rank
    K = len(rb)
    cols = (([_worse(float(rb[k]), float(rf[k]), max) for k in range(K)], "%.3f"), (eb, "%.1f"),
            ([_worse(float(lo[k]), float(hi[k]), min) for k in range(K)], "%.1f"), (lo, "%.1f"), (hi, "%.1f"))
    if K > 2:
        return [",".join(_fmt(f, float(v)) for v in col) for col, f in cols] + [",".join("%d" % int(v) for v in distinct)]
    return [_fmt(f, float(col[0])) for col, f in cols] + ["%d" % int(distinct[0])]


def rank_notice(what, error):
    """The one line printed when the rank pass refuses a group of events: too many draws or chains for the device's
    sort, or too few draws for the interval."""
    return "NOTICE: no rank diagnostics for %s: %s" % (what, error)


def write_diagnostics(filename, rows, rank=False):
    """rows: iterable of (event_name, rhat, ess, mcse, lag, num_samples, num_chains); with rank=True an eighth element,
    format_rank_diagnostics' argument."""
    n = 0
    with open(filename, "w") as f:
        f.write("\t".join(HEADER_FIELDS + (RANK_FIELDS if rank else [])) + "\n")
        for row in rows:
            line = diagnostics_line(*row[:7])
            if rank:
                line += "\t" + "\t".join(format_rank_diagnostics(row[7]))
            f.write(line + "\n")
            n += 1
    return n


def header_mismatch(event_name, header, num_rows, num_chains):
    """The warning line for an event whose `.miso` header (dict with iters, burn_in, lag) does not give
    num_chains * ((iters - burn_in) div lag) = num_rows sample rows, or None.  A header without those fields says
    nothing either way."""
    try:
        iters, burn_in, lag = int(header["iters"]), int(header["burn_in"]), int(header["lag"])
        expect = num_chains * ((iters - burn_in) // lag)
    except (KeyError, ValueError, ZeroDivisionError):
        return None
    if expect == num_rows:
        return None
    return ("WARNING: %s: the header gives %d chains x ((%d - %d) div %d) = %d samples, the file has %d rows; "
            "diagnosed as %d chains" % (event_name, num_chains, iters, burn_in, lag, expect, num_rows, num_chains))
