"""Chain diagnostics of sampled events -- the table `<label>.miso_diag`, fed from the numbers the device computes
(`miso_batch_diagnose`, csrc/kernels_diagnose.hip): per event and isoform the split R-hat of its chains,
the effective sample size and Monte-Carlo standard error of the psi mean, and the lag at which Geyer's initial monotone
sequence was cut.  No reference counterpart: the reference reports none of these.

One row per event, in the order of the summary table (summary.py), tab-separated:

    event_name  rhat  ess  mcse  lag  num_samples  num_chains

Two-isoform events print the first isoform's scalars, more isoforms comma lists, as summary.format_credible_intervals
does.  A degenerate column (constant, or holding a NaN or an infinity) prints `nan` and lag 0.
"""
import math

HEADER_FIELDS = ["event_name", "rhat", "ess", "mcse", "lag", "num_samples", "num_chains"]


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


def write_diagnostics(filename, rows):
    """rows: iterable of (event_name, rhat, ess, mcse, lag, num_samples, num_chains)."""
    n = 0
    with open(filename, "w") as f:
        f.write("\t".join(HEADER_FIELDS) + "\n")
        for row in rows:
            f.write(diagnostics_line(*row) + "\n")
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
