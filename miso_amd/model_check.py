"""The `.miso_fit` table: the posterior predictive model check of single-end events (capi.Batch.model_check).

One row per event: do the event's reads fall into the gene's read classes the way the model behind psi says?
fit_pvalue is a posterior predictive p-value of the Freeman-Tukey discrepancy: conservative (under the model it
concentrates towards 1/2, it is not uniform), small when the class counts do not look like the model's -- 3' bias, a
mis-annotated exon, a repeat that swallowed one junction's reads.  tail_ge / tail_le say which class is short or in excess:
the fraction of replicates with at least / at most the observed count.  An event whose check did not run (status other
than ok: no gene structure, no reads, more than 64 classes or isoforms, no usable row) has NA in every column but its name."""

HEADER_FIELDS = ["event_name", "num_reads", "num_off_model", "num_classes", "num_rows", "fit_pvalue", "mean_disc_obs",
                 "mean_disc_rep", "observed", "expected", "tail_ge", "tail_le"]
NA = "NA"


def class_key(pattern, num_isoforms):
    """(1,0,...) of a class's set of isoforms: the `.miso` header's spelling of a read class"""
    return "(" + ",".join("1" if (int(pattern) >> k) & 1 else "0" for k in range(num_isoforms)) + ")"


def _keyed(keys, values, fmt):
    return ",".join("%s:%s" % (k, fmt % v) for k, v in zip(keys, values))


def model_fit_line(event_name, fit, num_isoforms):
    """One table row.  fit: a capi.ModelFit (or anything with its attributes)."""
    if fit.status != "ok":
        return "\t".join([event_name] + [NA] * (len(HEADER_FIELDS) - 1))
    head = [event_name, "%d" % fit.num_reads, "%d" % fit.num_off_model, "%d" % len(fit.pattern)]
    keys = [class_key(p, num_isoforms) for p in fit.pattern]
    rows = float(fit.rows)
    return "\t".join(head + [
        "%d" % fit.rows, "%.4f" % (fit.exceed / rows), "%.4f" % (fit.sum_obs / rows), "%.4f" % (fit.sum_rep / rows),
        _keyed(keys, [int(x) for x in fit.n], "%d"), _keyed(keys, [float(x) for x in fit.expected], "%.1f"),
        _keyed(keys, [int(x) / rows for x in fit.ge], "%.4f"), _keyed(keys, [int(x) / rows for x in fit.le], "%.4f")])


def write_model_fit(filename, rows):
    """rows: iterable of (event_name, fit, num_isoforms).  Returns the number of rows written."""
    n = 0
    with open(filename, "w") as f:
        f.write("\t".join(HEADER_FIELDS) + "\n")
        for name, fit, num_isoforms in rows:
            f.write(model_fit_line(name, fit, num_isoforms) + "\n")
            n += 1
    return n
