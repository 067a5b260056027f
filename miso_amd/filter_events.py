"""misopy/filter_events.py for Python 3: `.miso_bf` tables -> the differentially spliced two-isoform events.

    python -m miso_amd.filter_events --filter F.miso_bf [F2.miso_bf ...] --output-dir D \\
        [--num-total N] [--num-inc N] [--num-exc N] [--num-sum-inc-exc N] [--delta-psi X] [--bayes-factor X] \\
        [--apply-both] [--votes V] [--votes-same-direction] [--control FILE ...]

Host only: the tables are tens of thousands of short rows (nothing here loads the device library).  The tables are what
`samples_utils --compare-samples` / `--compare-groups` write; with several of them (biological replicates) `--votes V`
keeps the events that pass in at least V.

Semantics, from the reference:

  row test (filter_events.py:241-327)   From `sampleN_counts` inc = the count of class (1,0), exc = (0,1), both = (1,1), 0
      where a class is absent, (0,0) ignored (:27-58).  A sample passes the count filter when inc + exc + both >=
      num_total, inc + exc >= num_sum, inc >= num_inc and exc >= num_exc (:61-81).  A row passes when |diff| >=
      |delta_psi|, |bayes_factor| >= |bayes_factor filter| and the count filter passes in at least one sample -- in both
      with --apply-both (:309-321).  Equality passes everywhere; every threshold defaults to 0; |delta_psi| > 1 is an
      error (:250-252).  A Bayes factor above 1e12 (`inf`) counts as 1e12 (:225-239).
  not two isoforms (:258-263)   the number of isoforms is the number of names in the `isoforms` field; such a row ends
      the run with the reference's message and exit status 1, before any output is written.
  one file (:109-116)   the passing rows go to D/<basename>.filtered; --votes is ignored.
  several files (:83-185)   each file is filtered on its own; an event is kept when it passes in at least V files
      (:132-136); each file's output holds its own passing rows of the kept events (:170-185).  The reference then
      counts, among an event's passing rows, those over the Bayes-factor threshold and the signed ones over the delta-psi
      threshold, and deletes the event when `not bf_pass and dp_pass` (:138-168).  Every passing row already meets both
      thresholds, so with at least V passing rows bf_pass is true whenever the step is reached: it can never remove an
      event, and is not restated here.  V = 0 keeps every passing row.
  --control   parsed and unused in the reference (:354, :402-417): accepted, and reported as ignored.
  summary line per file (:336-339)   `%d/%d events pass the filter (%.2f percent).`

New, opt-in: --votes-same-direction keeps an event only when at least V of its passing rows have the same sign of `diff`
(a zero diff counts for neither sign) -- what the reference's comment at :138 says it meant to test.

Deliberate deviations:
  1. rows are written VERBATIM: the header line and each kept line byte for byte, in input order.  The reference passes
     every field through eval and csv.DictWriter (parse_csv.py): `0.50` becomes `0.5`, the isoform list a tuple's repr.
  2. two inputs with the same base name are an error, not a silent overwrite of one `.filtered` by the other.
  3. an empty table reports `0/0 events pass the filter (0.00 percent).` where the reference divides by zero.
"""
import os
import re
import sys

MAX_BF = 1e12                       # filter_events.py:231
NOT_TWO_ISOFORMS = ("Error: filter_events.py is only defined for MISO output on two-isoform alternative events. "
                    "Found a non-two isoform event: %s")


class NotTwoIsoforms(Exception):
    """A row of an event without exactly two isoforms (filter_events.py:258-263)."""


def get_counts(counts_str):
    """filter_events.py:27-58: (inc, exc, both) of a `(1,0):n,(0,1):m,...` field."""
    inc = exc = both = 0
    for cls, n in re.findall(r"(\([01],[01]\)):(\d+)", counts_str):
        if cls == "(1,0)":
            inc = int(n)
        elif cls == "(0,1)":
            exc = int(n)
        elif cls == "(1,1)":
            both = int(n)
    return inc, exc, both


def counts_pass(counts, num_total, num_inc, num_exc, num_sum):
    """filter_events.py:61-81."""
    inc, exc, both = counts
    return inc + exc + both >= num_total and inc + exc >= num_sum and inc >= num_inc and exc >= num_exc


def num_isoforms(field):
    """Names in the `isoforms` field: quoted names ('a','b') as the `.miso` header has them, else comma separated."""
    quoted = re.findall(r"'[^']*'|\"[^\"]*\"", field)
    return len(quoted) if quoted else len([x for x in field.split(",") if x.strip()])


def _bayes_factor(field):
    """filter_events.py:225-239, 291: the first value, at most 1e12."""
    return min(float(field.split(",")[0]), MAX_BF)


class Table:
    """One `.miso_bf` file as read: `header` and `lines` as bytes (with their line ends), `fields` per line."""

    def __init__(self, path):
        self.path = path
        with open(path, "rb") as f:
            data = f.read().splitlines(keepends=True)
        self.header = data[0] if data else b""
        self.lines = [ln for ln in data[1:] if ln.strip()]
        names = self.header.decode().rstrip("\r\n").split("\t")
        self.col = {n: i for i, n in enumerate(names)}
        need = ("event_name", "diff", "bayes_factor", "isoforms", "sample1_counts", "sample2_counts")
        missing = [n for n in need if n not in self.col]
        if self.lines and missing:
            raise ValueError("%s: no column %s" % (path, ", ".join(missing)))
        self.fields = [ln.decode().rstrip("\r\n").split("\t") for ln in self.lines]

    def get(self, row, name):
        return self.fields[row][self.col[name]]


def filter_rows(table, num_total=0, num_inc=0, num_exc=0, num_sum=0, delta_psi=0.0, bayes_factor=0.0, apply_both=False):
    """filter_events.py:241-327: indices of the table's rows that pass."""
    if abs(delta_psi) > 1:
        raise ValueError("Error: delta psi value outside [0, 1].")
    keep = []
    for r in range(len(table.lines)):
        if num_isoforms(table.get(r, "isoforms")) != 2:
            raise NotTwoIsoforms(NOT_TWO_ISOFORMS % table.get(r, "event_name"))
        if abs(float(table.get(r, "diff").split(",")[0])) < abs(delta_psi):
            continue
        if abs(_bayes_factor(table.get(r, "bayes_factor"))) < abs(bayes_factor):
            continue
        ok = [counts_pass(get_counts(table.get(r, "sample%d_counts" % s)), num_total, num_inc, num_exc, num_sum) for s in (1, 2)]
        if (all(ok) if apply_both else any(ok)):
            keep.append(r)
    return keep


def vote(tables, passing, votes, same_direction=False):
    """filter_events.py:122-136: names of the events that pass in at least `votes` of the tables; same_direction: with
    at least `votes` passing rows of one sign of `diff`."""
    n_pass, n_pos, n_neg = {}, {}, {}
    for t, keep in zip(tables, passing):
        for r in keep:
            name = t.get(r, "event_name")
            d = float(t.get(r, "diff").split(",")[0])
            n_pass[name] = n_pass.get(name, 0) + 1
            n_pos[name] = n_pos.get(name, 0) + (d > 0)
            n_neg[name] = n_neg.get(name, 0) + (d < 0)
    kept = {n for n, c in n_pass.items() if c >= votes}
    if same_direction:
        kept = {n for n in kept if max(n_pos[n], n_neg[n]) >= votes}
    return kept


def multi_filter(filter_filenames, output_dir, num_total=0, num_inc=0, num_exc=0, num_sum=0, delta_psi_filter=0.0,
                 bf_filter=0.0, vote_thresh=0, apply_both_samples=False, votes_same_direction=False, out=None):
    """filter_events.py:83-185.  Returns [(output filename, rows kept, rows read)], one per input."""
    out = out or sys.stdout
    filter_filenames = list(filter_filenames)
    if not filter_filenames:
        raise ValueError("Need at least one filename to filter (use --filter.)")
    bases = [os.path.basename(f) for f in filter_filenames]
    twice = sorted({b for b in bases if bases.count(b) > 1})
    if twice:
        raise ValueError("two inputs named %s would write the same .filtered file" % ", ".join(twice))
    if abs(delta_psi_filter) > 1:
        raise ValueError("Error: delta psi value outside [0, 1].")
    tables = [Table(f) for f in filter_filenames]
    passing = [filter_rows(t, num_total, num_inc, num_exc, num_sum, delta_psi_filter, bf_filter, apply_both_samples)
               for t in tables]
    if len(tables) > 1:
        kept = vote(tables, passing, vote_thresh, votes_same_direction)
        passing = [[r for r in keep if t.get(r, "event_name") in kept] for t, keep in zip(tables, passing)]
    os.makedirs(output_dir, exist_ok=True)
    done = []
    for t, keep, base in zip(tables, passing, bases):
        fname = os.path.join(output_dir, base + ".filtered")
        print("Filtering %s into %s" % (t.path, fname), file=out)
        with open(fname, "wb") as f:
            f.write(t.header)
            for r in keep:
                f.write(t.lines[r])
        total = len(t.lines)
        print("%d/%d events pass the filter (%.2f percent)." % (len(keep), total, 100.0 * len(keep) / total if total else 0.0),
              file=out)
        done.append((fname, len(keep), total))
    return done


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="filter_events: filtering MISO pairwise comparison output "
                                             "(two-isoform event annotations only)")
    ap.add_argument("--filter", dest="filter_filename", nargs="+", default=None,
                    help="Comparison file to filter or list of replicate files to filter.")
    ap.add_argument("--control", dest="control_filename", nargs="*", default=[],
                    help="Accepted and ignored, as in the reference.")
    ap.add_argument("--output-dir", dest="output_dir", default=None)
    ap.add_argument("--num-total", type=int, default=0)
    ap.add_argument("--num-inc", type=int, default=0)
    ap.add_argument("--num-exc", type=int, default=0)
    ap.add_argument("--num-sum-inc-exc", dest="num_sum", type=int, default=0)
    ap.add_argument("--delta-psi", type=float, default=0.0)
    ap.add_argument("--bayes-factor", type=float, default=0.0)
    ap.add_argument("--apply-both", action="store_true")
    ap.add_argument("--votes", dest="vote_thresh", type=int, default=0,
                    help="Replicate files in which an event must pass the filters.")
    ap.add_argument("--votes-same-direction", action="store_true",
                    help="... with the same sign of the difference in that many of them.")
    a = ap.parse_args(argv)
    if a.filter_filename is None:
        ap.error("Need at least one filename to filter (use --filter.)")
    if a.output_dir is None:
        ap.error("Need an output directory to output filtered file to (use --output-dir)")
    if a.control_filename:
        print("--control is ignored (as in the reference): %s" % ", ".join(a.control_filename))
    files = [os.path.abspath(os.path.expanduser(f)) for f in a.filter_filename]
    try:
        multi_filter(files, os.path.abspath(os.path.expanduser(a.output_dir)), a.num_total, a.num_inc, a.num_exc, a.num_sum,
                     a.delta_psi, a.bayes_factor, a.vote_thresh, apply_both_samples=a.apply_both,
                     votes_same_direction=a.votes_same_direction)
    except NotTwoIsoforms as err:
        print(err)
        return 1
    except ValueError as err:
        print(err, file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
