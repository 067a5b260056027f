"""Part-level psi: how often a part (an exon) of a gene is included, and how that differs between two samples.

An isoform-centric run gives one psi per isoform.  The inclusion of a part is the sum of the psi of the isoforms that hold
it; its posterior mean follows from the summary, its credible interval and every statement about its delta psi need the
joint draws.  They are taken where the draws are, by the isoform-group passes of the device
(capi.Batch.summarize_isoform_groups, capi.compare_pairs_isoform_groups): a group is an event and the set of its isoforms
that hold the part.  No reference counterpart.

    <X>.miso_part_summary           one row per (event, part): mean and credible interval of the part's inclusion
    <l1>_vs_<l2>.miso_part_dpsi     the same of either sample, then `.miso_dpsi`'s statistics of the difference

Rows come in event-name order, then part order (a run's merged parts are sorted: sort_table).  Parts are distinct by (start, end); a part every isoform holds, or none, has
nothing to estimate and gives no row; an event with one isoform, or with more than 64 (the width of a mask), gives none.

During a run: `miso --run INDEX BAM --output-dir OUT --read-len L --part-psi [--compare BAM2]` (miso.py; the workers get
run_miso --part-psi-file F / --part-psi-files F1 F2 FD).  Over existing trees (`.miso`, `.miso_db` or both):

    python -m miso_amd.samples_utils --summarize-parts SAMPLES_DIR INDEX_DIR OUT_DIR
    python -m miso_amd.samples_utils --compare-parts DIR1 DIR2 INDEX_DIR OUT_DIR [--comparison-labels A B]
                                                                                 [--delta-psi-thresholds T ...]

Not built: junction-level groups, pooling over replicate groups, Bayes factors per part; the mask interface carries them.
"""
import os
import sys
from collections import namedtuple

from . import capi, compare, gene_utils, gff_utils

MAX_MASK_ISOFORMS = 64

PartGroup = namedtuple("PartGroup", "label start end mask isoforms")

SUMMARY_HEAD = ["event_name", "part", "part_coords", "isoforms_with_part", "num_isoforms"]
SUMMARY_FIELDS = SUMMARY_HEAD + ["miso_posterior_mean", "ci_low", "ci_high"]
DPSI_SAMPLE_FIELDS = ["sample1_posterior_mean", "sample1_ci_low", "sample1_ci_high",
                      "sample2_posterior_mean", "sample2_ci_low", "sample2_ci_high"]


def gene_part_groups(gene_obj):
    """One PartGroup per distinct part of the gene that some isoforms hold and some do not, in the order of `gene_obj.parts`:
    parts are distinct by (start, end), the label is that of the first part with those coordinates; `isoforms` the indices
    of the isoforms that hold a part with those coordinates, `mask` the same as a set of bits.  A gene of more than 64
    isoforms has no masks: ValueError."""
    isoforms = gene_obj.isoforms
    if len(isoforms) > MAX_MASK_ISOFORMS:
        raise ValueError("%d isoforms: an isoform mask holds %d at most" % (len(isoforms), MAX_MASK_ISOFORMS))
    held = [{(p.start, p.end) for p in iso.parts} for iso in isoforms]
    seen, out = set(), []
    for part in gene_obj.parts:
        at = (part.start, part.end)
        if at in seen:
            continue
        seen.add(at)
        ks = [k for k, h in enumerate(held) if at in h]
        if 0 < len(ks) < len(isoforms):
            out.append(PartGroup(part.label, part.start, part.end, sum(1 << k for k in ks), ks))
    return out


class _Skipped:
    """events that give no rows for a reason worth a line on stderr, each kind named once"""

    def __init__(self):
        self.said = set()

    def say(self, kind, text):
        if kind not in self.said:
            self.said.add(kind)
            print(text, file=sys.stderr)


_PROCESS_SKIPPED = _Skipped()      # a run's launches share it: one notice per kind and process, not one per launch


def event_groups(genes, skipped=None):
    """genes[i]: event i's gene object, or None for an event to leave out.  -> (groups, places): the distinct (event, mask)
    pairs for the device, every mask of an event once, and places[i] = [(PartGroup, index into groups)] of event i.
    skipped: who names the events that give no rows (default: the process's, which says each kind once)."""
    skipped = skipped or _PROCESS_SKIPPED
    groups, places = [], []
    for i, gene in enumerate(genes):
        mine = []
        if gene is not None and len(gene.isoforms) > MAX_MASK_ISOFORMS:
            skipped.say("wide", "No part-level psi for events of more than %d isoforms (%s has %d)"
                        % (MAX_MASK_ISOFORMS, getattr(gene, "label", "event %d" % i), len(gene.isoforms)))
        elif gene is not None and len(gene.isoforms) > 1:
            at = {}
            for pg in gene_part_groups(gene):
                if pg.mask not in at:
                    at[pg.mask] = len(groups)
                    groups.append((i, pg.mask))
                mine.append((pg, at[pg.mask]))
        places.append(mine)
    return groups, places


def _head(name, gene, pg):
    return [name, str(pg.label), "%s:%d-%d:%s" % (getattr(gene, "chrom", None) or "NA", pg.start, pg.end,
                                                   getattr(gene, "strand", None) or "NA"),
            ",".join(str(k) for k in pg.isoforms), str(len(gene.isoforms))]


def summary_rows(batch, names, genes, confidence_level=0.95, as_text=True, skipped=None):
    """`.miso_part_summary` rows of a batch's events: (head fields, (mean, ci_low, ci_high))."""
    groups, places = event_groups(genes, skipped)
    if not groups:
        return []
    got = batch.summarize_isoform_groups(groups, confidence_level, as_text=as_text)
    return [(_head(names[i], genes[i], pg), got.summary(g)) for i, mine in enumerate(places) for pg, g in mine]


def dpsi_rows(batch1, batch2, names, genes, confidence_level=0.95, thresholds=compare.DEFAULT_DELTA_THRESHOLDS, as_text=True,
              skipped=None):
    """`.miso_part_dpsi` rows of two batches' events: (head fields, summary 1, summary 2, pair comparison)."""
    groups, places = event_groups(genes, skipped)
    if not groups:
        return []
    s1 = batch1.summarize_isoform_groups(groups, confidence_level, as_text=as_text)
    s2 = batch2.summarize_isoform_groups(groups, confidence_level, as_text=as_text)
    d = capi.compare_pairs_isoform_groups(batch1, batch2, groups, confidence_level, thresholds, as_text=as_text)
    return [(_head(names[i], genes[i], pg), s1.summary(g), s2.summary(g), d.pair_comparison(g))
            for i, mine in enumerate(places) for pg, g in mine]


def _three(summary):
    """mean and bounds as summary.py formats them; a group that is not finite prints NA"""
    return ["%.2f" % v if v == v else "NA" for v in summary]


def _dpsi_fields(pairs, n_thresholds):
    """the statistics columns of `.miso_dpsi` for one column (compare.dpsi_fields' formatting)"""
    med, lo, hi, gt, lt, ge, fin, M = pairs
    if not fin:
        return ["NA"] * (len(compare.DPSI_FIELDS) + n_thresholds)
    M = float(M)
    return ["%.4f" % v for v in [med, lo, hi, gt / M, lt / M] + [ge[j] / M for j in range(n_thresholds)]]


def write_part_summary(filename, rows):
    """rows: summary_rows' tuples, in the order they are to stand"""
    os.makedirs(os.path.dirname(os.path.abspath(filename)), exist_ok=True)
    with open(filename, "w") as f:
        f.write("\t".join(SUMMARY_FIELDS) + "\n")
        for head, summ in rows:
            f.write("\t".join(head + _three(summ)) + "\n")
    return len(rows)


def sort_table(filename):
    """The table's rows in event-name order, an event's rows in the order they stand (its part order): the one order of a
    run's merged per-launch and per-worker parts and of the tables over existing trees."""
    with open(filename) as f:
        lines = f.readlines()
    rows = sorted(lines[1:], key=lambda line: line.split("\t", 1)[0])       # (stable)
    with open(filename, "w") as f:
        f.writelines(lines[:1] + rows)
    return filename


def samples_refusal(num_samples, confidence_level=0.95):
    """Why the isoform-group passes would refuse columns of num_samples draws, or None: what a run checks before it samples"""
    from . import summary
    if num_samples > capi.MAX_ISOFORM_GROUP_DRAWS:
        return ("part-level psi takes %d samples per event at most, the sampler settings give %d"
                % (capi.MAX_ISOFORM_GROUP_DRAWS, num_samples))
    lo, hi = summary.credible_interval_ranks(num_samples, confidence_level)
    if not (lo > 0 and hi > 0 and hi < num_samples):
        return "part-level psi needs more samples for a credible interval than the sampler settings' %d" % num_samples
    return None


def dpsi_header_fields(thresholds):
    return SUMMARY_HEAD + DPSI_SAMPLE_FIELDS + compare.DPSI_FIELDS + ["prob_abs_diff_ge_%g" % t for t in thresholds]


def write_part_dpsi(filename, rows, thresholds):
    """rows: dpsi_rows' tuples, in the order they are to stand"""
    thresholds = compare.check_delta_thresholds(thresholds)
    os.makedirs(os.path.dirname(os.path.abspath(filename)), exist_ok=True)
    with open(filename, "w") as f:
        f.write("\t".join(dpsi_header_fields(thresholds)) + "\n")
        for head, s1, s2, pairs in rows:
            f.write("\t".join(head + _three(s1) + _three(s2) + _dpsi_fields(pairs, len(thresholds))) + "\n")
    return len(rows)


# ---- existing trees: the gene objects come from the index, the samples from the `.miso` files / `.miso_db` rows
class IndexGenes:
    """event name -> gene object from an index directory (index_gff.py): the one-file bundle where there is one, the
    per-gene pickles otherwise.  An event's name is its index file's base name."""

    def __init__(self, index_dir):
        self.by_event = {}
        for gene_id, path in gff_utils.get_gene_ids_to_gff_index(index_dir).items():
            self.by_event[os.path.basename(path)[:-len(".pickle")]] = (gene_id, path)
        bpath = os.path.join(index_dir, gff_utils.BUNDLE_BASENAME)
        self.bundle = gff_utils.load_indexed_gff_file(bpath) if os.path.isfile(bpath) else {}
        self.missing = []

    def gene(self, event_name):
        if event_name not in self.by_event:
            self.missing.append(event_name)
            return None
        gene_id, path = self.by_event[event_name]
        if gene_id in self.bundle:
            return gene_utils.gene_from_compact(self.bundle[gene_id])[0]
        return gff_utils.load_indexed_gff_file(path)[gene_id]["gene_object"]

    def report(self):
        if self.missing:
            print("Not in the index, skipped: %s" % ", ".join(sorted(set(self.missing))))


def _tree_batches(sources, names, device, decoder):
    """The named events of one or two trees as device batches, read and decoded as --summarize-samples does: yields
    (names of the batch's usable events, their indices in the batches, one batch per tree).  Events are grouped by their
    sample counts; one that a tree lacks, that does not parse, or whose isoform counts differ between the trees drops out."""
    from . import samples_utils as su
    stats = su._Stats(decoder)
    left = list(names)
    if decoder == "device":
        sides = []
        for src in sources:
            evs = su._read_events(*su._read_named(src, names))
            su._shape(evs)
            sides.append({e.name: e for e in evs})
        left, runs = [], {}
        for n in names:
            evs = [side.get(n) for side in sides]
            if any(e is None for e in evs):
                continue
            if all(su._device_ok(e) for e in evs) and len({e.K for e in evs}) == 1:
                runs.setdefault(tuple(e.S for e in evs), []).append(evs)
            else:
                left.append(n)
        for Ss, group in sorted(runs.items()):
            for run in su._text_batches(group, lambda evs: sum(len(e.body) for e in evs)):
                batches = [su._text_batch([evs[s] for evs in run], Ss[s], device, stats) for s in range(len(sources))]
                ok = [i for i in range(len(run)) if not any(b.status[i] for b in batches)]
                left += [run[i][0].name for i in range(len(run)) if i not in ok]
                yield [run[i][0].name for i in ok], ok, batches
    parsed = []
    for src in sources:
        have = [n for n in left if n in src]
        files, dbrows = su._read_named(src, have)
        parsed.append({e[0]: e for e in su._load_all(files + su._read_events([], dbrows))})
    runs = {}
    for n in sorted(left):
        evs = [side.get(n) for side in parsed]
        if any(e is None for e in evs) or len({e[1].shape[1] for e in evs}) != 1:
            continue
        runs.setdefault(tuple(e[1].shape[0] for e in evs), []).append(evs)
    for Ss, group in sorted(runs.items()):
        batches = [capi.SamplesBatch([evs[s][1] for evs in group], device=device) for s in range(len(sources))]
        yield [evs[0][0] for evs in group], list(range(len(group))), batches


def _placed(names, idx, n_events, index):
    """the batch's events as event_groups takes them: a gene where the event is usable and in the index"""
    genes, labels = [None] * n_events, [None] * n_events
    for name, i in zip(names, idx):
        genes[i], labels[i] = index.gene(name), name
    return labels, genes


def _level_ok(S, confidence_level):
    from . import summary
    return summary.credible_interval_ranks(S, confidence_level)[0] > 0 and S <= capi.MAX_ISOFORM_GROUP_DRAWS


def summarize_parts(samples_dir, index_dir, output_dir, confidence_level=0.95, device=0, decoder=None):
    """`--summarize-parts`: OUT_DIR/summary/<SAMPLES_DIR>.miso_part_summary of every event of the tree that the index knows."""
    from . import samples_utils as su
    index, skipped, by_event = IndexGenes(index_dir), _Skipped(), {}
    src = su._sources(samples_dir)
    for names, idx, (b,) in _tree_batches([src], sorted(src), device, su._decoder(decoder)):
        if not _level_ok(b.params.noIterations, confidence_level):
            print("Skipping %d events with %d samples" % (len(names), b.params.noIterations))
            continue
        labels, genes = _placed(names, idx, len(b), index)
        for row in summary_rows(b, labels, genes, confidence_level, as_text=False, skipped=skipped):
            by_event.setdefault(row[0][0], []).append(row)
    index.report()
    out = os.path.join(output_dir, "summary", os.path.basename(os.path.normpath(samples_dir)) + ".miso_part_summary")
    return out, write_part_summary(out, [r for n in sorted(by_event) for r in by_event[n]])


def compare_parts(sample1_dir, sample2_dir, index_dir, output_dir, confidence_level=0.95, sample_labels=None,
                  delta_thresholds=None, device=0, decoder=None):
    """`--compare-parts`: OUT_DIR/<l1>_vs_<l2>/bayes-factors/<l1>_vs_<l2>.miso_part_dpsi of the events both trees hold."""
    from . import samples_utils as su
    thresholds = compare.check_delta_thresholds(delta_thresholds or compare.DEFAULT_DELTA_THRESHOLDS)
    index, skipped, by_event = IndexGenes(index_dir), _Skipped(), {}
    l1, l2 = sample_labels or (os.path.basename(os.path.normpath(sample1_dir)), os.path.basename(os.path.normpath(sample2_dir)))
    f1, f2 = su._sources(sample1_dir), su._sources(sample2_dir)
    for names, idx, (b1, b2) in _tree_batches([f1, f2], sorted(set(f1) & set(f2)), device, su._decoder(decoder)):
        if not (_level_ok(b1.params.noIterations, confidence_level) and _level_ok(b2.params.noIterations, confidence_level)):
            print("Skipping %d events with %d and %d samples" % (len(names), b1.params.noIterations, b2.params.noIterations))
            continue
        labels, genes = _placed(names, idx, len(b1), index)
        for row in dpsi_rows(b1, b2, labels, genes, confidence_level, thresholds, as_text=False, skipped=skipped):
            by_event.setdefault(row[0][0], []).append(row)
    index.report()
    name = "%s_vs_%s" % (l1, l2)
    out = os.path.join(output_dir, name, "bayes-factors", name + ".miso_part_dpsi")
    return out, write_part_dpsi(out, [r for n in sorted(by_event) for r in by_event[n]], thresholds)
