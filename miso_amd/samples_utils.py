"""misopy/samples_utils.py (`summarize_miso --summarize-samples`) and misopy/hypothesis_test.py
(`compare_miso --compare-samples`) over EXISTING MISO output, for Python 3 and the GPU.

    python -m miso_amd.samples_utils --summarize-samples SAMPLES_DIR OUTPUT_DIR
    python -m miso_amd.samples_utils --compare-samples SAMPLES_DIR1 SAMPLES_DIR2 OUTPUT_DIR
    python -m miso_amd.samples_utils --diagnose-samples SAMPLES_DIR OUTPUT_DIR [--num-chains C]
    python -m miso_amd.samples_utils --compare-groups DIR[,DIR...] DIR[,DIR...] OUTPUT_DIR [--group-labels L[,L...] L[,L...]]
    python -m miso_amd.samples_utils --summarize-parts SAMPLES_DIR INDEX_DIR OUTPUT_DIR
    python -m miso_amd.samples_utils --compare-parts SAMPLES_DIR1 SAMPLES_DIR2 INDEX_DIR OUTPUT_DIR

The reference walks the samples directory (chromosome sub-directories of `<event>.miso`, or their packed form
`<chrom>.miso_db`, samples_utils.py:263-411), parses every event's "%.4f" rows and computes per event the posterior
mean and Chen-Shao interval (credible_intervals.py:4-72); compare_miso pairs the events present in both directories and
adds the Savage-Dickey Bayes factor (hypothesis_test.py:89-179, 186-345).  Here the directory's content decides what is
read: `.miso` files, `.miso_db` databases (miso_amd/miso_pack.py, miso_amd/miso_db.py) or both, each event once (a
file beats a row of the same name).  The numbers come from the same device kernels that serve a live run
(summarize_kernel, compare_kernel); the samples get to the device in one of two ways, MISO_TEXT_DECODE=device|host or
the `decoder` argument:

  device  the events' text is uploaded as it is and decoded by text_decode_kernel straight into the samples pool
          (capi.SamplesBatch.from_text).  An event outside the decoder's grammar (an exponent, `nan` as a value, a
          ragged row; include/miso_amd.h) is reported by its status and goes through the host parser in a batch of its
          own; `last_decode_stats` says how many did.
  host    every event is parsed on the host cores (numpy, a thread per core) and copied to the device
          (capi.SamplesBatch).

Both give the same doubles for the same text -- the correctly rounded value of every decimal -- so the tables are
byte-identical (tests/test_gpu_miso_text.py), and equal to the reference's on the same files (bounds bit for bit; see
tests/test_gpu_summary.py, tests/test_gpu_compare.py).  Out of scope as in the reference's own optional paths:
compressed-ID maps (`--use-compressed`), zipped outputs (miso_zip).

`--diagnose-samples` has no reference counterpart: the chain diagnostics (split R-hat, effective sample size, Monte-Carlo
standard error; diagnostics.py) of the files' four-decimal values, through the same readers and decoders.

`--compare-groups` is `--compare-samples` for biological replicates (what filter_events --votes reads): every pair of the
two groups gets the file the pairwise call writes, byte for byte, but every tree is read once, every sample decoded and
summarised once per chunk of events, and all pairs of a chunk come out of one launch (capi.compare_groups).
With `--exact-delta-posterior` the two groups also get `<A>_vs_<B>.miso_group_dpsi_exact`: delta psi pooled over all pairs of
replicates from their exact posteriors, without a draw, from each directory's `summary/<name>.miso_exact_stats`.
`--exact-paired-delta-posterior` is the same for paired-end replicates, from `summary/<name>.miso_exact_pairs`.
With `--delta-posterior` every pair also gets its `.miso_dpsi`, and the two groups one pooled table, `.miso_group_dpsi`: delta
psi over all differences between the pooled draws of the groups (capi.compare_pairs_groups).

`--summarize-parts` and `--compare-parts` give part-level psi: the inclusion of every exon of a multi-isoform gene, the sum of
the psi of the isoforms that hold it, with its credible interval, and its delta psi between two samples (part_psi.py;
DESIGN.md 23).
"""
import glob
import os
import sys
import time

import numpy as np

from . import capi, compare, diagnostics, miso_db, part_psi, summary
from .settings import Settings

# The default decoder: `device`, because it is the faster one end to end (profiles/miso_text.txt: a tree of
# 40 000 default-settings events, tools/miso_text_bench.py).  MISO_TEXT_DECODE overrides it, the functions' `decoder`
# argument overrides both.
DEFAULT_DECODER = "device"
# text of one device batch: bounds the host copy that joins the events' bodies into one buffer
TEXT_BATCH_BYTES = 1 << 30
# what the last summarize / compare did: events decoded on the device, events left to the host parser (their names),
# the decode kernels' time and bytes (capi.TextStats summed over the batches), wall seconds per stage
last_decode_stats = {}


def _decoder(decoder):
    d = decoder or os.environ.get("MISO_TEXT_DECODE") or DEFAULT_DECODER
    if d not in ("host", "device"):
        raise ValueError("MISO_TEXT_DECODE / decoder must be `host` or `device`, not %r" % (d,))
    return d


def get_samples_dir_filenames(samples_dir):
    """samples_utils.py:351-411: every `.miso` file and every `.miso_db` database of samples_dir, each looked for in the
    directory itself and one level down (chromosome sub-directories), sorted: files first."""
    found = []
    for ext in (".miso", miso_db.MISO_DB_EXT):
        direct = glob.glob(os.path.join(samples_dir, "*" + ext))
        nested = glob.glob(os.path.join(samples_dir, "*", "*" + ext))
        found.append(sorted(f for f in direct + nested if os.path.isfile(f) and not os.path.basename(f).startswith(".")))
    if found[0] and found[1]:
        print("WARNING: Directory %s has both *.miso and *.miso_db files" % samples_dir)
    return found[0] + found[1]


def list_events(samples_dir):
    """(files, rows): the `.miso` paths, and per database the event names to take from it.  Each event once: a row whose
    event is also a file is left out (the file wins), and so is a row whose name an earlier database had."""
    names = get_samples_dir_filenames(samples_dir)
    files = [f for f in names if not miso_db.is_miso_db_fname(f)]
    seen = {miso_db.strip_miso_ext(os.path.basename(f)) for f in files}
    rows = {}
    for dbf in names[len(files):]:
        with miso_db.MISODatabase(dbf) as db:
            mine = [n for n in dict.fromkeys(db.get_all_event_names()) if n not in seen]
        seen.update(mine)
        rows[dbf] = mine
    return files, rows


def _header_fields(header):
    line = header.split("\n", 1)[0]
    return dict(kv.split("=", 1) for kv in line[1:].split("\t") if "=" in kv)


def _parse_rows(body):
    """The rows "psi_1,...,psi_K<TAB>log_score" as samples [S, K], parsed by numpy's C reader in one go.  Empty lines
    are ignored and the last LF may be missing, as for the device decoder (include/miso_amd.h) and the reference's
    load_samples; K comes from the first non-empty line."""
    if body.startswith("\n") or "\n\n" in body:
        body = "\n".join(ln for ln in body.split("\n") if ln)
    if not body:
        raise ValueError("no sample rows")
    first = body.split("\n", 1)[0]
    K = first.split("\t")[0].count(",") + 1
    flat = np.array(body.replace("\t", ",").replace("\n", ",").strip(",").split(","), dtype=np.float64)
    rows = flat.reshape(-1, K + 1)
    return np.ascontiguousarray(rows[:, :K])


def parse_miso_file(path):
    """samples_utils.py:130-180 load_samples: (event name, samples [S, K], header dict)."""
    with open(path) as f:
        header = f.readline().rstrip("\n")
        f.readline()                                      # sampled_psi<TAB>log_score
        body = f.read()
    fields = dict(kv.split("=", 1) for kv in header[1:].split("\t") if "=" in kv)
    return os.path.basename(path)[:-len(".miso")], _parse_rows(body), fields


def parse_miso_text(name, header, rows):
    """parse_miso_file's twin for a packed event: a `.miso_db` row's (event_name, header, psi_vals_and_scores)."""
    return name, _parse_rows(rows), _header_fields(header)


class _Event:
    """One event's text as read: `header` (str, the two header lines) and `body` (bytes, the rows)."""
    __slots__ = ("name", "header", "body", "where", "K", "S")

    def __init__(self, name, header, body, where):
        self.name, self.header, self.body, self.where, self.K, self.S = name, header, body, where, 0, 0

    def parse(self):
        return parse_miso_text(self.name, self.header, self.body.decode())


def _parse_or_skip(ev):
    """An event that cannot be parsed (a header without sample rows, a truncated write) costs the run that event, not the
    directory: the reference skips what it cannot load (samples_utils.py:282-292 `Skipping ...`).  ev: a path or an
    _Event."""
    try:
        return parse_miso_file(ev) if isinstance(ev, str) else ev.parse()
    except (ValueError, IndexError, OSError) as err:
        print("Skipping %s: %s" % (os.path.basename(ev) if isinstance(ev, str) else ev.where, err))
        return None


def _threads(processes=None):
    """(not the affinity mask alone: under a CPU quota it names many more cores than the process may use)"""
    return processes or capi.usable_threads()


def _pool_map(fn, items, processes=None):
    """fn over items in THREADS: the work is C code that releases the GIL (numpy's parser, file reads, SQLite) and a
    thread pool never forks a process that has already initialised the GPU runtime -- the caller may have summarised
    another directory on the device a moment ago."""
    if len(items) < 64:
        return [fn(x) for x in items]
    from concurrent.futures import ThreadPoolExecutor
    n = _threads(processes)
    with ThreadPoolExecutor(n) as pool:
        return list(pool.map(fn, items, chunksize=max(1, len(items) // (8 * n))))


def _load_all(paths, processes=None):
    """Every file (or _Event) parsed on the host cores."""
    return [e for e in _pool_map(_parse_or_skip, paths, processes) if e is not None]


def _read_file(path):
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError as err:
        print("Skipping %s: %s" % (os.path.basename(path), err))
        return None
    cut = data.find(b"\n")
    cut = data.find(b"\n", cut + 1) if cut >= 0 else -1
    if cut < 0:
        print("Skipping %s: no sample rows" % os.path.basename(path))
        return None
    return _Event(os.path.basename(path)[:-len(".miso")], data[:cut + 1].decode(errors="replace"), data[cut + 1:], path)


def _read_db(job):
    """One database's wanted rows: one SELECT, the text as bytes (no decode / encode round trip)."""
    dbf, wanted = job
    wanted = set(wanted)
    out = {}
    with miso_db.MISODatabase(dbf, text_factory=bytes) as db:
        for name, rows, header in db:
            name = name.decode()
            if name in wanted and name not in out:
                out[name] = _Event(name, header.decode(errors="replace"), rows, "%s:%s" % (dbf, name))
    return list(out.values())


def _read_events(files, rows):
    """The events' text: files and databases read side by side, nothing parsed yet."""
    evs = [e for e in _pool_map(_read_file, files) if e is not None]
    for part in _pool_map(_read_db, [(dbf, names) for dbf, names in rows.items() if names]):
        evs.extend(part)
    return evs


def _text_batches(items, size_of):
    """items in runs of at most TEXT_BATCH_BYTES of text (at least one item each)."""
    run, n = [], 0
    for it in items:
        sz = size_of(it)
        if run and n + sz > TEXT_BATCH_BYTES:
            yield run
            run, n = [], 0
        run.append(it)
        n += sz
    if run:
        yield run


def _joined(evs):
    offs = np.zeros(len(evs) + 1, np.int64)
    np.cumsum([len(e.body) for e in evs], out=offs[1:])
    return b"".join(e.body for e in evs), offs


def _shape(evs):
    """Isoforms and rows of every event's text (capi.text_shape: host threads, no device)."""
    for run in _text_batches(evs, lambda e: len(e.body)):
        text, offs = _joined(run)
        K, S = capi.text_shape(text, offs)
        for e, k, s in zip(run, K, S):
            e.K, e.S = int(k), int(s)


def _device_ok(e):
    return 1 <= e.K <= capi.MISO_MAX_ISOFORMS and e.S >= 1


class _Stats:
    def __init__(self, decoder):
        self.clock = time.perf_counter
        self.d = {"decoder": decoder, "device_events": 0, "fallback_events": [], "chunks": 0, "text_bytes": 0,
                  "sample_bytes": 0, "kernel_ms": 0.0, "decode_ms": 0.0, "stage_s": {}}
        self.t = self.clock()

    def stage(self, name):
        now = self.clock()
        self.d["stage_s"][name] = self.d["stage_s"].get(name, 0.0) + now - self.t
        self.t = now

    def add(self, batch, evs):
        st = batch.text_stats
        for k in ("chunks", "text_bytes", "sample_bytes", "kernel_ms", "decode_ms"):
            self.d[k] += st[k]
        self.d["device_events"] += int(st["decoded"])
        self.d["fallback_events"] += [e.name for e, s in zip(evs, batch.status) if s and e.name not in self.d["fallback_events"]]

    def done(self):
        global last_decode_stats
        n = self.d["device_events"] + len(self.d["fallback_events"])
        self.d["fallback_share"] = len(self.d["fallback_events"]) / n if n else 0.0
        last_decode_stats = self.d


def _text_batch(evs, S, device, stats):
    text, offs = _joined(evs)
    b = capi.SamplesBatch.from_text(text, offs, [e.K for e in evs], S, device=device)
    stats.add(b, evs)
    return b


def _by_sample_count(events):
    groups = {}
    for ev in events:
        groups.setdefault(ev[1].shape[0], []).append(ev)
    return groups


def _summarize_parsed(events, confidence_level, device, rows, stats):
    """Summary rows of host-parsed events (name, samples [S, K], header dict)."""
    for S, group in sorted(_by_sample_count(events).items()):
        lo, _ = summary.credible_interval_ranks(S, confidence_level)
        if lo <= 0:                                      # the reference asserts both ranks > 0
            print("Skipping %d events with only %d samples" % (len(group), S))
            continue
        b = capi.SamplesBatch([g[1] for g in group], device=device)
        stats.stage("decode")
        b.summarize(confidence_level)                     # the files' values ARE the samples here
        for i, (name, _, hdr) in enumerate(group):
            rows.append((name,) + tuple(b.summary(i)) + (hdr,))
        stats.stage("summarize")


def summarize_sampler_results(samples_dir, summary_filename, confidence_level=0.95, device=0, decoder=None):
    """samples_utils.py:263-329: one summary row per event of samples_dir (`.miso` files and `.miso_db` rows)."""
    decoder = _decoder(decoder)
    stats = _Stats(decoder)
    files, dbrows = list_events(samples_dir)
    rows = []
    if decoder == "host":
        evs = _read_events([], dbrows)
        stats.stage("read")
        events = _load_all(files + evs)
        stats.stage("parse")
        _summarize_parsed(events, confidence_level, device, rows, stats)
    else:
        evs = _read_events(files, dbrows)
        stats.stage("read")
        _shape(evs)
        stats.stage("shape")
        left = [e for e in evs if not _device_ok(e)]
        groups = {}
        for e in evs:
            if _device_ok(e):
                groups.setdefault(e.S, []).append(e)
        for S, group in sorted(groups.items()):
            lo, _ = summary.credible_interval_ranks(S, confidence_level)
            if lo <= 0:
                print("Skipping %d events with only %d samples" % (len(group), S))
                continue
            for run in _text_batches(group, lambda e: len(e.body)):
                b = _text_batch(run, S, device, stats)
                stats.stage("decode")
                b.summarize(confidence_level)
                for i, e in enumerate(run):
                    if b.status[i]:
                        left.append(e)
                    else:
                        rows.append((e.name,) + tuple(b.summary(i)) + (_header_fields(e.header),))
                stats.stage("summarize")
        # what the device decoder did not take: through the host parser, in batches of their own
        stats.d["fallback_events"] += [e.name for e in left if e.name not in stats.d["fallback_events"]]
        _summarize_parsed(_load_all(left), confidence_level, device, rows, stats)
    rows.sort(key=lambda r: r[0])
    os.makedirs(os.path.dirname(os.path.abspath(summary_filename)), exist_ok=True)
    n = summary.write_summary(summary_filename, rows)
    stats.stage("write")
    stats.done()
    return n


def _diagnosable(S, num_chains, n_events):
    if (S // num_chains) // 2 >= 4:
        return True
    print("Skipping %d events with only %d samples for %d chains" % (n_events, S, num_chains))
    return False


def _rank_diagnostics(b, num_chains, Ks, what):
    """Per event the six arrays of the rank pass, or None where the pass refuses the batch's shape (one notice line)."""
    try:
        b.diagnose_rank(num_chains, diagnostics.RANK_CONFIDENCE_LEVEL)
    except capi.InternalError as e:
        print(diagnostics.rank_notice(what, e))
        return [None] * len(Ks)
    return b.rank_diagnostics_many(range(len(Ks)), Ks)


def _diagnose_rows(b, names, headers, Ks, S, num_chains, rows, status=None, rank=False):
    b.diagnose(num_chains)
    diags = b.diagnostics_many(range(len(names)), Ks)
    if rank:
        ranks = _rank_diagnostics(b, num_chains, Ks, "%d events of %d samples in %d chains" % (len(names), S, num_chains))
    for i, (name, hdr) in enumerate(zip(names, headers)):
        if status is not None and status[i]:
            continue
        warn = diagnostics.header_mismatch(name, hdr, S, num_chains)
        if warn:
            print(warn)
        rows.append((name,) + tuple(diags[i]) + (S, num_chains) + ((ranks[i],) if rank else ()))


def _diagnose_parsed(events, num_chains, device, rows, stats, rank=False):
    """Diagnostics rows of host-parsed events (name, samples [S, K], header dict)."""
    for S, group in sorted(_by_sample_count(events).items()):
        if not _diagnosable(S, num_chains, len(group)):
            continue
        b = capi.SamplesBatch([g[1] for g in group], device=device)
        stats.stage("decode")
        _diagnose_rows(b, [g[0] for g in group], [g[2] for g in group], [g[1].shape[1] for g in group], S, num_chains, rows,
                       rank=rank)
        stats.stage("diagnose")


def diagnose_sampler_results(samples_dir, diag_filename, num_chains=None, device=0, decoder=None, rank=False):
    """One diagnostics row per event of samples_dir (`.miso` files and `.miso_db` rows): what the files' four-decimal
    values say about their chains.  num_chains: the chains the rows interleave (row s is chain s % num_chains), default
    the settings' num_chains; an event whose header disagrees with its row count is named and diagnosed all the same.
    rank: also the six columns of the rank-normalised pass (diagnostics.py)."""
    if num_chains is None:
        num_chains = int(Settings.get_sampler_params()["num_chains"])
    num_chains = int(num_chains)
    if num_chains < 1:
        raise ValueError("--num-chains must be at least 1")
    decoder = _decoder(decoder)
    stats = _Stats(decoder)
    files, dbrows = list_events(samples_dir)
    rows = []
    if decoder == "host":
        evs = _read_events([], dbrows)
        stats.stage("read")
        events = _load_all(files + evs)
        stats.stage("parse")
        _diagnose_parsed(events, num_chains, device, rows, stats, rank)
    else:
        evs = _read_events(files, dbrows)
        stats.stage("read")
        _shape(evs)
        stats.stage("shape")
        left = [e for e in evs if not _device_ok(e)]
        groups = {}
        for e in evs:
            if _device_ok(e):
                groups.setdefault(e.S, []).append(e)
        for S, group in sorted(groups.items()):
            if not _diagnosable(S, num_chains, len(group)):
                continue
            for run in _text_batches(group, lambda e: len(e.body)):
                b = _text_batch(run, S, device, stats)
                stats.stage("decode")
                _diagnose_rows(b, [e.name for e in run], [_header_fields(e.header) for e in run], [e.K for e in run], S,
                               num_chains, rows, status=b.status, rank=rank)
                left += [e for i, e in enumerate(run) if b.status[i]]
                stats.stage("diagnose")
        stats.d["fallback_events"] += [e.name for e in left if e.name not in stats.d["fallback_events"]]
        _diagnose_parsed(_load_all(left), num_chains, device, rows, stats, rank)
    rows.sort(key=lambda r: r[0])
    os.makedirs(os.path.dirname(os.path.abspath(diag_filename)), exist_ok=True)
    n = diagnostics.write_diagnostics(diag_filename, rows, rank=rank)
    stats.stage("write")
    stats.done()
    return n


def _sources(samples_dir):
    """event name -> where it is: a `.miso` path, or (database, name)."""
    files, dbrows = list_events(samples_dir)
    src = {os.path.basename(p)[:-len(".miso")]: p for p in files}
    for dbf, names in dbrows.items():
        for n in names:
            src.setdefault(n, (dbf, n))
    return src


def _read_named(src, names):
    files = [src[n] for n in names if isinstance(src[n], str)]
    dbrows = {}
    for n in names:
        if not isinstance(src[n], str):
            dbrows.setdefault(src[n][0], []).append(n)
    return files, dbrows


MAX_PAIR_DRAWS = 8192      # miso_batch_compare_pairs: draws per event and sample (both sorted columns stay in LDS)


def _delta_posterior(b1, b2, n, names, S, confidence_level, delta):
    """delta = (thresholds, results): results[name] = Batch.pair_comparison of every event of the two batches -- delta psi
    over all pairs of their draws --, or None where the samples are too long for the pass (one notice per
    call of output_samples_comparison: results[None] remembers it)."""
    if delta is None:
        return
    thresholds, results = delta
    if S > MAX_PAIR_DRAWS:
        if None not in results:
            print("No delta psi posterior for events of more than %d samples (%s has %d): their rows print NA"
                  % (MAX_PAIR_DRAWS, names[0], S))
            results[None] = None
        results.update((name, None) for name in names)
        return
    b1.compare_pairs(b2, confidence_level, thresholds)
    results.update((name, b1.pair_comparison(i)) for i, name in enumerate(names))


def _compare_parsed(pairs, confidence_level, smoothing, device, rows, delta=None):
    """Comparison rows of host-parsed pairs ((name, samples, header), (name, samples, header)); delta: _delta_posterior's."""
    groups = {}
    for a, b2 in pairs:
        if a[1].shape != b2[1].shape:
            print("Skipping %s: the two samples differ in isoforms or sample count" % a[0])
            continue
        groups.setdefault(a[1].shape[0], []).append((a, b2))
    for S, group in sorted(groups.items()):
        lo, _ = summary.credible_interval_ranks(S, confidence_level)
        if lo <= 0 or S < 2:
            continue
        b1 = capi.SamplesBatch([g[0][1] for g in group], device=device)
        b2 = capi.SamplesBatch([g[1][1] for g in group], device=device)
        b1.summarize(confidence_level); b2.summarize(confidence_level)
        b1.compare(b2, smoothing)
        _delta_posterior(b1, b2, len(group), [g[0][0] for g in group], S, confidence_level, delta)
        for i, (a, c) in enumerate(group):
            _, _, bf, _ = b1.comparison(i)
            rows.append((a[0], tuple(b1.summary(i)), tuple(b2.summary(i)), bf, a[2], c[2]))


def output_samples_comparison(sample1_dir, sample2_dir, output_dir, confidence_level=0.95, smoothing=0.3,
                              sample_labels=None, device=0, decoder=None, delta_thresholds=None):
    """hypothesis_test.py:186-345: events present in BOTH directories (262-264), `<l1>_vs_<l2>.miso_bf`.
    delta_thresholds (--delta-posterior): also `<l1>_vs_<l2>.miso_dpsi` beside it, the table of delta psi over all pairs of
    the two samples' draws (compare.write_dpsi) for the same events; the `.miso_bf` is what it is without."""
    delta = None if delta_thresholds is None else (compare.check_delta_thresholds(delta_thresholds), {})
    decoder = _decoder(decoder)
    stats = _Stats(decoder)
    l1, l2 = sample_labels or (os.path.basename(os.path.normpath(sample1_dir)), os.path.basename(os.path.normpath(sample2_dir)))
    f1, f2 = _sources(sample1_dir), _sources(sample2_dir)
    common = sorted(set(f1) & set(f2))
    print("Given %d events in %s and %d in %s: %d in both" % (len(f1), sample1_dir, len(f2), sample2_dir, len(common)))
    rows = []
    if decoder == "host":
        sides = []
        for src in (f1, f2):
            files, dbrows = _read_named(src, common)
            sides.append({e[0]: e for e in _load_all(files + _read_events([], dbrows))})
        ev1, ev2 = sides
        both = sorted(set(ev1) & set(ev2))                # (an event that could not be parsed drops out of the pairing)
        stats.stage("read+parse")
        _compare_parsed([(ev1[n], ev2[n]) for n in both], confidence_level, smoothing, device, rows, delta)
    else:
        sides = []
        for src in (f1, f2):
            evs = _read_events(*_read_named(src, common))
            _shape(evs)
            sides.append({e.name: e for e in evs})
        ev1, ev2 = sides
        both = sorted(set(ev1) & set(ev2))
        stats.stage("read+shape")
        left, groups = [], {}
        for n in both:
            a, c = ev1[n], ev2[n]
            if not (_device_ok(a) and _device_ok(c)):
                left.append((a, c))
            elif (a.K, a.S) != (c.K, c.S):
                print("Skipping %s: the two samples differ in isoforms or sample count" % n)
            else:
                groups.setdefault(a.S, []).append((a, c))
        for S, group in sorted(groups.items()):
            lo, _ = summary.credible_interval_ranks(S, confidence_level)
            if lo <= 0 or S < 2:
                continue
            for run in _text_batches(group, lambda p: len(p[0].body) + len(p[1].body)):
                b1 = _text_batch([p[0] for p in run], S, device, stats)
                b2 = _text_batch([p[1] for p in run], S, device, stats)
                b1.summarize(confidence_level); b2.summarize(confidence_level)
                b1.compare(b2, smoothing)
                # (an event the decoder did not take comes back not finite here; the host parser's pass below replaces it)
                _delta_posterior(b1, b2, len(run), [p[0].name for p in run], S, confidence_level, delta)
                for i, (a, c) in enumerate(run):
                    if b1.status[i] or b2.status[i]:
                        left.append((a, c))
                        continue
                    _, _, bf, _ = b1.comparison(i)
                    rows.append((a.name, tuple(b1.summary(i)), tuple(b2.summary(i)), bf, _header_fields(a.header),
                                 _header_fields(c.header)))
        stats.stage("decode+compare")
        # pairs with a side the device decoder did not take: both sides through the host parser
        for a, c in left:
            for e in (a, c):
                if e.name not in stats.d["fallback_events"]:
                    stats.d["fallback_events"].append(e.name)
        parsed = [(_parse_or_skip(a), _parse_or_skip(c)) for a, c in left]
        _compare_parsed([p for p in parsed if p[0] is not None and p[1] is not None], confidence_level, smoothing,
                        device, rows, delta)
    rows.sort(key=lambda r: r[0])
    name = "%s_vs_%s" % (l1, l2)
    out = os.path.join(output_dir, name, "bayes-factors", name + ".miso_bf")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    compare.write_comparison(out, rows)
    if delta is not None:
        compare.write_dpsi(out[:-len(".miso_bf")] + ".miso_dpsi", [r + (delta[1][r[0]],) for r in rows], delta[0])
    stats.stage("write")
    stats.done()
    return out, len(rows)


# ---- replicate groups: every pair of two groups of sample directories in one device pass per chunk of events ----
# text of one group chunk, all samples together (what TEXT_BATCH_BYTES is to the two samples of a pair)
GROUP_TEXT_BYTES = TEXT_BATCH_BYTES


def group_labels(dirs1, dirs2, labels1=None, labels2=None):
    """The two groups' labels (default: the directories' base names), checked before anything is read: as many labels as
    directories, and no two pairs with the same `<l1>_vs_<l2>` (they would write the same file)."""
    out = []
    for which, dirs, labels in ((1, dirs1, labels1), (2, dirs2, labels2)):
        if not dirs:
            raise ValueError("group %d has no sample directory" % which)
        if labels is None:
            labels = [os.path.basename(os.path.normpath(d)) for d in dirs]
        labels = list(labels)
        if len(labels) != len(dirs):
            raise ValueError("group %d has %d directories and %d labels" % (which, len(dirs), len(labels)))
        out.append(labels)
    seen = {}
    for i, a in enumerate(out[0]):
        for j, c in enumerate(out[1]):
            name = "%s_vs_%s" % (a, c)
            if name in seen:
                raise ValueError("pairs %r and %r would both write %s: give distinct --group-labels" % (seen[name], (i, j), name))
            seen[name] = (i, j)
    return out[0], out[1]


def plan_group_comparison(listings1, listings2, chunk_bytes=None):
    """Which events of two groups of samples go where -- host only, nothing is read or decoded here.

    listingsN: per sample of group N an iterable of (name, K, S, decodable[, text_bytes]): an event the sample has, its
    isoforms and sample rows, whether the device route can take it (for text: 1 <= K <= MISO_MAX_ISOFORMS and S >= 1) and
    the size of its text (0 when left out).  Only events that at least one sample of EACH group has take part: the
    others are in no pair.  Returns a dict:

      chunks      [{"S", "present1", "present2", "names", "K", "bytes"}]: the events of the group route, i.e. those whose
                  samples all agree on (K, S) and are all decodable.  One chunk = one launch of the group kernel over the
                  samples that HAVE its events (present1 / present2: indices into the groups; a sample that lacks an
                  event is masked out of that event's pairs by not being in its chunk); events in name order, all with S
                  rows, their text over all present samples within chunk_bytes (at least one event a chunk).
      pair_route  names of events whose samples disagree on (K, S): every pair that has one goes the pairwise route (which
                  prints its `Skipping ...` line where the pair itself disagrees).
      fallback    names of events some sample cannot hand to the device route: every pair through the host parser.
      pairs_of    name -> [(i, j)] for the events of pair_route and fallback: the pairs whose two samples have it."""
    if chunk_bytes is None:
        chunk_bytes = GROUP_TEXT_BYTES
    have = ({}, {})                                       # name -> {sample index: (K, S, decodable, bytes)}
    for side, listings in enumerate((listings1, listings2)):
        for i, listing in enumerate(listings):
            for rec in listing:
                name, K, S, ok = rec[:4]
                nbytes = rec[4] if len(rec) > 4 else 0
                have[side].setdefault(name, {})[i] = (int(K), int(S), bool(ok), int(nbytes))
    plan = {"chunks": [], "pair_route": [], "fallback": [], "pairs_of": {}}
    classes = {}
    for name in sorted(set(have[0]) & set(have[1])):
        recs = list(have[0][name].values()) + list(have[1][name].values())
        if not all(r[2] for r in recs):
            where = plan["fallback"]
        elif len({r[:2] for r in recs}) > 1:
            where = plan["pair_route"]
        else:
            key = (recs[0][1], tuple(sorted(have[0][name])), tuple(sorted(have[1][name])))
            classes.setdefault(key, []).append((name, recs[0][0], sum(r[3] for r in recs)))
            continue
        where.append(name)
        plan["pairs_of"][name] = [(i, j) for i in sorted(have[0][name]) for j in sorted(have[1][name])]
    for (S, p1, p2), evs in sorted(classes.items()):
        run, n = [], 0
        for ev in evs + [None]:
            if ev is None or (run and n + ev[2] > chunk_bytes):
                if run:
                    plan["chunks"].append({"S": S, "present1": p1, "present2": p2, "names": [e[0] for e in run],
                                           "K": [e[1] for e in run], "bytes": n})
                run, n = [], 0
            if ev is not None:
                run.append(ev)
                n += ev[2]
    return plan


class _TextSample:
    """One sample directory for the group pass, decoder = device: its events' text, read once."""

    def __init__(self, src, names):
        evs = _read_events(*_read_named(src, names))
        _shape(evs)
        self.ev = {e.name: e for e in evs}
        self.parsed = {}

    def listing(self):
        return [(e.name, e.K, e.S, _device_ok(e), len(e.body)) for e in self.ev.values()]

    def batch(self, names, S, device, stats):
        return _text_batch([self.ev[n] for n in names], S, device, stats)

    def header(self, name):
        return _header_fields(self.ev[name].header)

    def parse(self, name):
        if name not in self.parsed:
            self.parsed[name] = _parse_or_skip(self.ev[name])
        return self.parsed[name]


class _ParsedSample:
    """The same, decoder = host: every event parsed on the host cores, once."""

    def __init__(self, src, names):
        files, dbrows = _read_named(src, names)
        self.ev = {e[0]: e for e in _load_all(files + _read_events([], dbrows))}

    def listing(self):
        return [(n, a.shape[1], a.shape[0], True, a.nbytes) for n, a, _ in self.ev.values()]

    def batch(self, names, S, device, stats):
        b = capi.SamplesBatch([self.ev[n][1] for n in names], device=device)
        b.status = np.zeros(len(names), np.int32)
        return b

    def header(self, name):
        return self.ev[name][2]

    def parse(self, name):
        return self.ev[name]


MAX_GROUP_PAIR_DRAWS = capi.MAX_GROUP_PAIR_DRAWS      # miso_batch_compare_pairs_groups: pooled draws per event and group
DEFAULT_GROUP_NAMES = ("group1", "group2")


class _GroupDelta:
    """--compare-groups --delta-posterior: what the pairwise tables and the pooled table are written from.
    pair[(i, j)]: _delta_posterior's results of that pair of samples.  rows: compare.write_group_dpsi's, one per event that a
    sample of each group has.  A cause for NA is said once per call (notice)."""

    def __init__(self, thresholds, n1, n2):
        self.thresholds = compare.check_delta_thresholds(thresholds)
        self.pair = {(i, j): {} for i in range(n1) for j in range(n2)}
        self.rows = []
        self.said = set()
        self.kernel_ms = 0.0

    def of_pair(self, i, j):
        """_delta_posterior's `delta` for the pair; its own notice is printed by the first pair that meets the cause"""
        res = self.pair[(i, j)]
        if "pair_draws" in self.said:
            res[None] = None
        return self.thresholds, res

    def seen(self, i, j):
        if None in self.pair[(i, j)]:
            self.said.add("pair_draws")

    def notice(self, cause, text):
        if cause not in self.said:
            print(text)
            self.said.add(cause)

    def pooled(self, batches1, batches2, names, K, S, confidence_level):
        """{name: pair_comparison} of the events of two lists of batches, pooled on the device; None for all of them where a
        group's draws are too many for the pass"""
        for g, bs in ((1, batches1), (2, batches2)):
            if len(bs) * S > MAX_GROUP_PAIR_DRAWS:
                self.notice("group_draws", "No pooled delta psi for events of more than %d draws a group (%s: group %d has %d "
                            "samples of %d): their rows print NA" % (MAX_GROUP_PAIR_DRAWS, names[0], g, len(bs), S))
                return {name: None for name in names}
        gp = capi.compare_pairs_groups(batches1, batches2, confidence_level, self.thresholds, noiso=K)
        self.kernel_ms += gp.kernel_ms
        return {name: gp.pair_comparison(e) for e, name in enumerate(names)}


def _group_delta_parsed(gd, samples, names, pairs_of, confidence_level, device):
    """The pooled rows of the events the group route did not take (gd: _GroupDelta): pooled from the host parser's doubles
    over the samples that have the event where those agree on (K, S) -- the same doubles, the same device pass --, NA where
    they do not or where the parser refuses the event in some sample too."""
    classes = {}
    for name in names:
        have = [sorted({p[g] for p in pairs_of[name]}) for g in (0, 1)]
        parsed = [[samples[g][i].parse(name) for i in have[g]] for g in (0, 1)]
        header = samples[0][have[0][0]].header(name)
        flat = parsed[0] + parsed[1]
        if any(p is None for p in flat):
            gd.notice("unparsed", "No pooled delta psi for events that could not be parsed in some sample (%s): their rows print NA"
                      % name)
        elif len({p[1].shape for p in flat}) > 1:
            gd.notice("shapes", "No pooled delta psi for events whose samples differ in isoforms or sample count (%s): their rows "
                      "print NA" % name)
        else:
            S, K = flat[0][1].shape
            classes.setdefault((S, tuple(have[0]), tuple(have[1])), []).append((name, K, parsed, header))
            continue
        gd.rows.append((name, len(have[0]), len(have[1]), None, None, None, header))
    for (S, p1, p2), evs in sorted(classes.items()):
        lo, _ = summary.credible_interval_ranks(S, confidence_level)
        if lo <= 0 or S < 2:                              # as the chunks of the group route: no interval, no rows
            continue
        batches = [[capi.SamplesBatch([ev[2][g][a][1] for ev in evs], device=device) for a in range(len(p))]
                   for g, p in enumerate((p1, p2))]
        for bs in batches:
            for b in bs:
                b.summarize(confidence_level)
        res = gd.pooled(batches[0], batches[1], [ev[0] for ev in evs], [ev[1] for ev in evs], S, confidence_level)
        for e, (name, K, _, header) in enumerate(evs):
            means = [[b.summary(e)[0] for b in bs] for bs in batches]
            gd.rows.append((name, len(p1), len(p2), means[0], means[1], res[name], header))


def output_group_comparisons(dirs1, dirs2, output_dir, labels1=None, labels2=None, confidence_level=0.95, smoothing=0.3,
                             device=0, decoder=None, delta_thresholds=None, group_names=None):
    """compare_miso for replicates: every pair (dirs1[i], dirs2[j]) as output_samples_comparison writes it -- the same
    `<l1>_vs_<l2>/bayes-factors/<l1>_vs_<l2>.miso_bf`, byte for byte -- with every tree listed and read once, every
    sample's text decoded and summarised once, and all pairs of a chunk of events in one launch
    (capi.compare_groups).  plan_group_comparison decides which events take that route.  Returns [(path, n_rows)] in
    row-major pair order.
    delta_thresholds (--delta-posterior): also `<l1>_vs_<l2>.miso_dpsi` beside every `.miso_bf`, as output_samples_comparison
    writes it, and the pooled table `<A>_vs_<B>/delta-psi/<A>_vs_<B>.miso_group_dpsi` (group_names = (A, B), default
    group1, group2): delta psi over all pairs of the two groups' pooled draws (capi.compare_pairs_groups), one
    row per event that a sample of each group has; its (path, n_rows) is the last of the list.  Without it the files are what
    they are without the option."""
    labels1, labels2 = group_labels(dirs1, dirs2, labels1, labels2)
    decoder = _decoder(decoder)
    stats = _Stats(decoder)
    n1, n2 = len(dirs1), len(dirs2)
    gd = None if delta_thresholds is None else _GroupDelta(delta_thresholds, n1, n2)
    group_names = tuple(group_names or DEFAULT_GROUP_NAMES)
    stats.d.update({"samples": n1 + n2, "pairs": n1 * n2, "group_events": 0, "pair_route_events": [], "group_chunks": 0,
                    "compare_kernel_ms": 0.0})
    srcs = [[_sources(d) for d in dirs] for dirs in (dirs1, dirs2)]
    stats.stage("list")
    # a sample reads the events that some sample of the other group has too: the others are in no pair
    others = [set().union(*srcs[1 - g]) for g in (0, 1)]
    make = _ParsedSample if decoder == "host" else _TextSample
    samples = [[make(src, sorted(set(src) & others[g])) for src in srcs[g]] for g in (0, 1)]
    stats.stage("read+parse" if decoder == "host" else "read+shape")
    plan = plan_group_comparison([s.listing() for s in samples[0]], [s.listing() for s in samples[1]])
    stats.stage("plan")
    rows = {(i, j): [] for i in range(n1) for j in range(n2)}
    routed = {name: "fallback" for name in plan["fallback"]}
    routed.update({name: "pair" for name in plan["pair_route"]})
    pairs_of = dict(plan["pairs_of"])

    for ch in plan["chunks"]:
        S, names, K = ch["S"], ch["names"], ch["K"]
        lo, _ = summary.credible_interval_ranks(S, confidence_level)
        if lo <= 0 or S < 2:                              # as the pairwise route: no interval, no comparison
            continue
        present = (ch["present1"], ch["present2"])
        batches = [[samples[g][i].batch(names, S, device, stats) for i in present[g]] for g in (0, 1)]
        stats.stage("decode")
        summ = []
        for g in (0, 1):
            for b in batches[g]:
                b.summarize(confidence_level)
            summ.append([b.summaries(range(len(names)), K) for b in batches[g]])
        stats.stage("summarize")
        cmp = capi.compare_groups(batches[0], batches[1], smoothing, noiso=K)
        stats.d["compare_kernel_ms"] += cmp.kernel_ms
        stats.d["group_chunks"] += 1
        stats.stage("compare")
        if gd is not None:
            for a, i in enumerate(present[0]):
                for c, j in enumerate(present[1]):
                    # (an event the decoder did not take comes back not finite here; the host parser's pass below replaces it)
                    _delta_posterior(batches[0][a], batches[1][c], len(names), names, S, confidence_level, gd.of_pair(i, j))
                    gd.seen(i, j)
            pooled = gd.pooled(batches[0], batches[1], names, K, S, confidence_level)
            stats.stage("delta")
        bad = np.zeros(len(names), bool)
        for g in (0, 1):
            for b in batches[g]:
                bad |= np.asarray(b.status) != 0
        hdrs = [[[None if bad[e] else samples[g][i].header(n) for e, n in enumerate(names)] for i in present[g]]
                for g in (0, 1)]
        for a, i in enumerate(present[0]):
            for c, j in enumerate(present[1]):
                bf = cmp.out[a, c]
                out = rows[(i, j)]
                for e, name in enumerate(names):
                    if not bad[e]:
                        out.append((name, summ[0][a][e], summ[1][c][e], bf[cmp.offs[e] + 2:cmp.offs[e + 1]:4],
                                    hdrs[0][a][e], hdrs[1][c][e]))
        if gd is not None:
            for e, name in enumerate(names):
                if not bad[e]:
                    gd.rows.append((name, len(present[0]), len(present[1]), [sm[e][0] for sm in summ[0]],
                                    [sm[e][0] for sm in summ[1]], pooled[name], hdrs[0][0][e]))
        for e, name in enumerate(names):
            if bad[e]:                                    # outside the device decoder's grammar in some sample
                routed[name] = "fallback"
                pairs_of[name] = [(i, j) for i in present[0] for j in present[1]]
        stats.d["group_events"] += int((~bad).sum())
        del batches, cmp
        stats.stage("rows")

    # what the group route did not take, pair by pair as output_samples_comparison does it: through the host parser
    # (the same doubles as the device decoder's), _compare_parsed prints the `Skipping ...` of a pair that disagrees
    left = {}
    for name in sorted(routed):
        for pair in pairs_of[name]:
            left.setdefault(pair, []).append(name)
    for (i, j), names in sorted(left.items()):
        parsed = [(samples[0][i].parse(n), samples[1][j].parse(n)) for n in names]
        _compare_parsed([p for p in parsed if p[0] is not None and p[1] is not None], confidence_level, smoothing, device,
                        rows[(i, j)], None if gd is None else gd.of_pair(i, j))
        if gd is not None:
            gd.seen(i, j)
    stats.d["fallback_events"] = sorted(n for n, r in routed.items() if r == "fallback")
    stats.d["pair_route_events"] = sorted(n for n, r in routed.items() if r == "pair")
    stats.stage("pairwise")
    if gd is not None:
        pair_route = sorted(n for n, r in routed.items() if r == "pair")
        if pair_route:
            gd.notice("shapes", "No pooled delta psi for events whose samples differ in isoforms or sample count (%s): their "
                      "rows print NA" % pair_route[0])
        for name in pair_route:
            have = [sorted({p[g] for p in pairs_of[name]}) for g in (0, 1)]
            gd.rows.append((name, len(have[0]), len(have[1]), None, None, None, samples[0][have[0][0]].header(name)))
        _group_delta_parsed(gd, samples, sorted(n for n, r in routed.items() if r == "fallback"), pairs_of, confidence_level,
                            device)
        stats.d["pairs_groups_kernel_ms"] = gd.kernel_ms
        stats.stage("delta")

    written = []
    for i in range(n1):
        for j in range(n2):
            name = "%s_vs_%s" % (labels1[i], labels2[j])
            out = os.path.join(output_dir, name, "bayes-factors", name + ".miso_bf")
            os.makedirs(os.path.dirname(out), exist_ok=True)
            rows[(i, j)].sort(key=lambda r: r[0])
            compare.write_comparison(out, rows[(i, j)])
            if gd is not None:
                compare.write_dpsi(out[:-len(".miso_bf")] + ".miso_dpsi", [r + (gd.pair[(i, j)][r[0]],) for r in rows[(i, j)]],
                                   gd.thresholds)
            written.append((out, len(rows[(i, j)])))
    if gd is not None:
        name = "%s_vs_%s" % group_names
        out = os.path.join(output_dir, name, "delta-psi", name + ".miso_group_dpsi")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        gd.rows.sort(key=lambda r: r[0])
        written.append((out, compare.write_group_dpsi(out, gd.rows, gd.thresholds)))
    stats.stage("write")
    stats.done()
    return written


MAX_EXACT_GROUP = 8     # replicates a group in the exact pooled pass (include/miso_amd.h miso_exact_delta_groups)


class _ExactKind:
    """What the two pooled exact tables differ in.  flag: as the messages name it; suffix, read: a sample directory's table;
    written_by: the run that leaves it; call(tables, have, evs): the capi call for the events `evs`, which the replicates
    have[g] of group g hold with exact = 1."""

    def __init__(self, flag, suffix, read, written_by, call):
        self.flag, self.suffix, self.read, self.written_by, self.call = flag, suffix, read, written_by, call

    def path(self, sample_dir):
        return os.path.join(sample_dir, "summary", os.path.basename(os.path.normpath(sample_dir)) + self.suffix)


def _exact_stats_call(tables, have, evs, probs, z):
    s1, s2 = ([[tables[g][r][name][1] for r in have[g]] for name in evs] for g in (0, 1))
    return capi.exact_delta_groups(s1, s2, probs, z)


def _exact_pairs_call(tables, have, evs, probs, z):
    groups = [[([tables[g][r][name][1] for name in evs], [tables[g][r][name][2] for name in evs]) for r in have[g]] for g in (0, 1)]
    return capi.exact_paired_delta_groups(groups[0], groups[1], probs, z)


_EXACT_STATS = _ExactKind("--exact-delta-posterior", ".miso_exact_stats", compare.read_exact_stats,
                          "miso --run ... --exact --exact-stats", _exact_stats_call)
_EXACT_PAIRS = _ExactKind("--exact-paired-delta-posterior", ".miso_exact_pairs", compare.read_exact_pairs,
                          "miso --run ... --paired-end M SD --exact-paired --exact-paired-stats", _exact_pairs_call)


def _check_exact_tables(kind, dirs1, dirs2):
    """ValueError, before any work, unless both groups have 1 .. 8 directories and each holds the kind's table"""
    for which, dirs in enumerate((dirs1, dirs2)):
        if not 1 <= len(dirs) <= MAX_EXACT_GROUP:
            raise ValueError("Error: %s pools between 1 and %d replicates a group, group %d has %d"
                             % (kind.flag, MAX_EXACT_GROUP, which + 1, len(dirs)))
    for d in list(dirs1) + list(dirs2):
        if not os.path.isfile(kind.path(d)):
            raise ValueError("Error: %s has no %s (written by %s)" % (d, os.path.relpath(kind.path(d), d), kind.written_by))


def _output_group_exact(kind, dirs1, dirs2, output_dir, delta_thresholds, group_names):
    """`<A>_vs_<B>/delta-psi/<A>_vs_<B>.miso_group_dpsi_exact`, delta psi of the two groups pooled over all pairs of replicates
    from their exact posteriors, without a draw, from each sample directory's table of the kind.  An event is pooled over the
    replicates that have it with exact = 1: the events are grouped by which replicates those are, one device call per such
    pattern.  An event without such a replicate on a side, or one the device call does not take, prints NA; one notice per
    cause.  Returns (path, n_rows)."""
    _check_exact_tables(kind, dirs1, dirs2)
    thresholds = compare.check_delta_thresholds(compare.DEFAULT_DELTA_THRESHOLDS if delta_thresholds is None else delta_thresholds)
    group_names = tuple(group_names or DEFAULT_GROUP_NAMES)
    tables = [[kind.read(kind.path(d)) for d in dirs] for dirs in (dirs1, dirs2)]
    names = sorted(set().union(*[t.keys() for g in tables for t in g]))
    patterns = {}
    for name in names:
        have = tuple(tuple(r for r, t in enumerate(g) if name in t and t[name][0]) for g in tables)
        patterns.setdefault(have, []).append(name)
    rows = {}
    n_none = n_unequal = 0
    for have, evs in patterns.items():
        if not have[0] or not have[1]:
            n_none += len(evs)
            for name in evs:
                rows[name] = (name, len(have[0]), len(have[1]), None, {})
            continue
        res = kind.call(tables, have, evs, compare.EXACT_DPSI_PROBS, compare.delta_points(thresholds))
        for j, name in enumerate(evs):
            row = res.row(j)
            n_unequal += row is None
            rows[name] = (name, len(have[0]), len(have[1]), row, {})
    if n_none:
        print("Notice: %d event(s) have no replicate with an exact posterior in one of the groups: NA in the pooled table" % n_none)
    # (single-end only: the paired-end pass takes every event whose replicates' tables say exact = 1)
    if n_unequal and kind is _EXACT_STATS:
        print("Notice: %d event(s) differ in effective lengths among their replicates: NA in the pooled table" % n_unequal)
    name = "%s_vs_%s" % group_names
    out = os.path.join(output_dir, name, "delta-psi", name + ".miso_group_dpsi_exact")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    return out, compare.write_group_dpsi_exact(out, [rows[n] for n in names], thresholds)


def exact_stats_path(sample_dir):
    """where `miso --run ... --exact --exact-stats` leaves a sample directory's table"""
    return _EXACT_STATS.path(sample_dir)


def check_exact_stats_tables(dirs1, dirs2):
    """ValueError, before any work, unless both groups have 1 .. 8 directories and each holds its `.miso_exact_stats` table"""
    _check_exact_tables(_EXACT_STATS, dirs1, dirs2)


def output_group_exact_delta(dirs1, dirs2, output_dir, delta_thresholds=None, group_names=None):
    """--compare-groups --exact-delta-posterior: the pooled exact table (_output_group_exact; capi.exact_delta_groups, DESIGN.md
    20a) from each sample directory's `.miso_exact_stats` table.  An event with unequal effective lengths among its replicates
    prints NA too."""
    return _output_group_exact(_EXACT_STATS, dirs1, dirs2, output_dir, delta_thresholds, group_names)


def exact_pairs_path(sample_dir):
    """where `miso --run ... --paired-end M SD --exact-paired --exact-paired-stats` leaves a sample directory's table"""
    return _EXACT_PAIRS.path(sample_dir)


def check_exact_pairs_tables(dirs1, dirs2):
    """ValueError, before any work, unless both groups have 1 .. 8 directories and each holds its `.miso_exact_pairs` table"""
    _check_exact_tables(_EXACT_PAIRS, dirs1, dirs2)


def output_group_exact_paired_delta(dirs1, dirs2, output_dir, delta_thresholds=None, group_names=None):
    """--compare-groups --exact-paired-delta-posterior: the same for paired-end replicates (capi.exact_paired_delta_groups,
    DESIGN.md 20b), from each sample directory's `.miso_exact_pairs` table."""
    return _output_group_exact(_EXACT_PAIRS, dirs1, dirs2, output_dir, delta_thresholds, group_names)


def parse_group_args(compare_groups, group_labels_arg=None):
    """`--compare-groups DIR[,DIR...] DIR[,DIR...] OUTPUT_DIR [--group-labels L[,L...] L[,L...]]` ->
    (dirs1, dirs2, output_dir, labels1, labels2); the labels are checked (group_labels) before anything is read."""
    g1, g2, out_dir = compare_groups
    split = lambda v: [x for x in v.split(",") if x]  # noqa: E731
    dirs1, dirs2 = ([os.path.abspath(os.path.expanduser(p)) for p in split(g)] for g in (g1, g2))
    l1 = l2 = None
    if group_labels_arg:
        l1, l2 = (split(v) for v in group_labels_arg)
    l1, l2 = group_labels(dirs1, dirs2, l1, l2)
    return dirs1, dirs2, os.path.abspath(os.path.expanduser(out_dir)), l1, l2


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="summarize_miso / compare_miso over directories of .miso files")
    ap.add_argument("--summarize-samples", nargs=2, metavar=("SAMPLES_DIR", "OUTPUT_DIR"))
    ap.add_argument("--compare-samples", nargs=3, metavar=("SAMPLES_DIR1", "SAMPLES_DIR2", "OUTPUT_DIR"))
    ap.add_argument("--diagnose-samples", nargs=2, metavar=("SAMPLES_DIR", "OUTPUT_DIR"),
                    help="chain diagnostics (split R-hat, ESS, MCSE) of every event: OUTPUT_DIR/summary/<name>.miso_diag")
    ap.add_argument("--num-chains", type=int, default=None,
                    help="with --diagnose-samples: chains the sample rows interleave (default: the settings' num_chains, 6)")
    ap.add_argument("--rank-diagnostics", action="store_true",
                    help="with --diagnose-samples: six more columns from the rank-normalised pass (rank R-hat, bulk ESS, ESS of "
                         "the 95 %% interval's bounds, distinct values)")
    ap.add_argument("--comparison-labels", nargs=2, default=None)
    ap.add_argument("--compare-groups", nargs=3, metavar=("DIR[,DIR...]", "DIR[,DIR...]", "OUTPUT_DIR"),
                    help="every pair of two groups of sample directories (replicates), one .miso_bf per pair")
    ap.add_argument("--group-labels", nargs=2, default=None, metavar=("L[,L...]", "L[,L...]"))
    ap.add_argument("--group-names", nargs=2, default=None, metavar=("A", "B"),
                    help="with --compare-groups --delta-posterior: the two groups' names in the pooled table's path, "
                         "OUTPUT_DIR/A_vs_B/delta-psi/A_vs_B.miso_group_dpsi (default group1 group2)")
    ap.add_argument("--delta-posterior", action="store_true",
                    help="with --compare-groups: the same beside every pair's .miso_bf, and the pooled table "
                         "<A>_vs_<B>.miso_group_dpsi of delta psi over all pairs of the two groups' pooled draws.  "
                         "With --compare-samples: also write <l1>_vs_<l2>.miso_dpsi beside the .miso_bf -- median and 95 %% "
                         "credible interval of delta psi, P(delta psi > 0), P(delta psi < 0) and P(|delta psi| >= T) over ALL "
                         "pairs of the two samples' draws, for events of any number of isoforms")
    ap.add_argument("--exact-delta-posterior", action="store_true",
                    help="with --compare-groups: also the pooled table <A>_vs_<B>.miso_group_dpsi_exact of delta psi over all "
                         "pairs of replicates from their exact posteriors, without a draw -- from every sample directory's "
                         "summary/<name>.miso_exact_stats, which miso --run ... --exact --exact-stats writes")
    ap.add_argument("--exact-paired-delta-posterior", action="store_true",
                    help="with --compare-groups, for paired-end replicates: the same pooled table from every sample directory's "
                         "summary/<name>.miso_exact_pairs, which miso --run ... --paired-end M SD --exact-paired "
                         "--exact-paired-stats writes (not together with --exact-delta-posterior)")
    ap.add_argument("--delta-psi-thresholds", nargs="+", type=float, default=None, metavar="T",
                    help="the thresholds T of --delta-posterior, --exact-delta-posterior and --exact-paired-delta-posterior, each "
                         "in (0, 1), at most four (default 0.1 0.2)")
    ap.add_argument("--summarize-parts", nargs=3, metavar=("SAMPLES_DIR", "INDEX_DIR", "OUTPUT_DIR"),
                    help="part-level psi (part_psi.py): mean and credible interval of every exon's inclusion, "
                         "OUTPUT_DIR/summary/<name>.miso_part_summary; the gene models come from the index directory")
    ap.add_argument("--compare-parts", nargs=4, metavar=("SAMPLES_DIR1", "SAMPLES_DIR2", "INDEX_DIR", "OUTPUT_DIR"),
                    help="the same of either sample and delta psi over all pairs of their draws, per exon: "
                         "<l1>_vs_<l2>.miso_part_dpsi (labels: --comparison-labels, thresholds: --delta-psi-thresholds)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    for opt, given in (("--summarize-parts", a.summarize_parts), ("--compare-parts", a.compare_parts)):
        if given and not os.path.isdir(given[-2]):
            ap.error("%s: no index directory %s" % (opt, given[-2]))
    if a.delta_posterior and not (a.compare_samples or a.compare_groups):      # argument errors, before any work
        # (both wordings: scripts and tests match on the older "goes with --compare-samples")
        ap.error("--delta-posterior needs --compare-samples or --compare-groups "
                 "(--delta-posterior goes with --compare-samples, and with --compare-groups)")
    if a.exact_delta_posterior and not a.compare_groups:
        ap.error("--exact-delta-posterior goes with --compare-groups")
    if a.exact_paired_delta_posterior and not a.compare_groups:
        ap.error("--exact-paired-delta-posterior goes with --compare-groups")
    if a.exact_paired_delta_posterior and a.exact_delta_posterior:
        ap.error("one of --exact-delta-posterior (single-end replicates) and --exact-paired-delta-posterior (paired-end), not both")
    if a.group_names and not (a.compare_groups and (a.delta_posterior or a.exact_delta_posterior or a.exact_paired_delta_posterior)):
        ap.error("--group-names goes with --compare-groups --delta-posterior (or --exact-delta-posterior)")
    if a.delta_psi_thresholds is not None:
        if not (a.delta_posterior or a.exact_delta_posterior or a.exact_paired_delta_posterior or a.compare_parts):
            ap.error("--delta-psi-thresholds goes with --delta-posterior")
        try:
            compare.check_delta_thresholds(a.delta_psi_thresholds)
        except ValueError as err:
            ap.error(str(err))
    if a.summarize_samples:
        samples_dir, out_dir = (os.path.abspath(os.path.expanduser(p)) for p in a.summarize_samples)
        label = os.path.basename(os.path.normpath(samples_dir))          # summarize_miso.py: <dir name>.miso_summary
        fname = os.path.join(out_dir, "summary", label + ".miso_summary")
        n = summarize_sampler_results(samples_dir, fname, device=a.device)
        print("Summarized %d events into %s" % (n, fname))
    if a.diagnose_samples:
        samples_dir, out_dir = (os.path.abspath(os.path.expanduser(p)) for p in a.diagnose_samples)
        label = os.path.basename(os.path.normpath(samples_dir))
        fname = os.path.join(out_dir, "summary", label + ".miso_diag")
        n = diagnose_sampler_results(samples_dir, fname, num_chains=a.num_chains, device=a.device, rank=a.rank_diagnostics)
        print("Diagnosed %d events into %s" % (n, fname))
    elif a.num_chains is not None:
        ap.error("--num-chains goes with --diagnose-samples")
    elif a.rank_diagnostics:
        ap.error("--rank-diagnostics goes with --diagnose-samples")
    thr = None
    if a.delta_posterior:
        thr = compare.DEFAULT_DELTA_THRESHOLDS if a.delta_psi_thresholds is None else a.delta_psi_thresholds
    if a.compare_samples:
        d1, d2, out_dir = (os.path.abspath(os.path.expanduser(p)) for p in a.compare_samples)
        out, n = output_samples_comparison(d1, d2, out_dir, sample_labels=a.comparison_labels, device=a.device,
                                           delta_thresholds=thr)
        print("Compared %d events into %s" % (n, out))
    if a.compare_groups:
        try:
            dirs1, dirs2, out_dir, l1, l2 = parse_group_args(a.compare_groups, a.group_labels)
            if a.exact_delta_posterior:
                check_exact_stats_tables(dirs1, dirs2)
            if a.exact_paired_delta_posterior:
                check_exact_pairs_tables(dirs1, dirs2)
        except ValueError as err:
            ap.error(str(err))
        for out, n in output_group_comparisons(dirs1, dirs2, out_dir, l1, l2, device=a.device, delta_thresholds=thr,
                                               group_names=a.group_names):
            print("Compared %d events into %s" % (n, out))
        if a.exact_delta_posterior:
            print("Pooled %d events into %s" % output_group_exact_delta(
                dirs1, dirs2, out_dir, delta_thresholds=a.delta_psi_thresholds, group_names=a.group_names)[::-1])
        if a.exact_paired_delta_posterior:
            print("Pooled %d events into %s" % output_group_exact_paired_delta(
                dirs1, dirs2, out_dir, delta_thresholds=a.delta_psi_thresholds, group_names=a.group_names)[::-1])
    elif a.group_labels:
        ap.error("--group-labels goes with --compare-groups")
    if a.summarize_parts:
        samples_dir, index_dir, out_dir = (os.path.abspath(os.path.expanduser(p)) for p in a.summarize_parts)
        print("Summarized %d parts into %s" % part_psi.summarize_parts(samples_dir, index_dir, out_dir, device=a.device)[::-1])
    if a.compare_parts:
        d1, d2, index_dir, out_dir = (os.path.abspath(os.path.expanduser(p)) for p in a.compare_parts)
        print("Compared %d parts into %s" % part_psi.compare_parts(d1, d2, index_dir, out_dir, sample_labels=a.comparison_labels,
                                                                   delta_thresholds=a.delta_psi_thresholds, device=a.device)[::-1])
    if not (a.summarize_samples or a.compare_samples or a.compare_groups or a.diagnose_samples or a.summarize_parts
            or a.compare_parts):
        ap.print_help()
    return 0


if __name__ == "__main__":
    sys.exit(main())
