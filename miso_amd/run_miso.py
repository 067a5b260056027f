"""misopy/run_miso.py for Python 3 and for a GPU: compute Psi for a set of genes / events.

The reference loops `for gene: fetch reads -> MISOSampler.run_sampler` (run_miso.py:34-206), one
C call per event on one CPU core.  A GPU wants thousands of events per launch, so the same steps
are split in two: `collect_gene_events` does everything the reference does per gene up to the
sampler call (index lookup, the read-length sanity check, transcript bounds, fetch, strand /
read-length filters, mate pairing, the minimum-read filter, output path), and
`compute_gene_psi` hands the whole list to `MISOSampler.run_sampler_batch` -- one batch per
launch, one `.miso` file per event, byte layout as in the reference.

    python -m miso_amd.run_miso --compute-gene-psi GENE_IDS INDEXED.pickle BAM OUT --read-len 36
    python -m miso_amd.run_miso --compute-genes-from-file GENES.txt BAM OUT --read-len 36 \
           [--paired-end MEAN SD] [--overhang-len N] [--settings-filename F] [--device D]
           [--seed S] [--first-event-id I]
"""
import os
import sys
import time

import numpy as np

from . import gene_utils, gff_utils, sam_utils
from .settings import Settings

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)
import miso_sampler as miso  # noqa: E402  (flat import: it shares `pysplicing` with its tests)


def collect_gene_events(gene_entries, bamfile, output_dir, read_len, overhang_len,
                        paired_end=None, event_type=None, verbose=True, native=False, entry_offset=0, cache=None):
    """run_miso.py:98-206 up to (not including) sampler.run_sampler, for many genes.
    gene_entries: iterable of (gene_id, indexed_gff_filename).
    Returns (events, info): events = [(reads, gene_obj, output_filename, None, index in gene_entries)] for
    MISOSampler.run_sampler_batch, info = per gene status strings (for logs / tests).
    entry_offset / cache: a long gene list collected piece by piece (compute_gene_psi: the next piece is collected while
    the last one is sampled) -- the entries' numbers go on from entry_offset, the loaded index files are kept in `cache`."""
    settings = Settings.get()
    min_event_reads = Settings.get_min_event_reads()
    strand_rule = Settings.get_strand_param()
    filter_reads = settings.get("filter_reads", True)               # run_miso.py:91-94
    events, info = [], {}
    cache = {} if cache is None else cache
    loaded = cache.setdefault("loaded", {})
    bundles = cache.setdefault("bundles", {})      # index root -> {gene_id: gene_info} from genes_bundle.pickle (or None)
    for entry_no, (gene_id, gff_index_filename) in enumerate(gene_entries, entry_offset):
        root = os.path.dirname(os.path.dirname(gff_index_filename))
        if root not in bundles:
            bpath = os.path.join(root, gff_utils.BUNDLE_BASENAME)
            bundles[root] = gff_utils.load_indexed_gff_file(bpath) if os.path.isfile(bpath) else None
        tx_bounds = None
        ready = cache.get("genes", {}).pop((root, gene_id), None)    # made by preload_genes while the alignments were decoded
        if ready is not None:
            gene_obj, tx_bounds = ready
            gff_genes = {gene_id: {"gene_object": gene_obj}}
        elif bundles[root] is not None and gene_id in bundles[root]:
            gene_obj, tx_bounds = gene_utils.gene_from_compact(bundles[root][gene_id])
            gff_genes = {gene_id: {"gene_object": gene_obj}}
        else:
            if not os.path.exists(gff_index_filename):
                print("Error: No GFF %s" % gff_index_filename)
                info[gene_id] = "no index"
                continue
            if gff_index_filename not in loaded:
                loaded.clear()                                      # one index file at a time, as before
                loaded[gff_index_filename] = gff_utils.load_indexed_gff_file(gff_index_filename)
            gff_genes = loaded[gff_index_filename]
        if gene_id not in gff_genes:
            info[gene_id] = "not in index"
            continue
        gene_info = gff_genes[gene_id]
        gene_obj = gene_info['gene_object']
        # Sanity check: if the isoforms are all shorter than the read, skip (run_miso.py:110-115)
        if all(l < read_len for l in gene_obj.iso_lens):
            if verbose:
                print("All isoforms of %s shorter than %d, so skipping" % (gene_id, read_len))
            info[gene_id] = "isoforms shorter than reads"
            continue
        tx_start, tx_end = tx_bounds or \
            gff_utils.get_inclusive_txn_bounds(gene_info['hierarchy'][gene_id])
        chrom = sam_utils.resolve_chrom(bamfile, gene_obj.chrom)
        if event_type is not None:
            chrom_dir = os.path.join(output_dir, event_type, gene_obj.chrom)
        else:
            chrom_dir = os.path.join(output_dir, gene_obj.chrom)
        miso_basename = os.path.basename(gff_index_filename)
        if not miso_basename.endswith(".pickle"):
            raise ValueError("Error: Invalid index file %s" % gff_index_filename)
        output_filename = os.path.join(chrom_dir, miso_basename[:-len(".pickle")])
        if native:
            # the reads stay in the file: fetch, pairing, filters and the minimum-read rule are
            # applied natively when the sampler adds the event to its batch
            if strand_rule == "fr-secondstrand":
                raise Exception("fr-secondstrand currently unsupported.")     # sam_utils.py:331
            region = miso.AlnRegion(bamfile, chrom, tx_start, tx_end, strand_rule=strand_rule,
                                    target_strand=gene_obj.strand, read_len=read_len,
                                    min_reads=min_event_reads if filter_reads else 0)
            events.append((region, gene_obj, output_filename, None, entry_no))
            info[gene_id] = "region %s:%d-%d" % (chrom, tx_start, tx_end)
            continue
        try:
            reads, num_raw_reads = bamfile.parse_reads(
                chrom, tx_start, tx_end, paired_end=bool(paired_end), strand_rule=strand_rule,
                target_strand=gene_obj.strand, given_read_len=read_len)
        except ValueError:
            if verbose:
                print("Cannot fetch reads in region: %s:%d-%d" % (chrom, tx_start, tx_end))
            reads, num_raw_reads = ((), ()), 0
        if filter_reads and num_raw_reads < min_event_reads:
            if verbose:
                print("Only %d reads in gene, skipping (needed >= %d reads)"
                      % (num_raw_reads, min_event_reads))
            info[gene_id] = "only %d reads" % num_raw_reads
            continue
        events.append((reads, gene_obj, output_filename, None, entry_no))
        info[gene_id] = "%d reads" % num_raw_reads
    return events, info


def preload_genes(gene_entries, cache):
    """The annotation side of collect_gene_events -- index bundles, gene objects, transcript bounds -- for genes that come
    from a bundle, kept in `cache` for it: none of it needs the alignment file, so compute_gene_psi does it WHILE the file
    is being decoded (interpreter work beside native work)."""
    bundles = cache.setdefault("bundles", {})
    genes = cache.setdefault("genes", {})
    for gene_id, gff_index_filename in gene_entries:
        root = os.path.dirname(os.path.dirname(gff_index_filename))
        if root not in bundles:
            bpath = os.path.join(root, gff_utils.BUNDLE_BASENAME)
            bundles[root] = gff_utils.load_indexed_gff_file(bpath) if os.path.isfile(bpath) else None
        b = bundles[root]
        if b is not None and gene_id in b:
            genes[(root, gene_id)] = gene_utils.gene_from_compact(b[gene_id])


def _check_device(device):
    """A worker that was handed a device it cannot open (the dispatcher counted GPUs the process may not use) stops
    here with a clear message and a non-zero exit status instead of failing batch by batch."""
    from . import capi
    n = capi.device_count()
    if not 0 <= int(device) < n:
        raise SystemExit("miso: --device %d, but this process can open %d HIP device(s)" % (int(device), n))


def compute_gene_psi(gene_ids, gff_index_filename, bam_filename, output_dir, read_len,
                     overhang_len, paired_end=None, event_type=None, verbose=True, bamfile=None,
                     seed=None, first_event_id=0, device=None, gene_entries=None,
                     max_events_per_launch=8192, summary_file=None, write_files=True, event_ids=None,
                     diagnostics_file=None, exact=None, exact_paired=None, rank_diagnostics=False, exact_stats_file=None,
                     exact_pairs_file=None, model_check_file=None, part_psi_file=None):
    """run_miso.py:34-206.  `gene_entries` (list of (gene_id, index file)) generalises the
    reference's (gene_ids, one index file) so a whole batch file is one GPU batch.  event_ids[k] (optional): entry k's
    number in the random-number counter (default first_event_id + k).  diagnostics_file: also write the chain
    diagnostics table of this run (diagnostics.py), per launch from the resident samples, merged like the summary parts;
    rank_diagnostics: that table with the six columns of the rank-normalised pass.
    exact: single-end two-isoform events take the exact-posterior mode (None: the settings' `exact` key).
    exact_paired: the same switch for the paired-end two-isoform events of a --paired-end run (None: the settings'
    `exact_paired` key); nothing on a single-end run.
    exact_stats_file (the single-end exact mode only): also write the `.miso_exact_stats` table of the written events
    (compare.write_exact_stats), parts merged like the diagnostics table's.
    exact_pairs_file (the paired exact mode only): also write the `.miso_exact_pairs` table of the written events
    (compare.write_exact_pairs), parts merged the same way.
    model_check_file (single-end only): also write the `.miso_fit` table of this run, the posterior predictive model check
    of every written event (model_check.py), per launch from the resident samples with the run's seed, parts merged the
    same way; nothing else changes with it.
    part_psi_file: also write the `.miso_part_summary` table of this run, the inclusion of every part of the written
    multi-isoform events (part_psi.py), per launch from the resident samples, parts merged the same way; nothing else changes
    with it."""
    if model_check_file is not None and paired_end:
        raise ValueError("the model check takes single-end events only")
    fit_parts = []
    part_parts = []
    exact = Settings.get_exact() if exact is None else bool(exact)
    if exact_stats_file is not None and (paired_end or not exact):
        raise ValueError("the exact statistics table needs the exact-posterior mode (single-end)")
    stat_parts = []
    exact_paired = Settings.get_exact_paired() if exact_paired is None else bool(exact_paired)
    if exact_pairs_file is not None and not (paired_end and exact_paired):
        raise ValueError("the exact pairs table needs the paired exact-posterior mode (paired-end)")
    pair_parts = []
    os.makedirs(output_dir, exist_ok=True)
    if gene_entries is None:
        gene_entries = [(g, gff_index_filename) for g in gene_ids]
    print("Computing Psi for %d genes..." % len(gene_entries))
    print("  - BAM: %s" % bam_filename)
    print("  - Outputting to: %s" % output_dir)
    if paired_end:
        print("  - Paired-end mode: ", paired_end)
    settings_params = Settings.get_sampler_params()
    burn_in, lag = settings_params["burn_in"], settings_params["lag"]
    num_iters, num_chains = settings_params["num_iters"], settings_params["num_chains"]
    if part_psi_file is not None:
        _check_part_psi(settings_params)
    if device is not None:
        _check_device(device)
        os.environ["MISO_DEVICE"] = str(int(device))               # read by pysplicing per launch
    t0 = time.time()
    own = bamfile is None
    import threading
    opened = {}
    if own:      # decoded on a thread of its own (native code), the annotation work of the first stage beside it
        def _open():
            try:
                opened["file"] = sam_utils.load_bam_reads(bam_filename)
            except BaseException as e:
                opened["error"] = e
        opener = threading.Thread(target=_open, daemon=True)
        opener.start()
    if paired_end:
        mean_frag_len = int(paired_end[0])
        frag_variance = np.power(int(paired_end[1]), 2)             # run_miso.py:80-83
    # Four stages, each on a thread of its own, a chunk of genes in each (round 6; round 5 collected the whole list
    # first and ran launch -> headers -> files of a batch on one thread: 3.5 of a 40 000-event run's 6.9 s):
    #   collect   index lookup, gene objects, regions (Python)                          this function's producer thread
    #   prepare   the regions' reads out of the decoded alignment file into a batch (native, parallel)    main thread
    #   launch    upload, sample, download (native; the GPU)                                               `gpu` thread
    #   output    header lines, .miso files, summary rows (native formatting and writing)                   `out` thread
    # Nothing here changes anybody's random stream: every event carries its number in the caller's gene list.
    import queue
    from concurrent.futures import ThreadPoolExecutor
    chunks = queue.Queue(maxsize=2)
    info, n_events, t_collect = {}, [0], [0.0]
    failure = []

    t_prepare = [0.0]

    def producer():
        nonlocal bamfile
        cache = {}
        try:
            if own:
                tc = time.time()
                preload_genes(gene_entries, cache)
                t_collect[0] += time.time() - tc
                opener.join()
                if "error" in opened:
                    raise opened["error"]
                bamfile = opened["file"]
                if os.environ.get("MISO_TIMING"):
                    print("[miso] alignment file open %.2f s after the start, gene objects made beside it in %.2f s"
                          % (time.time() - t0, t_collect[0]))
            for lo in range(0, len(gene_entries), max_events_per_launch):
                tc = time.time()
                evs, inf = collect_gene_events(gene_entries[lo:lo + max_events_per_launch], bamfile, output_dir, read_len,
                                               overhang_len, paired_end=paired_end, event_type=event_type,
                                               verbose=verbose, native=True, entry_offset=lo, cache=cache)
                t_collect[0] += time.time() - tc
                info.update(inf)
                n_events[0] += len(evs)
                chunks.put((lo, evs))
        except BaseException as e:       # the consumer must not wait for a chunk that will never come
            failure.append(e)
        finally:
            chunks.put(None)

    threading.Thread(target=producer, daemon=True).start()
    written = []
    summary_parts = []
    diag_parts = []
    with ThreadPoolExecutor(1) as gpu, ThreadPoolExecutor(1) as out:
        in_flight = []       # output futures, oldest first: at most two batches behind the one being prepared
        while True:
            item = chunks.get()
            if item is None:
                break
            lo, chunk = item
            if not chunk:
                continue
            # sampler parameters as in run_miso.py:151-171 (num_isoforms only sizes an unused matrix)
            if paired_end:
                params = miso.get_paired_end_sampler_params(2, mean_frag_len, frag_variance, read_len,
                                                            overhang_len=overhang_len)
                if exact_paired:
                    params["exact_paired"] = 1     # miso_sampler.py prepare_batch
            else:
                params = miso.get_single_end_sampler_params(2, read_len, overhang_len)
                if exact:
                    params["exact"] = 1     # miso_sampler.py prepare_batch
                if model_check_file is not None:
                    params["model_check"] = 1
            sampler = miso.MISOSampler(params, paired_end=bool(paired_end), log_dir=output_dir)
            # every event keeps the number it has in the caller's gene list: skipped genes, chunking
            # and the number of GPUs do not change anybody's random stream
            chunk = [ev[:4] + (_event_number(ev[4], first_event_id, event_ids),) for ev in chunk]
            tp = time.time()
            state = sampler.prepare_batch(num_iters, chunk, num_chains=num_chains, burn_in=burn_in,
                                          lag=lag, verbose=verbose)
            t_prepare[0] += time.time() - tp
            while len(in_flight) >= 2:
                written += in_flight.pop(0).result()
            part = None if summary_file is None else "%s.part%06d" % (summary_file, lo)
            if part:
                summary_parts.append(part)
            dpart = None if diagnostics_file is None else "%s.part%06d" % (diagnostics_file, lo)
            if dpart:
                diag_parts.append(dpart)
            spart = None if exact_stats_file is None else "%s.part%06d" % (exact_stats_file, lo)
            if spart:
                stat_parts.append(spart)
            ppart = None if exact_pairs_file is None else "%s.part%06d" % (exact_pairs_file, lo)
            if ppart:
                pair_parts.append(ppart)
            fpart = None if model_check_file is None else "%s.part%06d" % (model_check_file, lo)
            if fpart:
                fit_parts.append(fpart)
            qpart = None if part_psi_file is None else "%s.part%06d" % (part_psi_file, lo)
            if qpart:
                part_parts.append(qpart)
            launched = gpu.submit(sampler.launch_batch, state, seed=seed, first_event_id=first_event_id + lo)

            def outputs(sampler=sampler, state=state, launched=launched, part=part, dpart=dpart, spart=spart, ppart=ppart,
                        fpart=fpart, qpart=qpart):
                launched.result()
                return sampler.output_batch(state, verbose=verbose, summary_file=part, write_files=write_files,
                                            diagnostics_file=dpart, rank_diagnostics=rank_diagnostics, exact_stats_file=spart,
                                            exact_pairs_file=ppart, model_fit_file=fpart, part_psi_file=qpart)
            in_flight.append(out.submit(outputs))
        for f in in_flight:
            written += f.result()
    if failure:
        raise failure[0]
    t1 = t0 + t_collect[0]
    if summary_file is not None:
        merge_tables(summary_parts, summary_file)
    if diagnostics_file is not None:
        merge_tables(diag_parts, diagnostics_file)
    if exact_stats_file is not None:
        merge_tables(stat_parts, exact_stats_file)
    if exact_pairs_file is not None:
        merge_tables(pair_parts, exact_pairs_file)
    if model_check_file is not None:
        merge_tables(fit_parts, model_check_file)
    if part_psi_file is not None:
        _merge_part_tables(part_parts, part_psi_file)
    t2 = time.time()
    if verbose:
        print("Collected %d events in %.2f s (beside the decoding / sampling), batches prepared in %.2f s, whole run %.2f s"
              % (n_events[0], t1 - t0, t_prepare[0], t2 - t0))
    if own:
        bamfile.close()
    return written, info


def _merge_part_tables(parts, filename):
    """merge_tables for a part-level table (part_psi.py), then the one order such a table has: by event name"""
    from . import part_psi
    return part_psi.sort_table(merge_tables(parts, filename))


def _check_part_psi(p):
    """The sampler settings' samples per event must suit the isoform-group passes: refused before anything is sampled"""
    from . import part_psi
    why = part_psi.samples_refusal(p["num_chains"] * (p["num_iters"] - p["burn_in"]) // p["lag"])
    if why:
        raise ValueError(why)


def _event_number(k, first_event_id, event_ids):
    """Entry k's id in the random-number counter: its number in the whole gene list."""
    return first_event_id + k if event_ids is None else int(event_ids[k])


def merge_tables(parts, filename, remove=True):
    """Concatenate tab-separated tables that share a header line (per-batch / per-GPU parts)."""
    os.makedirs(os.path.dirname(os.path.abspath(filename)), exist_ok=True)
    header_done = False
    with open(filename, "w") as out:
        for part in parts:
            if not os.path.isfile(part):
                continue
            with open(part) as f:
                header = f.readline()
                if not header_done:
                    out.write(header)
                    header_done = True
                for line in f:
                    out.write(line)
            if remove:
                os.remove(part)
    return filename


def compare_gene_psi(gene_entries, bam1_filename, bam2_filename, output_dir1, output_dir2,
                     comparison_file, read_len, overhang_len, paired_end=None, event_type=None,
                     verbose=True, seed=None, first_event_id=0, device=None,
                     max_events_per_launch=4096, event_ids=None, samples=None, diagnostics_files=None, exact=None,
                     exact_comparison_file=None, delta_thresholds=None, exact_paired=None, rank_diagnostics=False,
                     delta_posterior_file=None, exact_delta_file=None, exact_stats_files=None, model_check_files=None,
                     part_psi_files=None):
    """Two RNA-seq samples over the same genes in one go (BASELINE configs[4]): both samples are
    sampled on this GPU, their `.miso` files written like two `miso --run`s would, and the
    `.miso_bf` table of `compare_miso` (hypothesis_test.py:186-345) comes from Bayes factors
    computed on the device while the samples are still in HBM.
    event_ids[k]: as for compute_gene_psi.  samples[k] (`miso --run --compare --prefilter`): the samples whose
    coverage filter entry k passes, "1", "2" or "1,2".  An entry is collected only in those samples; one that passes
    in one sample only is sampled there alone (with that sample's seed) and is not compared.
    diagnostics_files: (file1, file2), each sample's chain diagnostics table (diagnostics.py), parts merged like the
    comparison's; rank_diagnostics: with the six columns of the rank-normalised pass.
    exact_comparison_file (the exact mode only): the `.miso_bf_exact` table of the exact comparison (compare.py
    write_exact_comparison), parts merged like the comparison's; delta_thresholds: its thresholds t of P(|delta psi| >= t).
    delta_posterior_file (any mode): the `.miso_dpsi` table of delta psi over all pairs of the two samples' draws (compare.py
    write_dpsi), parts merged like the comparison's, with the same delta_thresholds.
    exact_delta_file (with exact_comparison_file only): the `.miso_dpsi_exact` table of delta psi's median and credible
    interval from the exact CDF (compare.py write_exact_dpsi), parts merged like the exact comparison's.
    exact_stats_files (the single-end exact mode only): (file1, file2), each sample's `.miso_exact_stats` table
    (compare.py write_exact_stats), parts merged like the diagnostics tables'.
    model_check_files (single-end only): (file1, file2), each sample's `.miso_fit` table (model_check.py), each drawn with its
    sample's seed, parts merged like the diagnostics tables'.
    part_psi_files (any mode): (file1, file2, file_d), each sample's `.miso_part_summary` table and the `.miso_part_dpsi` table
    of the compared events (part_psi.py), with the same delta_thresholds; parts merged, then in event-name order."""
    if exact_delta_file is not None and exact_comparison_file is None:
        raise ValueError("the exact delta psi table goes with the exact comparison")
    for d in (output_dir1, output_dir2):
        os.makedirs(d, exist_ok=True)
    if device is not None:
        _check_device(device)
        os.environ["MISO_DEVICE"] = str(int(device))
    exact = Settings.get_exact() if exact is None else bool(exact)
    exact_paired = Settings.get_exact_paired() if exact_paired is None else bool(exact_paired)
    if exact_comparison_file is not None and paired_end and not exact_paired:
        raise ValueError("the exact comparison of paired-end samples needs the paired exact-posterior mode")
    if exact_comparison_file is not None and not paired_end and not exact:
        raise ValueError("the exact comparison needs the exact-posterior mode (single-end)")
    if exact_stats_files is not None and (paired_end or not exact):
        raise ValueError("the exact statistics tables need the exact-posterior mode (single-end)")
    stat_parts = ([], [])
    if model_check_files is not None and paired_end:
        raise ValueError("the model check takes single-end events only")
    fit_parts = ([], [])
    part_parts = ([], [], [])
    p = Settings.get_sampler_params()
    if part_psi_files is not None:
        _check_part_psi(p)
    bam1, bam2 = sam_utils.load_bam_reads(bam1_filename), sam_utils.load_bam_reads(bam2_filename)
    evs = []
    for which, bam, out in (("1", bam1, output_dir1), ("2", bam2, output_dir2)):
        ks = [k for k in range(len(gene_entries)) if samples is None or which in samples[k].split(",")]
        ev, _ = collect_gene_events([gene_entries[k] for k in ks], bam, out, read_len, overhang_len,
                                    paired_end=paired_end, event_type=event_type, verbose=verbose)
        evs.append([e[:4] + (ks[e[4]],) for e in ev])        # numbered in gene_entries
    ev1, ev2 = evs
    # pair by gene: only genes that passed the filters in BOTH samples are compared
    # (compare_miso leaves out events missing from one directory, hypothesis_test.py:262-264)
    by_no2 = {e[4]: e for e in ev2}
    pairs = [(a, by_no2[a[4]]) for a in ev1 if a[4] in by_no2]
    parts = []
    xparts = []
    eparts = []
    dpsi_parts = []
    diag_parts = ([], [])
    if paired_end:
        mean_frag_len = int(paired_end[0])
        frag_variance = np.power(int(paired_end[1]), 2)
    for lo in range(0, len(pairs), max_events_per_launch):
        chunk = pairs[lo:lo + max_events_per_launch]
        if paired_end:
            params = miso.get_paired_end_sampler_params(2, mean_frag_len, frag_variance, read_len,
                                                        overhang_len=overhang_len)
            if exact_paired:
                params["exact_paired"] = 1     # miso_sampler.py prepare_batch
        else:
            params = miso.get_single_end_sampler_params(2, read_len, overhang_len)
            if exact:
                params["exact"] = 1     # miso_sampler.py prepare_batch
        sampler = miso.MISOSampler(params, paired_end=bool(paired_end), log_dir=output_dir1)
        part = "%s.part%06d" % (comparison_file, lo)
        parts.append(part)
        dparts = None
        if diagnostics_files is not None:
            dparts = tuple("%s.part%06d" % (f, lo) for f in diagnostics_files)
            for which in (0, 1):
                diag_parts[which].append(dparts[which])
        fparts = None
        if model_check_files is not None:
            fparts = tuple("%s.part%06d" % (f, lo) for f in model_check_files)
            for which in (0, 1):
                fit_parts[which].append(fparts[which])
        sparts = None
        if exact_stats_files is not None:
            sparts = tuple("%s.part%06d" % (f, lo) for f in exact_stats_files)
            for which in (0, 1):
                stat_parts[which].append(sparts[which])
        qparts = None
        if part_psi_files is not None:
            qparts = tuple("%s.part%06d" % (f, lo) for f in part_psi_files)
            for which in (0, 1, 2):
                part_parts[which].append(qparts[which])
        xpart = None
        if exact_comparison_file is not None:
            xpart = "%s.part%06d" % (exact_comparison_file, lo)
            xparts.append(xpart)
        epart = None
        if exact_delta_file is not None:
            epart = "%s.part%06d" % (exact_delta_file, lo)
            eparts.append(epart)
        dpsi_part = None
        if delta_posterior_file is not None:
            dpsi_part = "%s.part%06d" % (delta_posterior_file, lo)
            dpsi_parts.append(dpsi_part)
        sampler.run_comparison_batch(p["num_iters"], [a[:3] for a, _ in chunk],
                                     [b[:3] for _, b in chunk], part, num_chains=p["num_chains"],
                                     burn_in=p["burn_in"], lag=p["lag"], seed=seed,
                                     first_event_id=first_event_id + lo, verbose=verbose,
                                     event_ids=[_event_number(a[4], first_event_id, event_ids) for a, _ in chunk],
                                     diagnostics_files=dparts, exact_comparison_file=xpart,
                                     delta_thresholds=delta_thresholds, rank_diagnostics=rank_diagnostics,
                                     delta_posterior_file=dpsi_part, exact_delta_file=epart, exact_stats_files=sparts,
                                     model_fit_files=fparts, part_psi_files=qparts)
    merge_tables(parts, comparison_file)
    if delta_posterior_file is not None:
        merge_tables(dpsi_parts, delta_posterior_file)
    if exact_comparison_file is not None:
        merge_tables(xparts, exact_comparison_file)
    if exact_delta_file is not None:
        merge_tables(eparts, exact_delta_file)
    if samples is not None:
        # sample 2's stream: the seed MISOCompareBatch derives for it (pysplicingmodule.c)
        seed2 = None if seed is None else (int(seed) ^ 0x5851F42D4C957F2D) & 0xFFFFFFFFFFFFFFFF
        for which, ev, out, s in (("1", ev1, output_dir1, seed), ("2", ev2, output_dir2, seed2)):
            alone = [e[:4] + (_event_number(e[4], first_event_id, event_ids),) for e in ev if samples[e[4]] == which]
            if not alone:
                continue
            if paired_end:
                params = miso.get_paired_end_sampler_params(2, mean_frag_len, frag_variance, read_len,
                                                            overhang_len=overhang_len)
                if exact_paired:
                    params["exact_paired"] = 1     # miso_sampler.py prepare_batch
            else:
                params = miso.get_single_end_sampler_params(2, read_len, overhang_len)
                if exact:
                    params["exact"] = 1     # miso_sampler.py prepare_batch
                if model_check_files is not None:
                    params["model_check"] = 1
            sampler = miso.MISOSampler(params, paired_end=bool(paired_end), log_dir=out)
            dpart = None
            if diagnostics_files is not None:
                dpart = "%s.alone" % diagnostics_files[int(which) - 1]
                diag_parts[int(which) - 1].append(dpart)
            spart = None
            if exact_stats_files is not None:
                spart = "%s.alone" % exact_stats_files[int(which) - 1]
                stat_parts[int(which) - 1].append(spart)
            fpart = None
            if model_check_files is not None:
                fpart = "%s.alone" % model_check_files[int(which) - 1]
                fit_parts[int(which) - 1].append(fpart)
            qpart = None
            if part_psi_files is not None:
                qpart = "%s.alone" % part_psi_files[int(which) - 1]
                part_parts[int(which) - 1].append(qpart)
            sampler.run_sampler_batch(p["num_iters"], alone, num_chains=p["num_chains"], burn_in=p["burn_in"],
                                      lag=p["lag"], seed=s, verbose=verbose, diagnostics_file=dpart,
                                      rank_diagnostics=rank_diagnostics, exact_stats_file=spart, model_fit_file=fpart,
                                      part_psi_file=qpart)
    if diagnostics_files is not None:
        for which in (0, 1):
            merge_tables(diag_parts[which], diagnostics_files[which])
    if exact_stats_files is not None:
        for which in (0, 1):
            merge_tables(stat_parts[which], exact_stats_files[which])
    if model_check_files is not None:
        for which in (0, 1):
            merge_tables(fit_parts[which], model_check_files[which])
    if part_psi_files is not None:
        for which in (0, 1, 2):
            _merge_part_tables(part_parts[which], part_psi_files[which])
    return len(pairs)


def read_genes_file(genes_filename):
    """Two-column, tab-delimited: gene ID, indexed GFF file (run_miso.py:236-250)."""
    return read_genes_file_columns(genes_filename)[0]


def read_genes_file_columns(genes_filename):
    """A batch file with its optional columns (`miso --run --prefilter`): 3rd the gene's number in the whole gene list,
    4th the samples whose coverage filter it passes.  Returns (entries, numbers or None, samples or None); a column is
    given for every line or for none."""
    entries, numbers, samples = [], [], []
    with open(genes_filename) as genes_in:
        for line in genes_in:
            if not line.strip():
                continue
            fields = line.strip().split("\t")
            if len(fields) not in (2, 3, 4):
                raise ValueError("%s: a batch file line has 2 to 4 columns: %r" % (genes_filename, line))
            entries.append((fields[0], fields[1]))
            if len(fields) > 2:
                numbers.append(int(fields[2]))
            if len(fields) > 3:
                samples.append(fields[3])
    for col in (numbers, samples):
        if col and len(col) != len(entries):
            raise ValueError("%s: optional columns must be given on every line" % genes_filename)
    return entries, numbers or None, samples or None


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="MISO (Mixture of Isoforms model) on MI355X")
    ap.add_argument("--compute-gene-psi", nargs=4, metavar=("GENE_IDS", "INDEX", "BAM", "OUT"))
    ap.add_argument("--compute-genes-from-file", nargs=3, metavar=("GENES_FILE", "BAM", "OUT"))
    ap.add_argument("--compare-genes-from-file", nargs=6,
                    metavar=("GENES_FILE", "BAM1", "BAM2", "OUT1", "OUT2", "BF_FILE"),
                    help="sample both RNA-seq samples and write the Bayes-factor table")
    ap.add_argument("--summary-file", default=None,
                    help="also write the summarize_miso table of this run (device-side summaries)")
    ap.add_argument("--diagnostics-file", default=None,
                    help="also write the chain diagnostics table of this run (split R-hat, ESS, MCSE; device-side)")
    ap.add_argument("--diagnostics-files", nargs=2, default=None, metavar=("FILE1", "FILE2"),
                    help="with --compare-genes-from-file: the chain diagnostics table of each sample")
    ap.add_argument("--rank-diagnostics", action="store_true",
                    help="with --diagnostics-file(s): six more columns from the rank-normalised pass")
    ap.add_argument("--model-check-file", default=None, metavar="F",
                    help="with --compute-genes-from-file, single-end: also write the `.miso_fit` table of this run, per event the "
                         "posterior predictive check of its reads against the model's read classes (device-side)")
    ap.add_argument("--model-check-files", nargs=2, default=None, metavar=("FILE1", "FILE2"),
                    help="with --compare-genes-from-file, single-end: that table of each sample")
    ap.add_argument("--part-psi-file", default=None, metavar="F",
                    help="with --compute-genes-from-file: also write the `.miso_part_summary` table of this run, per part (exon) "
                         "of every multi-isoform event the mean and credible interval of its inclusion (device-side)")
    ap.add_argument("--part-psi-files", nargs=3, default=None, metavar=("FILE1", "FILE2", "FILE_D"),
                    help="with --compare-genes-from-file: that table of each sample, and the `.miso_part_dpsi` table of the parts' "
                         "delta psi over all pairs of the two samples' draws (thresholds: --delta-psi-thresholds)")
    ap.add_argument("--no-miso-files", action="store_true",
                    help="with --summary-file: only the table, no per-event .miso files")
    ap.add_argument("--exact", action="store_true",
                    help="single-end two-isoform events: independent draws from the exact posterior of Psi instead of chains "
                         "(also the settings key `exact`)")
    ap.add_argument("--exact-paired", action="store_true",
                    help="with --paired-end: paired-end two-isoform events draw independently from the exact posterior of Psi "
                         "instead of running chains (also the settings key `exact_paired`)")
    ap.add_argument("--exact-stats-file", default=None, metavar="F",
                    help="with --compute-genes-from-file and the exact mode (single-end): also write the `.miso_exact_stats` "
                         "table, per event the seven statistics its exact posterior is made of")
    ap.add_argument("--exact-stats-files", nargs=2, default=None, metavar=("FILE1", "FILE2"),
                    help="with --compare-genes-from-file and the exact mode (single-end): that table of each sample")
    ap.add_argument("--exact-pairs-file", default=None, metavar="F",
                    help="with --compute-genes-from-file and the paired exact mode (--paired-end, --exact-paired): also write the "
                         "`.miso_exact_pairs` table, per event the six statistics and the drawing pairs' probabilities its exact "
                         "posterior is made of (in the order of 10 bytes a pair)")
    ap.add_argument("--exact-comparison-file", default=None, metavar="F",
                    help="with --compare-genes-from-file and the exact mode: also write the exact comparison's table "
                         "(Bayes factors and P(|delta psi| >= T) from the posteriors' tables, no sampling error)")
    ap.add_argument("--exact-delta-file", default=None, metavar="F",
                    help="with --exact-comparison-file: also write the table of delta psi's median and 95 %% credible interval, "
                         "P(delta psi > 0) and P(|delta psi| >= T) from the exact CDF of delta psi (no sampling error)")
    ap.add_argument("--delta-psi-thresholds", nargs="+", type=float, default=None, metavar="T",
                    help="the thresholds T of --exact-comparison-file and --delta-posterior-file, each in (0, 1), at most four "
                         "(default 0.1 0.2)")
    ap.add_argument("--delta-posterior-file", default=None, metavar="F",
                    help="with --compare-genes-from-file, any mode: also write the table of delta psi over all pairs of the two "
                         "samples' draws (median, credible interval, P(delta psi > 0), P(|delta psi| >= T))")
    ap.add_argument("--paired-end", nargs=2, type=float, metavar=("MEAN", "SD"))
    ap.add_argument("--read-len", type=int)
    ap.add_argument("--overhang-len", type=int)
    ap.add_argument("--event-type", default=None)
    ap.add_argument("--settings-filename", default=None)
    ap.add_argument("--device", type=int, default=None, help="HIP device of this process")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--first-event-id", type=int, default=0,
                    help="global index of this shard's first event (results do not depend on sharding)")
    a = ap.parse_args(argv)
    Settings.load(a.settings_filename)
    if a.read_len is None:
        print("Error: must provide --read-len.")
        return 1
    overhang_len = a.overhang_len if a.overhang_len is not None else 1
    paired_end = tuple(a.paired_end) if a.paired_end else None
    if (a.model_check_file or a.model_check_files) and paired_end:
        ap.error("--model-check-file(s): the model check is single-end only (a paired-end read's class is compatibility x "
                 "fragment length)")
    if a.model_check_file and not a.compute_genes_from_file:
        ap.error("--model-check-file goes with --compute-genes-from-file")
    if a.model_check_files and not a.compare_genes_from_file:
        ap.error("--model-check-files goes with --compare-genes-from-file")
    if a.part_psi_file and not a.compute_genes_from_file:
        ap.error("--part-psi-file goes with --compute-genes-from-file")
    if a.part_psi_files and not a.compare_genes_from_file:
        ap.error("--part-psi-files goes with --compare-genes-from-file")
    if a.part_psi_file or a.part_psi_files:
        try:
            _check_part_psi(Settings.get_sampler_params())
        except ValueError as err:
            ap.error("--part-psi-file(s): %s" % err)
    exact = bool(a.exact) or Settings.get_exact()       # the flag, or `exact = True` under [sampler] of the settings file
    if a.exact_paired and not paired_end:
        ap.error("--exact-paired goes with --paired-end")
    exact_paired = bool(paired_end) and (bool(a.exact_paired) or Settings.get_exact_paired())
    if a.diagnostics_file and not a.compute_genes_from_file:
        print("Error: --diagnostics-file goes with --compute-genes-from-file.")
        return 1
    if a.diagnostics_files and not a.compare_genes_from_file:
        print("Error: --diagnostics-files goes with --compare-genes-from-file.")
        return 1
    if a.rank_diagnostics and not (a.diagnostics_file or a.diagnostics_files):
        print("Error: --rank-diagnostics goes with --diagnostics-file or --diagnostics-files.")
        return 1
    if a.exact_comparison_file is not None:
        if paired_end and a.compare_genes_from_file:
            if not exact_paired:
                print("Error: --exact-comparison-file with --paired-end needs the paired exact mode (--exact-paired).")
                return 1
        elif not a.compare_genes_from_file or paired_end or not exact:
            print("Error: --exact-comparison-file goes with --compare-genes-from-file and the exact mode (single-end).")
            return 1
    if a.exact_delta_file is not None and a.exact_comparison_file is None:
        print("Error: --exact-delta-file goes with --exact-comparison-file.")
        return 1
    if a.exact_stats_file is not None and (not a.compute_genes_from_file or paired_end or not exact):
        print("Error: --exact-stats-file goes with --compute-genes-from-file and the exact mode (single-end).")
        return 1
    if a.exact_stats_files is not None and (not a.compare_genes_from_file or paired_end or not exact):
        print("Error: --exact-stats-files goes with --compare-genes-from-file and the exact mode (single-end).")
        return 1
    if a.exact_pairs_file is not None and (not a.compute_genes_from_file or not exact_paired):
        print("Error: --exact-pairs-file goes with --compute-genes-from-file and the paired exact mode (--paired-end, --exact-paired).")
        return 1
    if a.delta_posterior_file is not None and not a.compare_genes_from_file:
        print("Error: --delta-posterior-file goes with --compare-genes-from-file.")
        return 1
    if a.delta_psi_thresholds is not None:
        try:
            miso.compare.check_delta_thresholds(a.delta_psi_thresholds)
        except ValueError as err:
            print(err)
            return 1
    if a.compare_genes_from_file:
        genes_filename, bam1, bam2, out1, out2, bf = (os.path.abspath(os.path.expanduser(x))
                                                     for x in a.compare_genes_from_file)
        entries, numbers, samples = read_genes_file_columns(genes_filename)
        n = compare_gene_psi(entries, bam1, bam2, out1, out2, bf, a.read_len, overhang_len,
                             paired_end=paired_end, event_type=a.event_type, seed=a.seed,
                             first_event_id=a.first_event_id, device=a.device, event_ids=numbers,
                             samples=samples, diagnostics_files=a.diagnostics_files, exact=exact,
                             exact_comparison_file=(os.path.abspath(os.path.expanduser(a.exact_comparison_file))
                                                    if a.exact_comparison_file else None),
                             delta_thresholds=a.delta_psi_thresholds, exact_paired=exact_paired,
                             rank_diagnostics=a.rank_diagnostics,
                             delta_posterior_file=(os.path.abspath(os.path.expanduser(a.delta_posterior_file))
                                                   if a.delta_posterior_file else None),
                             exact_delta_file=(os.path.abspath(os.path.expanduser(a.exact_delta_file))
                                               if a.exact_delta_file else None),
                             exact_stats_files=a.exact_stats_files, model_check_files=a.model_check_files,
                             part_psi_files=a.part_psi_files)
        print("Compared %d genes" % n)
    elif a.compute_genes_from_file:
        genes_filename, bam_filename, output_dir = (os.path.abspath(os.path.expanduser(p))
                                                    for p in a.compute_genes_from_file)
        for p in (genes_filename, bam_filename):
            if not os.path.isfile(p):
                print("Error: %s does not exist." % p)
                return 1
        entries, numbers, _ = read_genes_file_columns(genes_filename)
        compute_gene_psi(None, None, bam_filename, output_dir, a.read_len, overhang_len,
                         paired_end=paired_end, event_type=a.event_type, gene_entries=entries,
                         seed=a.seed, first_event_id=a.first_event_id, device=a.device, event_ids=numbers,
                         summary_file=a.summary_file,
                         write_files=not (a.no_miso_files and a.summary_file),
                         diagnostics_file=a.diagnostics_file, exact=exact, exact_paired=exact_paired,
                         rank_diagnostics=a.rank_diagnostics, exact_stats_file=a.exact_stats_file,
                         exact_pairs_file=a.exact_pairs_file, model_check_file=a.model_check_file,
                         part_psi_file=a.part_psi_file)
        print("Processed %d genes" % len(entries))
    elif a.compute_gene_psi:
        gene_ids = a.compute_gene_psi[0].split(",")
        gff_filename, bam_filename, output_dir = (os.path.abspath(os.path.expanduser(p))
                                                  for p in a.compute_gene_psi[1:])
        compute_gene_psi(gene_ids, gff_filename, bam_filename, output_dir, a.read_len,
                         overhang_len, paired_end=paired_end, event_type=a.event_type,
                         seed=a.seed, first_event_id=a.first_event_id, device=a.device, exact=exact,
                         exact_paired=exact_paired)
    else:
        ap.print_help()
    return 0


if __name__ == "__main__":
    sys.exit(main())
