"""misopy/miso.py (`miso --run`) for Python 3 and GPUs.

    python -m miso_amd.miso --run INDEXED_GFF_DIR ALIGNMENTS.bam --output-dir OUT --read-len 36 \
           [--paired-end MEAN SD] [--overhang-len N] [--settings-filename F] [--event-type T]
           [-p N_GPUS] [--seed S] [--prefilter]

The reference's GenesDispatcher (miso.py:69-337) splits the gene list into `num_processors`
chunks (cluster_utils.chunk_list) and runs `run_miso.py --compute-genes-from-file` on each in its
own process, one CPU core per process.  Here a chunk is a GPU: `-p N` = number of GPUs of this
node (default: all visible), one child process per GPU, each sampling its contiguous chunk as GPU
batches; no communication between them.  Every event keeps its GLOBAL index in the Philox counter
(`--first-event-id`), so the .miso files do not depend on N.  Cluster submission (`--use-cluster`,
SGE) is outside the path and not provided.

`--prefilter` (miso.py:379-404, run_events_analysis.py:28-68) counts the records of the alignment file that lie whole
inside the index's genes (`genes.gff`) on the GPU instead of with bedtools (exon_utils.get_bam_gff_coverage,
csrc/kernels_coverage.hip), in a short-lived child process: the dispatcher itself never initialises HIP.  Only the
genes with at least min_event_reads are dispatched, each with its number in the whole gene list (a third column of the
batch files), so a kept gene's .miso file is the one a run without --prefilter writes.
"""
import os
import subprocess
import sys
import time

from . import gff_utils
from .settings import Settings


def chunk_list(seq, num):
    """cluster_utils.py:23-32."""
    avg = len(seq) / float(num)
    out = []
    last = 0.0
    while last < len(seq):
        out.append(seq[int(last):int(last + avg)])
        last += avg
    return out


def _kfd_gpu_nodes():
    """GPU nodes of the KFD topology: every GPU of the HOST, including ones this process may not open (a container's
    device cgroup, render-node permissions, a 1-GPU lease on an 8-GPU box) -- an upper bound, never the answer."""
    nodes = "/sys/class/kfd/kfd/topology/nodes"
    n = 0
    try:
        for d in os.listdir(nodes):
            props = dict(line.split()[:2] for line in open(os.path.join(nodes, d, "properties")) if line.strip())
            if int(props.get("simd_count", "0")) > 0:
                n += 1
    except (OSError, ValueError):
        return None
    return n


def visible_gpus():
    """GPUs this run may use, WITHOUT initialising HIP in the dispatcher (it only starts worker
    processes; a parent that holds a GPU context and forks is the fragile pattern bench.py avoids):
    HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES if set, else a short-lived child process asks the runtime -- it
    reports the devices this process can really open.  The KFD topology (all GPUs of the host) only caps that
    answer, or stands in when the child cannot be started."""
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            return len([x for x in v.split(",") if x.strip() != ""])
    code = "import sys; sys.path.insert(0, %r); import pysplicing; print(int(pysplicing.deviceCount()))" \
        % os.path.dirname(os.path.abspath(__file__))
    kfd = _kfd_gpu_nodes()
    try:
        out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                             text=True, timeout=120)
        n = int(out.stdout.strip().splitlines()[-1])
        return n if kfd is None else min(n, kfd) if kfd > 0 else n
    except (OSError, ValueError, IndexError, subprocess.SubprocessError):
        return kfd or 0


class PrefilterError(Exception):
    """No event passes the coverage filter, or the coverage pass failed: nothing is dispatched."""


def _coverage_child(bam_filename, gff_filename, output_filename):
    """The coverage pass of --prefilter, forked from the dispatcher: on GPU 0, over the alignments the dispatcher
    decoded when it did (inherited), else over the file opened here; writes the table and exits."""
    rc = 1
    try:
        from . import exon_utils, sam_utils
        bamfile = sam_utils._PRELOADED.get(os.path.abspath(os.path.expanduser(bam_filename)))
        exon_utils.compute_bam_gff_coverage(bam_filename, gff_filename, output_filename, bamfile=bamfile, device=0)
        rc = 0
    except BaseException:
        import traceback
        traceback.print_exc()
    finally:
        sys.stdout.flush(); sys.stderr.flush()
        os._exit(rc)


def _forked_worker(argv, log, worker_no=0, n_workers=1):
    """One worker of `miso --run`, forked from the dispatcher: output to its log file, its share of the
    host cores (the native stages -- read collection, CIGAR parsing, `.miso` formatting -- size their
    thread pools by the affinity mask: N workers with all cores each would oversubscribe N-fold), then
    run_miso.main on this process's own GPU (the dispatcher never touched the GPU runtime)."""
    fd = os.open(log, os.O_WRONLY | os.O_CREAT | os.O_APPEND, 0o644)
    if n_workers > 1:
        try:
            cores = sorted(os.sched_getaffinity(0))
            mine = cores[worker_no::n_workers] or cores
            os.sched_setaffinity(0, mine)
        except (AttributeError, OSError):
            pass
    sys.stdout.flush(); sys.stderr.flush()
    os.dup2(fd, 1); os.dup2(fd, 2)
    rc = 1
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        if root not in sys.path:
            sys.path.insert(0, root)
        from . import run_miso
        rc = run_miso.main(argv)
    except BaseException:
        import traceback
        traceback.print_exc()
    finally:
        sys.stdout.flush(); sys.stderr.flush()
        os._exit(rc if isinstance(rc, int) else 1)


class GenesDispatcher(object):
    """miso.py:69-337, with GPUs for processors."""

    def __init__(self, gff_dir, bam_filename, output_dir, read_len, overhang_len,
                 settings_fname=None, paired_end=None, gene_ids=None, num_proc=None,
                 event_type=None, seed=None, summarize=False, compare_bam=None,
                 labels=("sample1", "sample2"), summary_only=False, prefilter=False, diagnostics=False, exact=False,
                 exact_compare=False, delta_thresholds=None, exact_paired=False, rank_diagnostics=False,
                 delta_posterior=False, exact_delta_posterior=False, exact_stats=False, exact_paired_stats=False,
                 model_check=False, part_psi=False):
        # --part-psi: beside the outputs the `.miso_part_summary` table (part_psi.py) of every directory of `.miso` files and,
        # with --compare, `<l1>_vs_<l2>.miso_part_dpsi` beside the `.miso_bf`; merged like a diagnostics table, then sorted
        self.part_psi = bool(part_psi)
        # --model-check: beside the outputs the `.miso_fit` table (model_check.py) of every directory of `.miso` files, merged
        # like a diagnostics table; single-end only
        self.model_check = bool(model_check)
        if self.model_check and paired_end is not None:
            raise ValueError("--model-check is single-end only")
        # --exact-stats: beside the outputs the `.miso_exact_stats` table (compare.py) of every directory of `.miso` files,
        # merged like a diagnostics table
        self.exact_stats = bool(exact_stats)
        # --exact-paired-stats: the same for the paired exact mode, the `.miso_exact_pairs` table (no --compare)
        self.exact_paired_stats = bool(exact_paired_stats)
        self.exact_paired = bool(exact_paired)     # --exact-paired: handed on to every worker
        # --exact-delta-posterior: beside the `.miso_bf_exact` table the `.miso_dpsi_exact` (compare.py), merged like it
        self.exact_delta_posterior = bool(exact_delta_posterior)
        # --delta-posterior: beside the `.miso_bf` table the all-pairs `.miso_dpsi` (compare.py), merged like a diagnostics
        # table, with the same delta_thresholds
        self.delta_posterior = bool(delta_posterior)
        self.rank_diagnostics = bool(rank_diagnostics)   # --rank-diagnostics: six more columns in every diagnostics table
        self.summary_only = bool(summary_only)
        self.exact = bool(exact)       # --exact: handed on to every worker
        # --exact-compare / --exact-paired-compare: beside the `.miso_bf` table the exact comparison's `.miso_bf_exact` (compare.py), merged like a
        # diagnostics table; delta_thresholds: its thresholds (None: the workers' default)
        self.exact_compare = bool(exact_compare)
        self.delta_thresholds = None if delta_thresholds is None else [float(t) for t in delta_thresholds]
        self.diagnostics = bool(diagnostics)
        self.diag_tables = []          # --diagnostics: [(table, its per-worker parts)], one per output directory (run)
        self.prefilter = bool(prefilter)
        self.event_numbers = None      # --prefilter: gene id -> its number in the whole gene list
        self.gene_samples = None       # --prefilter --compare: gene id -> the samples whose filter it passes
        self.gff_dir, self.bam_filename, self.output_dir = gff_dir, bam_filename, output_dir
        if not os.path.isfile(self.bam_filename):
            raise IOError("BAM file %s not found." % self.bam_filename)
        self.read_len = read_len
        self.overhang_len = 1            # "For now setting overhang to 1 always" (miso.py:100-102)
        self.settings_fname, self.paired_end = settings_fname, paired_end
        self.event_type, self.seed = event_type, seed
        self.summarize, self.compare_bam, self.labels = summarize, compare_bam, labels
        if compare_bam is not None and not os.path.isfile(compare_bam):
            raise IOError("BAM file %s not found." % compare_bam)
        self.n_gpus = max(1, visible_gpus())
        self.num_processors = int(num_proc) if num_proc is not None else self.n_gpus
        self.batch_logs_dir = os.path.join(output_dir, "batch-logs")
        self.batch_genes_dir = os.path.join(output_dir, "batch-genes")
        os.makedirs(self.batch_logs_dir, exist_ok=True)
        os.makedirs(self.batch_genes_dir, exist_ok=True)
        self.gene_ids_to_gff_index = gff_utils.get_gene_ids_to_gff_index(gff_dir)
        self.gene_ids = list(gene_ids) if gene_ids is not None else \
            list(self.gene_ids_to_gff_index.keys())
        if len(self.gene_ids) == 0:
            raise ValueError("No genes to run on. Did you pass me the wrong path to your index "
                             "GFF directory? Or perhaps your indexed GFF directory is empty?")

    def apply_prefilter(self):
        """--prefilter (miso.py:379-404, run_events_analysis.py:28-68): keep the genes whose coverage table line passes,
        in index order; with --compare, those passing in either sample.  Raises PrefilterError when none passes."""
        from . import exon_utils
        genes_gff = os.path.join(self.gff_dir, "genes.gff")
        if not os.path.isfile(genes_gff):
            print("WARNING: Could not find 'genes.gff' in %s - skipping prefilter stage. Please reindex your GFF file "
                  "with the latest version to enable prefiltering." % self.gff_dir)
            return
        if self.compare_bam is None:
            targets = [(self.bam_filename, self.output_dir)]
        else:
            targets = [(self.bam_filename, os.path.join(self.output_dir, self.labels[0])),
                       (self.compare_bam, os.path.join(self.output_dir, self.labels[1]))]
        min_event_reads = Settings.get_min_event_reads()
        passing = []
        for bam, out_dir in targets:
            print("Prefiltering reads...")
            table = exon_utils.get_bam_gff_coverage(bam, genes_gff, out_dir, compute=self._coverage_in_child)
            passing.append(set(exon_utils.get_ids_passing_filter(table, min_event_reads)))
        self.event_numbers = {g: k for k, g in enumerate(self.gene_ids)}
        kept = [g for g in self.gene_ids if any(g in p for p in passing)]
        if not kept:
            raise PrefilterError("None of the events in %s appear to meet the read coverage filter. Check that your "
                                 "BAM headers in %s match the GFF headers of indexed events."
                                 % (self.gff_dir, ", ".join(b for b, _ in targets)))
        print("Total of %d events pass coverage filter." % len(kept))
        if self.compare_bam is not None:
            self.gene_samples = {g: ",".join(str(k + 1) for k, p in enumerate(passing) if g in p) for g in kept}
        self.gene_ids = kept

    def _coverage_in_child(self, bam_filename, gff_filename, output_filename):
        import multiprocessing
        sys.stdout.flush()
        p = multiprocessing.get_context("fork").Process(target=_coverage_child,
                                                        args=(bam_filename, gff_filename, output_filename))
        p.start()
        p.join()
        if p.exitcode != 0 or not os.path.isfile(output_filename):
            raise PrefilterError("the coverage pass over %s failed (exit %s)" % (bam_filename, p.exitcode))

    def _decode_once(self):
        """Decode the alignment file(s) here, through the HIP-free reader library, for the forked children."""
        from . import sam_utils
        sam_utils.use_reader_library()
        for path in (self.bam_filename, self.compare_bam):
            if path is not None:
                full = os.path.abspath(os.path.expanduser(path))
                if full not in sam_utils._PRELOADED:
                    sam_utils._PRELOADED[full] = sam_utils.Samfile(full, "rb")

    def output_batch_files(self):
        """miso.py:152-186: batch-<n>_genes.txt, two columns: gene ID, indexed file; with --prefilter a third, the
        gene's number in the whole gene list, and with --compare a fourth, the samples whose filter it passes."""
        batches = []
        first = 0
        for batch_num, ids in enumerate(chunk_list(self.gene_ids, self.num_processors)):
            fname = os.path.join(self.batch_genes_dir, "batch-%d_genes.txt" % batch_num)
            with open(fname, "w") as out:
                for gene_id in ids:
                    if gene_id not in self.gene_ids_to_gff_index:
                        print("Skipping: %s" % gene_id)
                        continue
                    line = "%s\t%s" % (gene_id, self.gene_ids_to_gff_index[gene_id])
                    if self.event_numbers is not None:
                        line += "\t%d" % self.event_numbers[gene_id]
                    if self.gene_samples is not None:
                        line += "\t%s" % self.gene_samples[gene_id]
                    out.write(line + "\n")
            batches.append((fname, len(ids), first))
            first += len(ids)
        return batches

    def run(self):
        t_run0 = time.time()
        fork = os.environ.get("MISO_DISPATCH", "fork") != "subprocess"
        if self.prefilter:
            # the coverage child inherits the one decode the workers will share (when they will share one)
            if fork and (self.num_processors > 1 or self.compare_bam is not None):
                try:
                    self._decode_once()
                except (ImportError, OSError, RuntimeError, ValueError):
                    from . import sam_utils
                    sam_utils._PRELOADED.clear()
            self.apply_prefilter()
            if os.environ.get("MISO_TIMING"):
                print("[miso] prefilter done %.2f s after run() started" % (time.time() - t_run0))
        batches = self.output_batch_files()
        if os.environ.get("MISO_TIMING"):
            print("[miso] batch files written in %.2f s" % (time.time() - t_run0))
        print("Preparing to run %d batches of jobs..." % len(batches))
        jobs = []
        parts = []
        if self.compare_bam is not None:
            out1, out2 = (os.path.join(self.output_dir, l) for l in self.labels)
            cmp_name = "%s_vs_%s" % self.labels
            table = os.path.join(self.output_dir, cmp_name, "bayes-factors", cmp_name + ".miso_bf")
        elif self.summarize:
            label = os.path.basename(os.path.normpath(self.output_dir))
            table = os.path.join(self.output_dir, "summary", label + ".miso_summary")
        else:
            table = None
        if table is not None:
            os.makedirs(os.path.dirname(table), exist_ok=True)
        self.diag_tables = []
        xtable = []                    # --exact-compare: [(table, its per-worker parts)], merged with the diagnostics tables
        dtable = []                    # --delta-posterior: likewise
        etable = []                    # --exact-delta-posterior: likewise
        if self.diagnostics:
            # one table per directory of `.miso` files: the output directory, or with --compare each label's
            for d in ([self.output_dir] if self.compare_bam is None else [out1, out2]):
                label = os.path.basename(os.path.normpath(d))
                self.diag_tables.append((os.path.join(d, "summary", label + ".miso_diag"), []))
                os.makedirs(os.path.dirname(self.diag_tables[-1][0]), exist_ok=True)
        n_diag = len(self.diag_tables)
        stables = []                   # --exact-stats: [(table, its per-worker parts)], one per directory of `.miso` files
        if self.exact_stats:
            for d in ([self.output_dir] if self.compare_bam is None else [out1, out2]):
                label = os.path.basename(os.path.normpath(d))
                stables.append((os.path.join(d, "summary", label + ".miso_exact_stats"), []))
                os.makedirs(os.path.dirname(stables[-1][0]), exist_ok=True)
        ftables = []                   # --model-check: [(table, its per-worker parts)], one per directory of `.miso` files
        if self.model_check:
            for d in ([self.output_dir] if self.compare_bam is None else [out1, out2]):
                label = os.path.basename(os.path.normpath(d))
                ftables.append((os.path.join(d, "summary", label + ".miso_fit"), []))
                os.makedirs(os.path.dirname(ftables[-1][0]), exist_ok=True)
        qtables = []                   # --part-psi: [(table, its per-worker parts)]: one per directory, then the comparison's
        if self.part_psi:
            for d in ([self.output_dir] if self.compare_bam is None else [out1, out2]):
                label = os.path.basename(os.path.normpath(d))
                qtables.append((os.path.join(d, "summary", label + ".miso_part_summary"), []))
                os.makedirs(os.path.dirname(qtables[-1][0]), exist_ok=True)
            if self.compare_bam is not None:
                qtables.append((table[:-len(".miso_bf")] + ".miso_part_dpsi", []))
        self.part_tables = [t for t, _ in qtables]
        if self.exact_paired_stats:    # --exact-paired-stats: (the `.miso_exact_pairs` table, its per-worker parts); no --compare
            label = os.path.basename(os.path.normpath(self.output_dir))
            ptable = (os.path.join(self.output_dir, "summary", label + ".miso_exact_pairs"), [])
            os.makedirs(os.path.dirname(ptable[0]), exist_ok=True)
        for batch_num, (fname, size, first) in enumerate(batches):
            if size == 0:
                continue
            part = None if table is None else "%s.gpu%d" % (table, batch_num)
            if part:
                parts.append(part)
            if self.compare_bam is not None:
                cmd = [sys.executable, "-m", "miso_amd.run_miso", "--compare-genes-from-file", fname,
                       self.bam_filename, self.compare_bam, out1, out2, part]
                if self.exact_compare:
                    if not xtable:
                        xtable.append((table + "_exact", []))
                    xtable[0][1].append("%s.gpu%d" % (xtable[0][0], batch_num))
                    cmd += ["--exact-comparison-file", xtable[0][1][-1]]
                    if self.exact_delta_posterior:
                        if not etable:
                            etable.append((table[:-len(".miso_bf")] + ".miso_dpsi_exact", []))
                        etable[0][1].append("%s.gpu%d" % (etable[0][0], batch_num))
                        cmd += ["--exact-delta-file", etable[0][1][-1]]
                if self.delta_posterior:
                    if not dtable:
                        dtable.append((table[:-len(".miso_bf")] + ".miso_dpsi", []))
                    dtable[0][1].append("%s.gpu%d" % (dtable[0][0], batch_num))
                    cmd += ["--delta-posterior-file", dtable[0][1][-1]]
                if (self.exact_compare or self.delta_posterior) and self.delta_thresholds is not None:
                    cmd += ["--delta-psi-thresholds"] + ["%r" % t for t in self.delta_thresholds]
                if n_diag:
                    dparts = ["%s.gpu%d" % (t, batch_num) for t, _ in self.diag_tables]
                    for (_, plist), dp in zip(self.diag_tables, dparts):
                        plist.append(dp)
                    cmd += ["--diagnostics-files"] + dparts + (["--rank-diagnostics"] if self.rank_diagnostics else [])
                if stables:
                    sparts = ["%s.gpu%d" % (t, batch_num) for t, _ in stables]
                    for (_, plist), sp in zip(stables, sparts):
                        plist.append(sp)
                    cmd += ["--exact-stats-files"] + sparts
                if ftables:
                    fparts = ["%s.gpu%d" % (t, batch_num) for t, _ in ftables]
                    for (_, plist), fp in zip(ftables, fparts):
                        plist.append(fp)
                    cmd += ["--model-check-files"] + fparts
                if qtables:
                    qparts = ["%s.gpu%d" % (t, batch_num) for t, _ in qtables]
                    for (_, plist), qp in zip(qtables, qparts):
                        plist.append(qp)
                    cmd += ["--part-psi-files"] + qparts
                    if self.delta_thresholds is not None and not (self.exact_compare or self.delta_posterior):
                        cmd += ["--delta-psi-thresholds"] + ["%r" % t for t in self.delta_thresholds]
            else:
                cmd = [sys.executable, "-m", "miso_amd.run_miso", "--compute-genes-from-file", fname,
                       self.bam_filename, self.output_dir]
                if part:
                    cmd += ["--summary-file", part]
                    if self.summary_only:
                        cmd += ["--no-miso-files"]
                if self.diag_tables:
                    self.diag_tables[0][1].append("%s.gpu%d" % (self.diag_tables[0][0], batch_num))
                    cmd += ["--diagnostics-file", self.diag_tables[0][1][-1]] + (["--rank-diagnostics"] if self.rank_diagnostics else [])
                if stables:
                    stables[0][1].append("%s.gpu%d" % (stables[0][0], batch_num))
                    cmd += ["--exact-stats-file", stables[0][1][-1]]
                if ftables:
                    ftables[0][1].append("%s.gpu%d" % (ftables[0][0], batch_num))
                    cmd += ["--model-check-file", ftables[0][1][-1]]
                if qtables:
                    qtables[0][1].append("%s.gpu%d" % (qtables[0][0], batch_num))
                    cmd += ["--part-psi-file", qtables[0][1][-1]]
                if self.exact_paired_stats:
                    ptable[1].append("%s.gpu%d" % (ptable[0], batch_num))
                    cmd += ["--exact-pairs-file", ptable[1][-1]]
            # more chunks than GPUs (-p above the GPU count) share the GPUs round robin
            cmd += ["--read-len", str(self.read_len), "--device", str(batch_num % self.n_gpus),
                    "--first-event-id", str(first)]
            if self.paired_end is not None:
                cmd += ["--paired-end", "%.1f" % float(self.paired_end[0]),
                        "%.1f" % float(self.paired_end[1])]
            else:
                cmd += ["--overhang-len", str(self.overhang_len)]
            if self.settings_fname is not None:
                cmd += ["--settings-filename", self.settings_fname]
            if self.event_type is not None:
                cmd += ["--event-type", self.event_type]
            if self.seed is not None:
                cmd += ["--seed", str(self.seed)]
            if self.exact:
                cmd += ["--exact"]
            if self.exact_paired:
                cmd += ["--exact-paired"]
            log = os.path.join(self.batch_logs_dir, "batch-%d-%s.log"
                               % (batch_num, time.strftime("%m-%d-%y_%H:%M:%S")))
            print("Running batch of %d genes on GPU %d.." % (size, batch_num % self.n_gpus))
            jobs.append((batch_num, cmd, log))
        self.diag_tables += xtable + dtable + etable + stables + ftables + qtables + ([ptable] if self.exact_paired_stats else [])
        # One decode per node: this process reads the alignment file(s) ONCE through the HIP-free reader
        # library and forks the workers, which inherit the decoded columns (copy-on-write, nothing copied);
        # each worker then initialises its own GPU.  The reference re-opens the BAM per event through an
        # index (run_miso.py:86,100); round 1 decoded the whole file in every worker (`-p 4` on one GPU was
        # slower than `-p 1`).  MISO_DISPATCH=subprocess: fresh interpreters that decode for themselves.
        if not fork or not jobs:
            return self._run_subprocesses(jobs, parts, table)
        import multiprocessing
        from . import sam_utils
        if len(jobs) == 1 and self.compare_bam is None:
            # one worker: nothing to share -- it opens the file itself, on a thread beside its annotation work
            # (run_miso.compute_gene_psi), instead of waiting here for a decode it could be working next to
            ctx = multiprocessing.get_context("fork")
            sys.stdout.flush()
            batch_num, cmd, log = jobs[0]
            p = ctx.Process(target=_forked_worker, args=(cmd[3:], log, 0, 1))
            p.start()
            return self._finish([(batch_num, p.join, lambda p=p: p.exitcode, log)], parts, table)
        try:
            self._decode_once()
        except (ImportError, OSError, RuntimeError, ValueError) as e:
            # no reader library (a partial build) or the one decode failed: the workers decode for themselves
            # (the jobs are built; nothing is re-done and the process's environment is left alone)
            print("One decode per node not possible (%s): starting workers that read the alignment file themselves" % e)
            sam_utils._PRELOADED.clear()
            return self._run_subprocesses(jobs, parts, table)
        if os.environ.get("MISO_TIMING"):
            print("[miso] alignment file(s) decoded %.2f s after run() started" % (time.time() - t_run0))
        ctx = multiprocessing.get_context("fork")
        sys.stdout.flush()
        waits = []
        for k, (batch_num, cmd, log) in enumerate(jobs):
            p = ctx.Process(target=_forked_worker, args=(cmd[3:], log, k, len(jobs)))
            p.start()
            waits.append((batch_num, p.join, lambda p=p: p.exitcode, log))
        return self._finish(waits, parts, table)

    def _run_subprocesses(self, jobs, parts, table):
        """One fresh interpreter per job, each decoding the alignment file itself (MISO_DISPATCH=subprocess, and the
        fall-back when the one decode per node is not possible)."""
        env = dict(os.environ)
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
        procs = []
        for batch_num, cmd, log in jobs:
            procs.append((batch_num, subprocess.Popen(cmd, stdout=open(log, "a"), stderr=subprocess.STDOUT, env=env), log))
        waits = [(b, p.wait, lambda p=p: p.returncode, log) for b, p, log in procs]
        return self._finish(waits, parts, table)

    def _finish(self, waits, parts, table):
        failed = 0
        for batch_num, wait, code, log in waits:
            wait()
            if code() != 0:
                failed += 1
                print("WARNING: batch %d might have failed (exit %s), see %s" % (batch_num, code(), log))
        if table is not None:
            from .run_miso import merge_tables
            merge_tables(parts, table)
            print("Wrote %s" % table)
        for diag_table, diag_parts in self.diag_tables:
            from .run_miso import merge_tables
            merge_tables(diag_parts, diag_table)
            if diag_table in getattr(self, "part_tables", ()):      # one order whatever the workers and launches were
                from . import part_psi
                part_psi.sort_table(diag_table)
            print("Wrote %s" % diag_table)
        return failed


def compute_all_genes_psi(gff_dir, bam_filename, read_len, output_dir, overhang_len=1,
                          paired_end=None, settings_fname=None, num_proc=None, event_type=None,
                          seed=None, summarize=False, compare_bam=None,
                          labels=("sample1", "sample2"), summary_only=False, prefilter=False, diagnostics=False, exact=False,
                          exact_compare=False, delta_thresholds=None, exact_paired=False, rank_diagnostics=False,
                          delta_posterior=False, exact_delta_posterior=False, exact_stats=False, exact_paired_stats=False,
                          model_check=False, part_psi=False):
    """miso.py:340-420."""
    print("Computing Psi values...")
    print("  - GFF index: %s" % gff_dir)
    print("  - BAM: %s" % bam_filename)
    print("  - Read length: %d" % read_len)
    print("  - Output directory: %s" % output_dir)
    os.makedirs(output_dir, exist_ok=True)
    return GenesDispatcher(gff_dir, bam_filename, output_dir, read_len, overhang_len,
                           settings_fname=settings_fname, paired_end=paired_end, num_proc=num_proc,
                           event_type=event_type, seed=seed, summarize=summarize or summary_only,
                           compare_bam=compare_bam, labels=labels, summary_only=summary_only,
                           prefilter=prefilter, diagnostics=diagnostics, exact=exact, exact_compare=exact_compare, exact_paired=exact_paired,
                           delta_thresholds=delta_thresholds, rank_diagnostics=rank_diagnostics,
                           delta_posterior=delta_posterior, exact_delta_posterior=exact_delta_posterior,
                           exact_stats=exact_stats, exact_paired_stats=exact_paired_stats, model_check=model_check,
                           part_psi=part_psi).run()


def main(argv=None):
    import argparse
    t_main0 = time.time()
    ap = argparse.ArgumentParser(description="MISO (Mixture of Isoforms model) on MI355X")
    ap.add_argument("--run", nargs=2, metavar=("INDEXED_GFF_DIR", "BAM"))
    ap.add_argument("--event-type", default=None)
    ap.add_argument("--settings-filename", default=None)
    ap.add_argument("--read-len", type=int, default=None)
    ap.add_argument("--paired-end", nargs=2, default=None, metavar=("MEAN", "SD"))
    ap.add_argument("--overhang-len", type=int, default=None)
    ap.add_argument("--output-dir", default=None)
    ap.add_argument("-p", dest="num_proc", type=int, default=None,
                    help="worker processes (default: one per visible GPU; more share the GPUs round robin)")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--summarize", action="store_true",
                    help="also write OUT/summary/<OUT>.miso_summary (summarize_miso's table) from "
                         "posterior means / credible intervals computed on the GPU during the run")
    ap.add_argument("--summary-only", action="store_true",
                    help="--summarize without the per-event .miso files: the run's product is the summary table alone "
                         "(what summarize_miso needs of a .miso file is its mean and credible interval, samples_utils.py:263-329)")
    ap.add_argument("--diagnostics", action="store_true",
                    help="also write OUT/summary/<OUT>.miso_diag: per event the split R-hat of its chains, the effective "
                         "sample size and the Monte-Carlo standard error of the Psi mean, computed on the GPU during the run; "
                         "with --compare one table per label: OUT/<label>/summary/<label>.miso_diag")
    ap.add_argument("--rank-diagnostics", action="store_true",
                    help="with --diagnostics: six more columns per event from the rank-normalised pass -- the larger of the bulk "
                         "and the folded rank R-hat, the bulk effective sample size, the effective sample size of the 95 %% "
                         "credible interval's two bounds and the smaller of them, and the number of distinct draws")
    ap.add_argument("--model-check", action="store_true",
                    help="single-end runs: also write OUT/summary/<OUT>.miso_fit (with --compare one table per label, where "
                         ".miso_diag goes): per event a posterior predictive check of its reads against the read classes the "
                         "model expects -- a p-value, observed and expected reads per class and which class is short or in "
                         "excess --, computed on the GPU during the run with the run's seed; every other output is unchanged")
    ap.add_argument("--part-psi", action="store_true",
                    help="also write OUT/summary/<OUT>.miso_part_summary: per part (exon) of every multi-isoform event how often "
                         "it is included -- the sum of the psi of the isoforms that hold it --, posterior mean and credible "
                         "interval from the joint draws, computed on the GPU during the run; with --compare one table per label "
                         "and <l1>_vs_<l2>.miso_part_dpsi beside the .miso_bf: each exon's delta psi over all pairs of the two "
                         "samples' draws (thresholds: --delta-psi-thresholds, default 0.1 0.2); every other output is unchanged")
    ap.add_argument("--exact", action="store_true",
                    help="single-end two-isoform events (SE, A3SS, A5SS, RI, MXE): no chains -- the posterior of Psi is tabulated "
                         "once per event on the GPU and the .miso file's samples are independent draws from it (percent_accept=100); "
                         "other events are sampled as always.  Also the settings key `exact` under [sampler].")
    ap.add_argument("--exact-stats", action="store_true",
                    help="with --exact: also write OUT/summary/<OUT>.miso_exact_stats (with --compare one table per label): per "
                         "event the seven statistics its exact posterior is made of, what `samples_utils --compare-groups "
                         "--exact-delta-posterior` pools replicates of separate runs from; every other output is unchanged")
    ap.add_argument("--exact-paired", action="store_true",
                    help="with --paired-end: paired-end two-isoform events run no chains -- the posterior of Psi, a product over "
                         "the event's read pairs, is tabulated once per event on the GPU and the .miso file's samples are "
                         "independent draws from it (percent_accept=100); other events are sampled as always.  Also the "
                         "settings key `exact_paired` under [sampler].")
    ap.add_argument("--exact-paired-stats", action="store_true",
                    help="with --exact-paired (and without --compare): also write OUT/summary/<OUT>.miso_exact_pairs: per event the "
                         "six statistics and the drawing pairs' probabilities its exact posterior is made of, what `samples_utils "
                         "--compare-groups --exact-paired-delta-posterior` pools replicates of separate runs from.  The table "
                         "grows with the drawing pairs, in the order of 10 bytes a pair; every other output is unchanged")
    ap.add_argument("--exact-compare", action="store_true",
                    help="with --compare and the exact mode: also write OUT/<l1>_vs_<l2>/bayes-factors/<l1>_vs_<l2>.miso_bf_exact -- "
                         "for the events the exact mode took in both samples the Bayes factor and P(|delta Psi| >= T) come from the "
                         "two posteriors' tables, without sampling error and whatever the seed; the .miso_bf table is unchanged")
    ap.add_argument("--exact-paired-compare", action="store_true",
                    help="with --compare, --paired-end and the paired exact mode: also write the .miso_bf_exact table of "
                         "--exact-compare for the events the paired exact mode took in both samples -- the product of the two "
                         "posteriors is tabulated over both samples' read pairs; the .miso files and the .miso_bf table are unchanged")
    ap.add_argument("--delta-psi-thresholds", nargs="+", type=float, default=None, metavar="T",
                    help="the thresholds T of --exact-compare / --exact-paired-compare / --delta-posterior, each in (0, 1), at "
                         "most four (default 0.1 0.2)")
    ap.add_argument("--delta-posterior", action="store_true",
                    help="with --compare, any mode and any number of isoforms: also write "
                         "OUT/<l1>_vs_<l2>/bayes-factors/<l1>_vs_<l2>.miso_dpsi -- median and 95 %% credible interval of delta Psi, "
                         "P(delta Psi > 0), P(delta Psi < 0) and P(|delta Psi| >= T) over ALL pairs of the two samples' draws, "
                         "computed on the GPU during the run; every other output is unchanged")
    ap.add_argument("--exact-delta-posterior", action="store_true",
                    help="with --exact-compare or --exact-paired-compare: also write "
                         "OUT/<l1>_vs_<l2>/bayes-factors/<l1>_vs_<l2>.miso_dpsi_exact -- median and 95 %% credible interval of delta "
                         "Psi, P(delta Psi > 0), P(delta Psi < 0) and P(|delta Psi| >= T) from the exact CDF of delta Psi, without "
                         "sampling error and whatever the seed; every other output is unchanged")
    ap.add_argument("--compare", metavar="BAM2", default=None,
                    help="second RNA-seq sample: sample both, write OUT/<label1>/, OUT/<label2>/ and the "
                         "compare_miso table OUT/<l1>_vs_<l2>/bayes-factors/<l1>_vs_<l2>.miso_bf")
    ap.add_argument("--labels", nargs=2, default=("sample1", "sample2"))
    ap.add_argument("--prefilter", default=False, action="store_true",
                    help="Prefilter events based on coverage. If given as argument, run will begin by mapping BAM "
                         "reads to event regions (counted on the GPU), and omit events that do not meet coverage "
                         "criteria from the run. By default, turned off. Note that events that do not meet the "
                         "coverage criteria will not be processed regardless, but --prefilter simply does this "
                         "filtering step at the start of the run, potentially saving computation time so that low "
                         "coverage events will not be processed or distributed to jobs.")
    a = ap.parse_args(argv)
    settings_filename = None if a.settings_filename is None else \
        os.path.abspath(os.path.expanduser(a.settings_filename))
    Settings.load(settings_filename)
    if a.exact_paired and a.paired_end is None:     # argument errors, before any work
        ap.error("--exact-paired goes with --paired-end")
    if a.model_check and a.paired_end is not None:
        ap.error("--model-check is single-end only: a paired-end read's class is compatibility x fragment length")
    if a.part_psi:
        from . import part_psi
        p = Settings.get_sampler_params()
        why = part_psi.samples_refusal(p["num_chains"] * (p["num_iters"] - p["burn_in"]) // p["lag"])
        if why:
            ap.error("--part-psi: %s" % why)
    if a.rank_diagnostics and not a.diagnostics:
        ap.error("--rank-diagnostics goes with --diagnostics")
    if a.exact_stats and (a.paired_end or not (a.exact or Settings.get_exact())):
        ap.error("--exact-stats needs the exact-posterior mode of single-end runs (--exact, or `exact = True` in the settings)")
    if a.exact_paired_stats:
        if a.paired_end is None or not (a.exact_paired or Settings.get_exact_paired()):
            ap.error("--exact-paired-stats needs the paired exact-posterior mode (--paired-end with --exact-paired, or "
                     "`exact_paired = True` in the settings)")
        if a.compare is not None:
            ap.error("--exact-paired-stats does not go with --compare")
    if a.exact_compare:
        if a.compare is None:
            ap.error("--exact-compare goes with --compare")
        if a.paired_end is not None:
            ap.error("--exact-compare: the exact-posterior mode takes single-end events only")
        if not (a.exact or Settings.get_exact()):
            ap.error("--exact-compare needs the exact-posterior mode (--exact, or `exact = True` in the settings)")
    if a.exact_paired_compare:
        if a.compare is None:
            ap.error("--exact-paired-compare goes with --compare")
        if a.paired_end is None:
            ap.error("--exact-paired-compare goes with --paired-end")
        if not (a.exact_paired or Settings.get_exact_paired()):
            ap.error("--exact-paired-compare needs the paired exact-posterior mode (--exact-paired, or `exact_paired = True` "
                     "in the settings)")
    if a.delta_posterior and a.compare is None:
        ap.error("--delta-posterior goes with --compare")
    if a.exact_delta_posterior and not (a.exact_compare or a.exact_paired_compare):
        ap.error("--exact-delta-posterior goes with --exact-compare or --exact-paired-compare")
    if a.delta_psi_thresholds is not None:
        if not (a.exact_compare or a.exact_paired_compare or a.delta_posterior or (a.part_psi and a.compare is not None)):
            ap.error("--delta-psi-thresholds goes with --exact-compare or --delta-posterior")
        from . import compare
        try:
            compare.check_delta_thresholds(a.delta_psi_thresholds)
        except ValueError as err:
            ap.error(str(err))
    if a.run is None:
        ap.print_help()
        return 0
    if a.output_dir is None:
        print("Error: need --output-dir to compute Psi values.")
        return 1
    if a.read_len is None:
        print("Error: need --read-len to compute Psi values.")
        return 1
    gff_dir, bam = (os.path.abspath(os.path.expanduser(p)) for p in a.run)
    try:
        failed = compute_all_genes_psi(gff_dir, bam, a.read_len,
                                       os.path.abspath(os.path.expanduser(a.output_dir)),
                                       overhang_len=a.overhang_len or 1, paired_end=a.paired_end,
                                       settings_fname=settings_filename, num_proc=a.num_proc,
                                       event_type=a.event_type, seed=a.seed, summarize=a.summarize,
                                       summary_only=a.summary_only,
                                       compare_bam=None if a.compare is None else
                                       os.path.abspath(os.path.expanduser(a.compare)),
                                       labels=tuple(a.labels), prefilter=a.prefilter, diagnostics=a.diagnostics,
                                       exact=a.exact, exact_compare=a.exact_compare or a.exact_paired_compare,
                                       exact_paired=a.exact_paired,
                                       delta_thresholds=a.delta_psi_thresholds, rank_diagnostics=a.rank_diagnostics,
                                       delta_posterior=a.delta_posterior, exact_delta_posterior=a.exact_delta_posterior,
                                       exact_stats=a.exact_stats, exact_paired_stats=a.exact_paired_stats,
                                       model_check=a.model_check, part_psi=a.part_psi)
    except PrefilterError as err:
        print("Error: %s" % err)
        return 1
    if os.environ.get("MISO_TIMING"):
        print("[miso] main() %.2f s" % (time.time() - t_main0))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
