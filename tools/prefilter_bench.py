"""`miso --run --prefilter` on a synthetic genome: E skipped-exon events on 20 chromosomes, every other one with
--low-reads reads (under min_event_reads = 20, so the prefilter drops half the events) and the rest with --reads reads,
written as GFF3 + SAM text.  Prints the decode time, the device pass split into its stages, and `miso --run` with and
without --prefilter at -p 1 and at -p = the GPUs available (or --procs).

    python tools/prefilter_bench.py [--events 40000] [--reads 1000] [--low-reads 10] [--keep DIR]
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def coverage_only(bam, gff, out, chunk):
    """One coverage pass in this process (started by main() as a child of its own): decode, then the device pass."""
    from miso_amd import exon_utils, sam_utils
    t0 = time.time()
    f = sam_utils.Samfile(bam)
    t_decode = time.time() - t0
    intervals = exon_utils.read_coverage_intervals(gff)
    counts, st = exon_utils.coverage_counts(f, intervals, chunk_records=chunk)   # first call: HIP start-up included
    t0 = time.time()
    counts, st = exon_utils.coverage_counts(f, intervals, chunk_records=chunk)
    t_pass = time.time() - t0
    t0 = time.time()
    with open(out, "w") as o:
        o.write(exon_utils.format_coverage(intervals, counts))
    t_write = time.time() - t0
    print("records %d, intervals %d, kept %d, intervals >= 20: %d | decode %.3f s | device pass %.3f s wall: tables "
          "%.1f ms, record pass %.1f ms (%d chunks of %d, copies + kernel, device time), rank step %.1f ms | "
          "table write %.3f s"
          % (len(f), len(intervals), st["kept"], int((counts >= 20).sum()), t_decode, t_pass, st["sort_ms"],
             st["records_ms"], st["chunks"], chunk or (1 << 22), st["rank_ms"], t_write), flush=True)


def generate(work, events, reads, low_reads):
    from miso_amd import workload
    gff, sam = os.path.join(work, "events.gff"), os.path.join(work, "reads.sam")
    nchr = 20
    per_chr = (events + nchr - 1) // nchr
    sam_recs = [[] for _ in range(nchr)]
    n_rec = 0
    with open(gff, "w") as g:
        g.write("##gff-version 3\n")
        for e in range(events):
            c, slot = e // per_chr, e % per_chr
            off = 10000 + slot * 5000
            exons, isoforms, pos, cig = workload.event_reads(e, 2, low_reads if e % 2 else reads, 36)
            ex = [(s + off, t + off) for s, t in exons]
            gid = "ev%06d" % e
            g.write("chr%d\tSE\tgene\t%d\t%d\t.\t+\t.\tID=%s;Name=%s\n" % (c + 1, ex[0][0], ex[-1][1], gid, gid))
            for m, iso in enumerate(isoforms):
                tid = "%s.%s" % (gid, "AB"[m])
                g.write("chr%d\tSE\tmRNA\t%d\t%d\t.\t+\t.\tID=%s;Parent=%s\n"
                        % (c + 1, ex[iso[0]][0], ex[iso[-1]][1], tid, gid))
                for x in iso:
                    g.write("chr%d\tSE\texon\t%d\t%d\t.\t+\t.\tID=%s.e%d;Parent=%s\n"
                            % (c + 1, ex[x][0], ex[x][1], tid, x, tid))
            recs = sam_recs[c]
            for i in range(len(pos)):
                recs.append("r%d_%d\t0\tchr%d\t%d\t255\t%s\t*\t0\t0\t%s\t%s\n"
                            % (e, i, c + 1, pos[i] + off, cig[i].decode(), "A" * 36, "I" * 36))
            n_rec += len(pos)
    with open(sam, "w") as s:
        s.write("@HD\tVN:1.0\tSO:unsorted\n")
        for c in range(nchr):
            s.write("@SQ\tSN:chr%d\tLN:%d\n" % (c + 1, 10000 + (per_chr + 1) * 5000))
        for recs in sam_recs:
            s.writelines(recs)
    return gff, sam, n_rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=40000)
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--low-reads", type=int, default=10)
    ap.add_argument("--keep", default=None)
    ap.add_argument("--procs", default=None, help="comma list of -p values (default: 1 and the GPUs available)")
    ap.add_argument("--coverage-only", nargs=4, metavar=("BAM", "GFF", "OUT", "CHUNK"), default=None)
    a = ap.parse_args()
    if a.coverage_only:
        bam, gff, out, chunk = a.coverage_only
        return coverage_only(bam, gff, out, int(chunk))
    from miso_amd import miso as miso_cli
    work = a.keep or tempfile.mkdtemp(prefix="miso_prefilter_")
    os.makedirs(work, exist_ok=True)
    t0 = time.time()
    gff, sam, n_rec = generate(work, a.events, a.reads, a.low_reads)
    t_gen = time.time() - t0
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), MISO_TIMING="1")
    idx, out = os.path.join(work, "indexed"), os.path.join(work, "out")
    shutil.rmtree(idx, ignore_errors=True)
    t0 = time.time()
    subprocess.check_call([sys.executable, "-m", "miso_amd.index_gff", "--index", gff, idx], env=env,
                          stdout=subprocess.DEVNULL)
    t_index = time.time() - t0
    settings = os.path.join(work, "settings.txt")
    open(settings, "w").write("[data]\nfilter_results = True\nmin_event_reads = 20\n[sampler]\n"
                              "burn_in = 500\nlag = 10\nnum_iters = 5000\nnum_chains = 6\n")
    print("events %d (every other one %d reads, the rest %d), %d records, SAM %.0f MB; generate %.1f s | index_gff %.1f s"
          % (a.events, a.low_reads, a.reads, n_rec, os.path.getsize(sam) / 1e6, t_gen, t_index), flush=True)
    genes_gff = os.path.join(idx, "genes.gff")
    for chunk in (0, 1 << 20):
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--coverage-only", sam, genes_gff,
                               os.path.join(work, "standalone.bed"), str(chunk)], env=env)
    gpus = max(1, miso_cli.visible_gpus())
    print("GPUs available: %d" % gpus)
    for procs in sorted({1, gpus}) if a.procs is None else [int(p) for p in a.procs.split(",")]:
        for extra in ([], ["--prefilter"]):
            shutil.rmtree(out, ignore_errors=True)
            t0 = time.time()
            r = subprocess.run([sys.executable, "-m", "miso_amd.miso", "--run", idx, sam, "--output-dir", out,
                                "--read-len", "36", "--settings-filename", settings, "-p", str(procs), "--seed", "1"]
                               + extra, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            t_run = time.time() - t0
            n_files = sum(len([f for f in fs if f.endswith(".miso")]) for _, _, fs in os.walk(out))
            print("miso --run -p %d%s: %.2f s (rc %d) -> %d .miso files"
                  % (procs, " " + " ".join(extra) if extra else "", t_run, r.returncode, n_files), flush=True)
            for ln in r.stdout.splitlines():
                if ln.startswith("[miso]") or ln.startswith("Coverage of") or "pass coverage filter" in ln:
                    print("    " + ln)
            logs = os.path.join(out, "batch-logs")
            for f in sorted(os.listdir(logs)):
                lines = open(os.path.join(logs, f)).read().strip().split("\n")
                m = [ln for ln in lines if re.match(r"Collected|Computing Psi for", ln)]
                print("    %s: %s" % (f, " | ".join(m)))
            if r.returncode != 0:
                print(r.stdout[-3000:])
                return 1
    if not a.keep:
        shutil.rmtree(work, ignore_errors=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
