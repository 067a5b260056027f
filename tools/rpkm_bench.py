"""`sam_rpkm --compute-rpkm` on a synthetic genome: G two-isoform genes (exons A-B-C and A-C, so four constitutive
parts per gene, the copies included) on 24 chromosomes and R single-end 36-bp reads per gene, a fifth of them spliced,
written as GFF3 + SAM text sorted by position.  Prints
  * the decode time and the stages of one capi.fetch_counts call over all constitutive parts (second call in the process,
    HIP already started), from its stats;
  * the same counts taken on the host, one miso_aln_fetch index look-up per part (count only: idx NULL, cap 0) through
    the same ctypes binding the package uses -- what sam_rpkm would do without the device pass -- and that both agree;
  * the whole tool, wall.

    python tools/rpkm_bench.py [--genes 50000] [--reads 200] [--keep DIR]
"""
import argparse
import ctypes as C
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NCHR = 24
EXONS = ((0, 149), (400, 499), (800, 949))      # A, B, C relative to the gene's offset
SPACING = 5000


def generate(work, genes, reads, seed=1):
    gff, sam = os.path.join(work, "genes.gff"), os.path.join(work, "reads.sam")
    per_chr = (genes + NCHR - 1) // NCHR
    with open(gff, "w") as g:
        g.write("##gff-version 3\n")
        for e in range(genes):
            c, off = "chr%d" % (e // per_chr + 1), 10000 + (e % per_chr) * SPACING
            gid = "g%06d" % e
            g.write("%s\tx\tgene\t%d\t%d\t.\t+\t.\tID=%s\n" % (c, off, off + EXONS[-1][1], gid))
            for tid, iso in ((gid + ".a", (0, 1, 2)), (gid + ".b", (0, 2))):
                g.write("%s\tx\tmRNA\t%d\t%d\t.\t+\t.\tID=%s;Parent=%s\n" % (c, off, off + EXONS[-1][1], tid, gid))
                for x in iso:
                    g.write("%s\tx\texon\t%d\t%d\t.\t+\t.\tID=%s.e%d;Parent=%s\n"
                            % (c, off + EXONS[x][0], off + EXONS[x][1], tid, x, tid))
    rng = np.random.default_rng(seed)
    n_rec = 0
    with open(sam, "w") as s:
        s.write("@HD\tVN:1.0\tSO:coordinate\n")
        for c in range(NCHR):
            s.write("@SQ\tSN:chr%d\tLN:%d\n" % (c + 1, 10000 + (per_chr + 1) * SPACING))
        for c in range(NCHR):
            n_genes = max(0, min(per_chr, genes - c * per_chr))
            off = 10000 + np.repeat(np.arange(n_genes, dtype=np.int64), reads) * SPACING
            pos = np.sort(off + rng.integers(-50, 1000, size=len(off)))
            spliced = rng.random(len(pos)) < 0.2
            tail = "\t255\t36M\t*\t0\t0\t*\t*\n", "\t255\t18M250N18M\t*\t0\t0\t*\t*\n"
            head = "r\t0\tchr%d\t" % (c + 1)
            s.writelines([head + str(p) + tail[k] for p, k in zip(pos.tolist(), spliced.tolist())])
            n_rec += len(pos)
    return gff, sam, n_rec


def host_fetch_counts(f, seqids, starts, ends):
    """One miso_aln_fetch per interval, count only."""
    from miso_amd import sam_utils
    L = sam_utils._native()
    fetch = L.miso_aln_fetch
    fetch.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    n = C.c_int64()
    ref_n = C.byref(n)
    out = np.zeros(len(seqids), np.int64)
    t0 = time.time()
    tids = [f.gettid(s) for s in seqids]
    for i in range(len(tids)):
        fetch(f._h, tids[i], starts[i], ends[i], None, 0, ref_n)
        out[i] = n.value
    return out, time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=50000)
    ap.add_argument("--reads", type=int, default=200)
    ap.add_argument("--keep", default=None)
    a = ap.parse_args()
    from miso_amd import capi, gene_utils, sam_rpkm, sam_utils
    work = a.keep or tempfile.mkdtemp(prefix="miso_rpkm_")
    os.makedirs(work, exist_ok=True)
    t0 = time.time()
    gff, sam, n_rec = generate(work, a.genes, a.reads)
    print("genes %d, %d records, SAM %.0f MB; generate %.1f s" % (a.genes, n_rec, os.path.getsize(sam) / 1e6,
                                                                  time.time() - t0), flush=True)
    t0 = time.time()
    gff_genes = gene_utils.load_genes_from_gff(gff, suppress_warnings=True)
    t_gff = time.time() - t0
    t0 = time.time()
    f = sam_utils.Samfile(sam)
    t_decode = time.time() - t0
    t0 = time.time()
    seqids, starts, ends = sam_rpkm.const_part_intervals(gff_genes, f)
    t_parts = time.time() - t0
    print("GFF into genes %.1f s | decode %.3f s | constitutive parts %d (collected in %.2f s)"
          % (t_gff, t_decode, len(seqids), t_parts), flush=True)
    capi.fetch_counts(f, seqids, starts, ends)               # first call: HIP start-up included
    for chunk in (0, 1 << 20):
        t0 = time.time()
        counts, st = capi.fetch_counts(f, seqids, starts, ends, chunk_records=chunk)
        t_pass = time.time() - t0
        print("device: fetch_counts %.1f ms wall in Python, %.1f ms in the call: tables %.1f ms, record pass %.1f ms (%d "
              "chunks of %d, copies + kernel, device time), rank step %.1f ms"
              % (t_pass * 1e3, st["total_ms"], st["sort_ms"], st["records_ms"], st["chunks"], chunk or (1 << 22),
                 st["rank_ms"]), flush=True)
        if chunk == 0:
            t_device = t_pass
    host, t_host = host_fetch_counts(f, seqids, starts, ends)
    print("host: %d miso_aln_fetch look-ups %.1f ms (%.2f us each) | equal counts: %s | parts with reads: %d, "
          "sum of counts %d" % (len(seqids), t_host * 1e3, t_host * 1e6 / max(len(seqids), 1),
                                bool((host == counts).all()), int((counts > 0).sum()), int(counts.sum())), flush=True)
    print("ratio host loop / device call: %.1f" % (t_host / t_device), flush=True)
    f.close()
    out = os.path.join(work, "out")
    shutil.rmtree(out, ignore_errors=True)
    devnull = open(os.devnull, "w")
    t0 = time.time()
    stdout, sys.stdout = sys.stdout, devnull
    try:
        rows = sam_rpkm.compute_rpkm(gff, sam, 36, out)
    finally:
        sys.stdout = stdout
    print("sam_rpkm --compute-rpkm, whole tool in this process: %.1f s, %d rows" % (time.time() - t0, len(rows)),
          flush=True)
    if not a.keep:
        shutil.rmtree(work, ignore_errors=True)
    return 0 if (host == counts).all() else 1


if __name__ == "__main__":
    sys.exit(main())
