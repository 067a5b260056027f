"""The density pass of sashimi_plot (capi.region_densities, csrc/kernels_density.hip) on a synthetic genome: --records
records over 40 000 skipped-exon loci on 20 chromosomes, written as SAM text, and the densities of the first 1 000 and of
all 40 000 loci.  Prints the decode time and, per case, the stages of the pass (host tables, mark pass, group passes, scan,
junction step, copy back) as median [min - max] over --repeats calls after one warm-up call, the number of region groups,
and the wall time of the call with the Python conversion of its results.

    python tools/density_bench.py [--records 20000000] [--repeats 5] [--keep DIR] [--out profiles/read_density.txt]
"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOCI, NCHR, SLOT = 40000, 20, 5000
# a locus: exons [0, 100), [600, 700), [1200, 1300) from its start; the region is the whole span
SPAN = 1300


def locus_start(k):
    return 10000 + (k % (LOCI // NCHR)) * SLOT


def generate(path, records, seed=1):
    """Records in file order by locus (sorted within a chromosome up to the jitter inside a locus)."""
    rng = np.random.RandomState(seed)
    per = records // LOCI
    kinds = ["50M", "36M", "30M2D20M", "25M500N25M", "25M1100N25M", "10S40M"]
    weights = [0.55, 0.08, 0.05, 0.2, 0.07, 0.05]
    with open(path, "w") as out:
        out.write("@HD\tVN:1.0\tSO:unsorted\n")
        for c in range(NCHR):
            out.write("@SQ\tSN:chr%d\tLN:%d\n" % (c + 1, 10000 + (LOCI // NCHR + 1) * SLOT))
        n = 0
        for first in range(0, LOCI, 500):
            loci = np.repeat(np.arange(first, first + 500), per)
            kind = rng.choice(len(kinds), size=len(loci), p=weights)
            offset = rng.randint(-40, SPAN - 10, size=len(loci))
            # spliced records start 25 bases before an exon's end
            offset = np.where(kind == 3, 75 + 600 * rng.randint(0, 2, size=len(loci)), offset)
            offset = np.where(kind == 4, 75, offset)
            pos = (10000 + (loci % (LOCI // NCHR)) * SLOT + offset).reshape(500, per)
            order = np.argsort(pos, axis=1, kind="stable")
            pos = np.take_along_axis(pos, order, axis=1).ravel()
            kind = np.take_along_axis(kind.reshape(500, per), order, axis=1).ravel()
            chrom = loci // (LOCI // NCHR) + 1
            out.write("".join("r%d\t0\tchr%d\t%d\t255\t%s\t*\t0\t0\t*\t*\n" % (n + i, c, p, kinds[k])
                              for i, (c, p, k) in enumerate(zip(chrom.tolist(), pos.tolist(), kind.tolist()))))
            n += len(loci)
    return n


def fmt(values):
    v = sorted(values)
    return "%.1f [%.1f - %.1f]" % (v[len(v) // 2], v[0], v[-1])


def measure(sam, repeats, out_path):
    """In a process of its own: decode, then every case."""
    from miso_amd import capi, sam_utils
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    t0 = time.time()
    f = sam_utils.Samfile(sam)
    say("records %d, decode %.3f s (SAM text, %.0f MB)" % (len(f), time.time() - t0, os.path.getsize(sam) / 1e6))
    for n_regions, budget in ((1000, 0), (LOCI, 0), (LOCI, 256 << 20)):
        names = ["chr%d" % (k // (LOCI // NCHR) + 1) for k in range(n_regions)]
        starts = [locus_start(k) for k in range(n_regions)]
        ends = [s + SPAN - 1 for s in starts]
        stats, walls = [], []
        for rep in range(repeats + 1):                       # the first call warms up (HIP start-up, pinned buffers)
            t0 = time.time()
            depth, wiggle, jxns, st = capi.region_densities(f, names, starts, ends, accum_bytes=budget)
            if rep:
                stats.append(st)
                walls.append(1e3 * (time.time() - t0))
        say("regions %d, budget %s: groups %d, chunks %d, qlen classes %d, fetched %d, junctions %d, covered bases %d"
            % (n_regions, "%d MiB" % (budget >> 20) if budget else "default (1 GiB)", st["groups"], st["chunks"],
               st["qlen_classes"], st["fetched"], sum(len(j) for j in jxns), sum(int((d > 0).sum()) for d in depth)))
        say("    ms, median [min - max] of %d: tables %s | mark pass %s | group passes %s | scan + finish %s | junctions %s "
            "| copy back %s | call %s | call + Python lists %s"
            % (repeats, fmt([s["tables_ms"] for s in stats]), fmt([s["mark_ms"] for s in stats]),
               fmt([s["records_ms"] for s in stats]), fmt([s["scan_ms"] for s in stats]),
               fmt([s["junction_ms"] for s in stats]), fmt([s["copy_ms"] for s in stats]),
               fmt([s["total_ms"] for s in stats]), fmt(walls)))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as o:
            o.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=20000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--keep", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_density.txt"))
    ap.add_argument("--measure", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.measure:
        return measure(a.measure, a.repeats, a.out)
    work = a.keep or tempfile.mkdtemp(prefix="miso_density_")
    os.makedirs(work, exist_ok=True)
    sam = os.path.join(work, "reads.sam")
    t0 = time.time()
    n = generate(sam, a.records)
    print("generated %d records in %.1f s" % (n, time.time() - t0), flush=True)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--measure", sam, "--repeats", str(a.repeats),
                          "--out", a.out], env=env)
    if not a.keep:
        shutil.rmtree(work, ignore_errors=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
