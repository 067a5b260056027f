#!/usr/bin/env python3
"""Times `--summarize-samples` over an existing MISO output tree with the `host` and the `device` text decoder, on the
unpacked tree (`.miso` files) and on its packed form (`.miso_db`, miso_amd/miso_pack.py), and `--pack` itself.

    python tools/miso_text_bench.py [--events 40000] [--rows 2700] [--repeats 3] [--out profiles/miso_text.txt]

The tree is generated here (seeded, nothing downloaded): --events two-isoform events of --rows sample rows each
(MISO's default settings give 6 chains x (5000 - 500) / 10 = 2700), rows "0.1234,0.8766<TAB>-1234.56", spread over 24
chromosome directories.  One warm-up round, then --repeats rounds; a round runs the four configurations one after the
other (host / device x unpacked / packed), so that drift of the machine hits all of them alike.  Reported per
configuration: wall time end to end (mean, min, max), wall time per stage as samples_utils counts them, and for the
device decoder the decode kernels' own time (HIP events) with the bytes it moved -- text read plus samples written --
per second, beside the HBM peak.  The last line applies the rule by which the default decoder is chosen: `device` only
if it beats `host` end to end on the unpacked tree by more than the spread of the repeats.

Without a device the tool still generates, packs, lists, reads and shapes the tree, and says where it stopped.
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from miso_amd import capi, miso_pack, samples_utils  # noqa: E402

HBM_PEAK_TBS = 8.0          # MI355X HBM3E, spec; about 6.3 TB/s is what a copy kernel reaches
N_CHROMS = 24
HEADER = ("#isoforms='%s.A','%s.B'\texon_lens=('e1',120),('e2',90),('e3',150)\titers=5000\tburn_in=500\tlag=10\t"
          "percent_accept=97.31\tproposal_type=drift\tcounts=(0,1):31,(1,0):12,(1,1):204\tassigned_counts=0:140,1:107\t"
          "chrom=%s\tstrand=+\tmRNA_starts=1000,1000\tmRNA_ends=9000,9000\nsampled_psi\tlog_score\n")


def event_rows(rng, rows):
    """rows x 23 bytes: "d.dddd,d.dddd<TAB>-dddd.dd<LF>" with psi_2 = 1 - psi_1, all by digit arithmetic."""
    a = rng.integers(0, 10001, size=rows)
    s = rng.integers(100000, 1000000, size=rows)
    out = np.empty((rows, 23), np.uint8)

    def put(col, v, width):                                  # v as `width` digits ending at column col + width - 1
        for i in range(width):
            out[:, col + width - 1 - i] = 48 + v % 10
            v = v // 10

    for col, v in ((0, a), (7, 10000 - a)):
        put(col, v // 10000, 1)
        out[:, col + 1] = ord(".")
        put(col + 2, v % 10000, 4)
    out[:, 6] = ord(",")
    out[:, 13] = ord("\t")
    out[:, 14] = ord("-")
    put(15, s // 100, 4)
    out[:, 19] = ord(".")
    put(20, s % 100, 2)
    out[:, 22] = ord("\n")
    return out.tobytes()


def generate(roots, events, rows, seed):
    """The same tree under every root.  Returns (files, bytes) of one of them."""
    rng = np.random.default_rng(seed)
    for root in roots:
        for c in range(N_CHROMS):
            os.makedirs(os.path.join(root, "chr%d" % (c + 1)))
    total = 0
    for e in range(events):
        chrom = "chr%d" % (e % N_CHROMS + 1)
        name = "ev%06d" % e
        data = (HEADER % (name, name, chrom)).encode() + event_rows(rng, rows)
        total += len(data)
        for root in roots:
            with open(os.path.join(root, chrom, name + ".miso"), "wb") as f:
                f.write(data)
    return events, total


def tree_size(root):
    files = size = 0
    for base, _, names in os.walk(root):
        for n in names:
            files += 1
            size += os.path.getsize(os.path.join(base, n))
    return files, size


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--events", type=int, default=40000)
    ap.add_argument("--rows", type=int, default=2700)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--workdir", default=None, help="where the trees go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args(argv)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    work = a.workdir or tempfile.mkdtemp(prefix="miso_text_bench_")
    os.makedirs(work, exist_ok=True)
    trees = {"unpacked": os.path.join(work, "unpacked", "sample"), "packed": os.path.join(work, "packed", "sample")}
    try:
        say("# miso_text_bench: %d events x %d rows, 2 isoforms, seed %d, %d repeats after one warm-up; %d host threads"
            % (a.events, a.rows, a.seed, a.repeats, capi.usable_threads()))
        t0 = time.perf_counter()
        generate(list(trees.values()), a.events, a.rows, a.seed)
        say("generate (both trees)      %8.2f s" % (time.perf_counter() - t0))
        t0 = time.perf_counter()
        failed = miso_pack.pack_dirs([trees["packed"]])
        t_pack = time.perf_counter() - t0
        if failed:
            say("pack FAILED for %d directories" % failed)
            return 1
        (uf, ub), (pf, pb) = tree_size(trees["unpacked"]), tree_size(trees["packed"])
        say("pack                       %8.2f s  (%.1f MB/s of text)" % (t_pack, ub / 1e6 / t_pack))
        say("unpacked tree              %8d files %10.1f MB" % (uf, ub / 1e6))
        say("packed tree                %8d files %10.1f MB" % (pf, pb / 1e6))
        if capi.device_count() < 1:
            for form, root in trees.items():
                t0 = time.perf_counter()
                files, rows = samples_utils.list_events(root)
                t1 = time.perf_counter()
                evs = samples_utils._read_events(files, rows)
                t2 = time.perf_counter()
                samples_utils._shape(evs)
                t3 = time.perf_counter()
                ok = all(e.K == 2 and e.S == a.rows for e in evs) and len(evs) == a.events
                say("%-9s list %.2f s, read %.2f s, shape %.2f s: %d events, shapes %s"
                    % (form, t1 - t0, t2 - t1, t3 - t2, len(evs), "ok" if ok else "WRONG"))
            say("no HIP device: the summaries have no CPU path; stopped before the first decode")
            return 0
        configs = [(d, f) for f in ("unpacked", "packed") for d in ("host", "device")]
        wall = {c: [] for c in configs}
        stages = {c: [] for c in configs}
        kern = {c: [] for c in configs}
        tables = {}
        for rep in range(a.repeats + 1):
            for c in configs:
                decoder, form = c
                out = os.path.join(work, "out", decoder, form, "sample.miso_summary")
                t0 = time.perf_counter()
                n = samples_utils.summarize_sampler_results(trees[form], out, device=a.device, decoder=decoder)
                dt = time.perf_counter() - t0
                st = dict(samples_utils.last_decode_stats)
                tables[c] = open(out, "rb").read()
                if n != a.events or (decoder == "device" and st["fallback_events"]):
                    say("WRONG: %s/%s summarized %d of %d events, %d fell back"
                        % (decoder, form, n, a.events, len(st["fallback_events"])))
                    return 1
                say("%s %-6s %-8s %8.2f s   %s" % ("warm-up" if rep == 0 else "round %d" % rep, decoder, form, dt,
                                                    " ".join("%s=%.2f" % kv for kv in st["stage_s"].items())))
                if rep:
                    wall[c].append(dt); stages[c].append(st["stage_s"]); kern[c].append(st)
        if len(set(tables.values())) != 1:
            say("WRONG: the four tables differ")
            return 1
        say()
        say("# --summarize-samples end to end, wall seconds over %d rounds (the four tables are byte-identical)" % a.repeats)
        for c in configs:
            w = wall[c]
            say("%-6s %-8s mean %8.2f  min %8.2f  max %8.2f   stages (mean): %s"
                % (c[0], c[1], np.mean(w), min(w), max(w),
                   " ".join("%s=%.2f" % (k, np.mean([s[k] for s in stages[c]])) for k in stages[c][0])))
        say()
        say("# the decode kernels alone (HIP events, summed over the chunks), text read + samples written")
        for c in configs:
            if c[0] != "device":
                continue
            ms = [k["kernel_ms"] for k in kern[c]]
            moved = kern[c][0]["text_bytes"] + kern[c][0]["sample_bytes"]
            cp = [k["decode_ms"] for k in kern[c]]
            say("device %-8s kernels %8.2f ms (min %.2f max %.2f), with the copies %8.2f ms, %d chunks; %.1f MB text + %.1f MB "
                "samples: %.1f GB/s = %.1f %% of the %.1f TB/s HBM peak"
                % (c[1], np.mean(ms), min(ms), max(ms), np.mean(cp), kern[c][0]["chunks"], kern[c][0]["text_bytes"] / 1e6,
                   kern[c][0]["sample_bytes"] / 1e6, moved / 1e6 / np.mean(ms), moved / 1e7 / np.mean(ms) / HBM_PEAK_TBS,
                   HBM_PEAK_TBS))
        h, d = wall["host", "unpacked"], wall["device", "unpacked"]
        spread = max(max(h) - min(h), max(d) - min(d))
        gain = np.mean(h) - np.mean(d)
        say()
        say("# rule: unpacked tree, host %.2f s - device %.2f s = %.2f s against a spread of %.2f s -> default decoder: %s"
            % (np.mean(h), np.mean(d), gain, spread, "device" if gain > spread else "host"))
        return 0
    finally:
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        if not a.workdir:
            shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
