#!/usr/bin/env python3
"""Times the comparison of two groups of replicate samples over existing MISO output trees, two ways: the n1 x n2 pairwise
`output_samples_comparison` calls (what `--compare-samples` per pair costs, and all there was before `--compare-groups`),
and one `output_group_comparisons`; and the group kernel alone with each of its LDS staging choices.

    python tools/compare_groups_bench.py [--events 40000] [--rows 2700] [--group 3] [--repeats 3] [--out profiles/compare_groups.txt]

The trees are generated here (seeded, nothing downloaded) as tools/miso_text_bench.py makes its tree: --group + --group
sample directories of --events two-isoform events with --rows sample rows each (MISO's default settings give 2700), every
sample with its own uniform psi -- so every (event, isoform, pair) takes the kernel-density branch with its S calls of
miso_det_exp, the expensive one.  One warm-up round, then --repeats rounds; a round runs the pairwise calls and then the
group pass, so that drift of the machine hits both alike.  Reported: wall seconds end to end (mean, min, max), the stages as
samples_utils counts them, and whether the tables agree byte for byte.  The last line applies the rule of DESIGN.md
section 13: the group pass counts as faster only if it wins by more than the spread of the repeats.

The staging part decodes one chunk of events of every sample and times capi.compare_groups(staging=...) on it (the
kernel's own time, HIP events) beside the n1 x n2 Batch.compare calls (wall time: they allocate, launch, copy and wait).
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from miso_amd import capi, samples_utils  # noqa: E402
from miso_text_bench import HEADER, N_CHROMS, event_rows  # noqa: E402


def generate(root, events, rows, seed):
    rng = np.random.default_rng(seed)
    for c in range(N_CHROMS):
        os.makedirs(os.path.join(root, "chr%d" % (c + 1)))
    total = 0
    for e in range(events):
        chrom = "chr%d" % (e % N_CHROMS + 1)
        name = "ev%06d" % e
        data = (HEADER % (name, name, chrom)).encode() + event_rows(rng, rows)
        total += len(data)
        with open(os.path.join(root, chrom, name + ".miso"), "wb") as f:
            f.write(data)
    return total


def stages_line(st):
    return " ".join("%s=%.2f" % kv for kv in st.items())


def staging_part(say, trees, events, rows, device, repeats):
    """One chunk of every sample on the device; the kernel with each staging, and the pairwise calls."""
    n = min(events, 4000)
    names = ["ev%06d" % e for e in range(n)]
    batches = []
    for group in trees:
        batches.append([])
        for tree in group:
            src = samples_utils._sources(tree)
            evs = samples_utils._read_events(*samples_utils._read_named(src, names))
            samples_utils._shape(evs)
            evs.sort(key=lambda e: e.name)
            text, offs = samples_utils._joined(evs)
            batches[-1].append(capi.SamplesBatch.from_text(text, offs, [e.K for e in evs], rows, device=device))
    n1, n2 = len(batches[0]), len(batches[1])
    say()
    say("# the comparison alone: %d events x 2 isoforms x %d rows, %d x %d samples; ms, %d repeats after one warm-up"
        % (n, rows, n1, n2, repeats))
    ref = first = None
    for staging in ("both", "smaller", "none", "auto"):
        ms = []
        try:
            for rep in range(repeats + 1):
                g = capi.compare_groups(batches[0], batches[1], staging=staging)
                if rep:
                    ms.append(g.kernel_ms)
        except capi.InternalError as err:
            say("group kernel, staging %-8s does not run: %s" % (staging, str(err).split(": ")[-1]))
            continue
        same = ref is None or np.array_equal(g.out.view(np.uint64), ref.view(np.uint64))
        if ref is None:
            ref, first = g.out, g
        say("group kernel, staging %-8s mean %8.2f  min %8.2f  max %8.2f   %s"
            % (staging, np.mean(ms), min(ms), max(ms), "same bits" if same else "BITS DIFFER"))
    wall = []
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        for b1 in batches[0]:
            for b2 in batches[1]:
                b1.compare(b2, 0.3)
        if rep:
            wall.append(1e3 * (time.perf_counter() - t0))
    some = range(0, n, max(1, n // 50))          # (the last pair's results are still in its first batch)
    pair = np.concatenate([np.concatenate(batches[0][-1].comparison(e)) for e in some])
    got = np.concatenate([np.concatenate(first.comparison(n1 - 1, n2 - 1, e)) for e in some])
    say("%d pairwise compare calls (wall)  mean %8.2f  min %8.2f  max %8.2f   %s"
        % (n1 * n2, np.mean(wall), min(wall), max(wall),
           "same bits as the group kernel" if np.array_equal(pair.view(np.uint64), got.view(np.uint64)) else "BITS DIFFER"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--events", type=int, default=40000)
    ap.add_argument("--rows", type=int, default=2700)
    ap.add_argument("--group", type=int, default=3, help="samples per group")
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

    work = a.workdir or tempfile.mkdtemp(prefix="compare_groups_bench_")
    os.makedirs(work, exist_ok=True)
    labels = [["ctl%d" % (i + 1) for i in range(a.group)], ["kd%d" % (i + 1) for i in range(a.group)]]
    trees = [[os.path.join(work, "trees", lab) for lab in group] for group in labels]
    try:
        say("# compare_groups_bench: %d + %d samples of %d events x %d rows, 2 isoforms, seed %d, %d repeats after one warm-up; "
            "%d host threads" % (a.group, a.group, a.events, a.rows, a.seed, a.repeats, capi.usable_threads()))
        t0 = time.perf_counter()
        size = sum(generate(tree, a.events, a.rows, a.seed + 17 * k) for k, tree in enumerate(trees[0] + trees[1]))
        say("generate (%d trees, %.1f MB)  %8.2f s" % (2 * a.group, size / 1e6, time.perf_counter() - t0))
        if capi.device_count() < 1:
            listings = []
            for group in trees:
                listings.append([])
                for tree in group:
                    src = samples_utils._sources(tree)
                    evs = samples_utils._read_events(*samples_utils._read_named(src, sorted(src)))
                    samples_utils._shape(evs)
                    listings[-1].append([(e.name, e.K, e.S, True, len(e.body)) for e in evs])
            plan = samples_utils.plan_group_comparison(*listings)
            say("plan: %d chunks, %d events on the group route" % (len(plan["chunks"]), sum(len(c["names"]) for c in plan["chunks"])))
            say("no HIP device: the comparison has no CPU path; stopped before the first decode")
            return 0
        wall = {"pairwise": [], "group": []}
        stages = {"pairwise": [], "group": []}
        for rep in range(a.repeats + 1):
            tag = "warm-up" if rep == 0 else "round %d" % rep
            out = os.path.join(work, "out", "pairwise")
            st_sum, tables = {}, {}
            t0 = time.perf_counter()
            for i, d1 in enumerate(trees[0]):
                for j, d2 in enumerate(trees[1]):
                    path, n = samples_utils.output_samples_comparison(d1, d2, out, sample_labels=(labels[0][i], labels[1][j]),
                                                                      device=a.device)
                    for k, v in samples_utils.last_decode_stats["stage_s"].items():
                        st_sum[k] = st_sum.get(k, 0.0) + v
                    tables[i, j] = (path, n)
            dt = time.perf_counter() - t0
            say("%s pairwise x %d  %8.2f s   %s" % (tag, a.group * a.group, dt, stages_line(st_sum)))
            if rep:
                wall["pairwise"].append(dt); stages["pairwise"].append(st_sum)
            out = os.path.join(work, "out", "group")
            t0 = time.perf_counter()
            done = samples_utils.output_group_comparisons(trees[0], trees[1], out, labels[0], labels[1], device=a.device)
            dt = time.perf_counter() - t0
            st = dict(samples_utils.last_decode_stats)
            say("%s group         %8.2f s   %s   (%d chunks, compare kernels %.1f ms)"
                % (tag, dt, stages_line(st["stage_s"]), st["group_chunks"], st["compare_kernel_ms"]))
            if rep:
                wall["group"].append(dt); stages["group"].append(st["stage_s"])
            pairs = [(i, j) for i in range(a.group) for j in range(a.group)]
            for (path, n), p in zip(done, pairs):
                if n != a.events or tables[p][1] != n or open(path, "rb").read() != open(tables[p][0], "rb").read():
                    say("WRONG: pair %r: the group table (%d rows) is not the pairwise table (%d rows)" % (p, n, tables[p][1]))
                    return 1
            if st["group_events"] != a.events or st["fallback_events"] or st["pair_route_events"]:
                say("WRONG: %d of %d events took the group route" % (st["group_events"], a.events))
                return 1
        say()
        say("# end to end, wall seconds over %d rounds (all %d tables byte-identical between the two routes)"
            % (a.repeats, a.group * a.group))
        for k in ("pairwise", "group"):
            w = wall[k]
            say("%-9s mean %8.2f  min %8.2f  max %8.2f   stages (mean): %s"
                % (k, np.mean(w), min(w), max(w), " ".join("%s=%.2f" % (s, np.mean([x[s] for x in stages[k]])) for s in stages[k][0])))
        p, g = wall["pairwise"], wall["group"]
        spread = max(max(p) - min(p), max(g) - min(g))
        gain = np.mean(p) - np.mean(g)
        say()
        say("# rule: pairwise %.2f s - group %.2f s = %.2f s against a spread of %.2f s (%.2fx) -> the group pass is %s"
            % (np.mean(p), np.mean(g), gain, spread, np.mean(p) / np.mean(g), "faster" if gain > spread else "NOT faster"))
        staging_part(say, trees, a.events, a.rows, a.device, a.repeats)
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
