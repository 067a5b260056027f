#!/usr/bin/env python3
"""GPU: per-phase shader cycles of the two-isoform step on the headline batch (40 000 single-end events x 1000 reads, 7500
iterations, one chain), in the planner's own launch.  Needs the -DMISO_K2_PROFILE build:

    tools/build_prof.sh && MISO_AMD_LIB=tools/_build/libmiso_prof.so python3 tools/k2_phase_cycles.py [--events N] [--out FILE]

Every event's first chain leaves its wavefront's counters in loglik[0..4] (kernels_k2.inl): cycles spent between the phase
marks, summed over the run's iterations -- wall cycles of that wavefront, its SIMD partner's issue included.  Printed: the
mean over a sample of events (every --stride-th), per iteration."""
import argparse
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from miso_amd import capi, workload  # noqa: E402

PHASES = ("pf_mh", "pf_thr", "pf_loop", "pf_red", "pf_rec")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=40000)
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=7500)
    ap.add_argument("--burn", type=int, default=2500)
    ap.add_argument("--stride", type=int, default=97, help="every stride-th event is read")
    ap.add_argument("--warm", type=int, default=1, help="launches in front of the one that is read (a process's first runs on a cold device)")
    ap.add_argument("--out")
    a = ap.parse_args()
    b = workload.build_batch(0, a.events, n_reads=a.reads, iters=a.iters, burn=a.burn)
    b.upload(0)
    for _ in range(a.warm + 1):
        b.launch(seed=42)
        ms = b.sync()
    b.download()
    rows = collections.defaultdict(list)
    for i in range(0, a.events, a.stride):
        r = b.result(i)
        rows["all"].append(np.asarray(r.loglik[:5], dtype=np.float64))
    lines = ["%s  |  %s  |  kernel %.2f ms  |  %d events x %d reads, %d iterations"
             % (os.environ.get("MISO_AMD_LIB", "libmiso_amd.so"), b.last_kernels(), ms, a.events, a.reads, a.iters)]
    for key, v in rows.items():
        m = np.mean(v, axis=0) / a.iters
        lines.append("%-4s n=%-5d " % (key, len(v)) + "  ".join("%s %8.1f" % (p, x) for p, x in zip(PHASES, m))
                     + "  sum %8.1f cycles per wavefront-iteration" % m.sum())
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
