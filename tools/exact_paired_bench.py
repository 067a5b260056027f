"""The paired-end exact-posterior mode against the default paired sampler on bench.py's paired-end two-isoform shape
(40 000 events x 1000 pairs, fragment lengths 250 +- 30, 7500 iterations, 2500 of them burn-in, one chain: S = 5000 rows per
event), in one process: the same uploaded batch launched in the default mode and, after miso_batch_set_exact_paired, in the
exact mode -- `--steps` timed launches each after a warm-up, kernel time = the HIP-event time of the launch
(miso_batch_sync), the minimum reported.  Then a batch of the same events with ONE row per event (the posterior stage:
two window passes and the table, plus one draw), and the hg19-like pair-count batch (20 .. 10^5 pairs per event), where
one wavefront carries the largest event.

    python tools/exact_paired_bench.py [--events 40000] [--pairs 1000] [--iters 7500 --burn 2500 --lag 1 --chains 1]
                                       [--steps 5] [--no-hg19] [--out profiles/exact_paired.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(batch, steps, seed=1):
    """kernel ms of `steps` launches after a warm-up one"""
    batch.launch(seed=seed, first_event_id=0)
    batch.sync()
    ms = []
    for _ in range(steps):
        batch.launch(seed=seed, first_event_id=0)
        ms.append(batch.sync())
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=40000)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=7500)
    ap.add_argument("--burn", type=int, default=2500)
    ap.add_argument("--lag", type=int, default=1)
    ap.add_argument("--chains", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-hg19", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_paired.txt"))
    a = ap.parse_args()
    from miso_amd import capi, workload
    if capi.device_count() < 1:
        print("exact_paired_bench: no HIP device -- nothing is measured without one")
        return 1
    S = a.chains * (a.iters - a.burn) // a.lag
    lines = ["exact_paired_bench: %d paired-end events, %d iterations (%d burn-in, lag %d), %d chain(s): S = %d rows per event"
             % (a.events, a.iters, a.burn, a.lag, a.chains, S)]
    rows = {}

    def measure(label, batch, events):
        ms = timed(batch, a.steps)
        best, med = min(ms), sorted(ms)[len(ms) // 2]
        rows[label] = best
        ks = batch.launch_stats()["kernels"]
        lines.append("%-34s %-28s kernel ms min %.3f median %.3f max %.3f (%d launches) | %.0f events/s at the minimum | %s"
                     % (label, batch.last_kernels(), best, med, max(ms), len(ms), events / (best * 1e-3),
                        ", ".join("%s: %d events" % (k["name"], k["chains"]) for k in ks if k["name"].startswith("exact"))
                        or "no exact events"))

    shapes = [("%d pairs" % a.pairs, a.pairs)] + ([] if a.no_hg19 else [("hg19-like pair counts", workload.HG19_LIKE)])
    for tag, n_reads in shapes:
        t0 = time.time()
        b = workload.build_batch(0, a.events, K=2, n_reads=n_reads, lag=a.lag, chains=a.chains, paired=True,
                                 iters=a.iters, burn=a.burn)
        b.upload(0)
        lines.append("%s: batch built and uploaded in %.1f s" % (tag, time.time() - t0))
        measure("%s, default" % tag, b, a.events)
        b.set_exact_paired(True)
        measure("%s, exact_paired" % tag, b, a.events)
        lines.append("%s: default / exact_paired kernel time: %.2f x" % (tag, rows["%s, default" % tag] / rows["%s, exact_paired" % tag]))
        del b
    b = workload.build_batch(0, a.events, K=2, n_reads=a.pairs, lag=a.lag, chains=a.chains, paired=True,
                             iters=a.burn + a.lag, burn=a.burn, exact_paired=True)
    b.upload(0)
    measure("%d pairs, exact_paired, one row" % a.pairs, b, a.events)
    del b
    full, post = rows["%d pairs, exact_paired" % a.pairs], rows["%d pairs, exact_paired, one row" % a.pairs]
    lines.append("exact_paired kernel at %d pairs: posterior stage (+ one row) %.3f ms, the %d rows (inversion, pair sum of the "
                 "log score, stores) %.3f ms" % (a.pairs, post, S, full - post))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
