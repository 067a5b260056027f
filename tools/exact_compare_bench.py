"""The exact comparison against its two yardsticks on the headline-shaped workload as TWO samples (bench.py's BASE_SHAPE:
40 000 single-end two-isoform events x 1000 reads, 7500 iterations, 2500 of them burn-in, one chain: S = 5000 rows per
event and sample), in one process: both samples run with exact=True (sample 2 is the same list of genes, its reads simulated with
the two isoforms' expression swapped and another seed, so every pair has its gene's effective lengths and another psi), then

    exact_compare at n_z = 0 and n_z = 4    the HIP-event time of the kernel (miso_batch_compare_ms),
    compare_kernel                           the sampled (KDE) comparison miso_batch_compare of the same two batches,
    exact_sample                             sample 1's launch (miso_batch_sync),

each the minimum of `--steps` after a warm-up.

    python tools/exact_compare_bench.py [--events 40000] [--reads 1000] [--iters 7500 --burn 2500 --lag 1 --chains 1]
                                        [--steps 5] [--out profiles/exact_compare.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_pair(events, reads, **kw):
    """two exact batches over the same genes, another psi and other reads in sample 2"""
    from miso_amd import capi, workload
    bs = [capi.Batch(36, exact=True, **kw) for _ in (0, 1)]
    for e in range(events):
        exons, isoforms, expr = workload.event_gene(e, 2)
        g = capi.Gene(exons, isoforms)
        for s, b in enumerate(bs):     # (sample 2: the isoforms' expression swapped)
            b.add_simulated(g, expr if s == 0 else expr[::-1].copy(), workload.event_n_reads(e, reads),
                            workload.GEN_SEED + e + s * events)
    return bs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=40000)
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=7500)
    ap.add_argument("--burn", type=int, default=2500)
    ap.add_argument("--lag", type=int, default=1)
    ap.add_argument("--chains", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_compare.txt"))
    a = ap.parse_args()
    from miso_amd import capi
    if capi.device_count() < 1:
        print("exact_compare_bench: no HIP device -- nothing is measured without one")
        return 1
    S = a.chains * (a.iters - a.burn) // a.lag
    lines = ["exact_compare_bench: two samples of %d events x %d reads, %d iterations (%d burn-in, lag %d), %d chain(s): "
             "S = %d rows per event and sample" % (a.events, a.reads, a.iters, a.burn, a.lag, a.chains, S)]
    t0 = time.time()
    b1, b2 = build_pair(a.events, a.reads, iters=a.iters, burn=a.burn, lag=a.lag, chains=a.chains)
    for b in (b1, b2):
        b.upload(0)
    t_build = time.time() - t0
    sample_ms = []
    for step in range(a.steps + 1):
        b1.launch(seed=1, first_event_id=0)
        ms = b1.sync()
        if step:
            sample_ms.append(ms)
    b2.launch(seed=2, first_event_id=0)
    b2.sync()

    def timed(call, pick):
        out = []
        for step in range(a.steps + 1):
            call()
            if step:
                out.append(pick())
        return out
    z4 = [0.1, -0.1, 0.2, -0.2]
    rows = [("exact_compare, n_z = 0", timed(lambda: b1.compare_exact(b2, []), lambda: b1.compare_ms()[1])),
            ("exact_compare, n_z = 4", timed(lambda: b1.compare_exact(b2, z4), lambda: b1.compare_ms()[1])),
            ("compare_kernel (KDE, smoothing 0.3)", timed(lambda: b1.compare(b2, 0.3), lambda: b1.compare_ms()[0])),
            ("exact_sample (sample 1's launch)", sample_ms)]
    n_pairs = sum(b1.exact_comparison(i) is not None for i in range(0, a.events, max(1, a.events // 1000)))
    for name, ms in rows:
        lines.append("%-38s kernel ms min %.3f median %.3f max %.3f (%d runs) | %.0f pairs/s at the minimum"
                     % (name, min(ms), sorted(ms)[len(ms) // 2], max(ms), len(ms), a.events / (min(ms) * 1e-3)))
    x0, x4, kde, smp = (min(ms) for _, ms in rows)
    lines.append("exact_compare: three tabulations %.3f ms (%.2f x the exact_sample launch of S rows), %.3f ms per delta psi "
                 "point; exact comparison at n_z = 4 / KDE comparison: %.1f x" % (x0, x0 / smp, (x4 - x0) / 4, x4 / kde))
    lines.append("every sampled pair comparable: %s; batches built in %.1f s" % (n_pairs == len(range(0, a.events, max(1, a.events // 1000))), t_build))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
