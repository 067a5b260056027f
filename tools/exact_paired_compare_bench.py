"""The paired-end exact comparison against its yardsticks on bench.py's paired-end two-isoform shape as TWO samples (40 000
events x 1000 read pairs, 7500 iterations, 2500 of them burn-in, one chain: S = 5000 rows per event and sample), in one
process: both samples run with exact_paired=True (sample 2 is the same list of genes, its pairs simulated with the two
isoforms' expression swapped, another seed and another fragment-length spread, so every pair of posteriors has its own
A and its own pairs), then

    exact_paired_compare at n_z = 0 and n_z = 4    the HIP-event time of the kernel (miso_batch_compare_ms),
    compare_kernel                                  the sampled (KDE) comparison miso_batch_compare of the same two batches,
    exact_paired_sample                             sample 1's launch (miso_batch_sync),
    exact_paired_sample, one row                    the same events with S = 1: the posterior stage,

each the minimum of `--steps` after a warm-up.

    python tools/exact_paired_compare_bench.py [--events 40000] [--pairs 1000] [--iters 7500 --burn 2500 --lag 1 --chains 1]
                                               [--steps 5] [--out profiles/exact_paired_compare.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARS = (900.0, 1600.0)      # the two samples' fragment-length variances


def build_sample(s, events, pairs, **kw):
    """sample s = 0, 1 over the same genes: another psi, other pairs and another fragment-length law in sample 2"""
    from miso_amd import capi, workload
    b = capi.Batch(36, paired=True, mean=250.0, var=VARS[s], exact_paired=True, **kw)
    for e in range(events):
        exons, isoforms, expr = workload.event_gene(e, 2, min_len=400, max_len=800, gap=300)
        b.add_simulated(capi.Gene(exons, isoforms), expr if s == 0 else expr[::-1].copy(), workload.event_n_reads(e, pairs),
                        workload.GEN_SEED + e + s * events)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=40000)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=7500)
    ap.add_argument("--burn", type=int, default=2500)
    ap.add_argument("--lag", type=int, default=1)
    ap.add_argument("--chains", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_paired_compare.txt"))
    a = ap.parse_args()
    from miso_amd import capi
    if capi.device_count() < 1:
        print("exact_paired_compare_bench: no HIP device -- nothing is measured without one")
        return 1
    S = a.chains * (a.iters - a.burn) // a.lag
    lines = ["exact_paired_compare_bench: two samples of %d paired-end events x %d read pairs, %d iterations (%d burn-in, lag %d), "
             "%d chain(s): S = %d rows per event and sample" % (a.events, a.pairs, a.iters, a.burn, a.lag, a.chains, S)]
    t0 = time.time()
    b1, b2 = (build_sample(s, a.events, a.pairs, iters=a.iters, burn=a.burn, lag=a.lag, chains=a.chains) for s in (0, 1))
    one = build_sample(0, a.events, a.pairs, iters=a.burn + a.lag, burn=a.burn, lag=a.lag, chains=1)
    for b in (b1, b2, one):
        b.upload(0)
    t_build = time.time() - t0

    def launches(b, seed):
        out = []
        for step in range(a.steps + 1):
            b.launch(seed=seed, first_event_id=0)
            ms = b.sync()
            if step:
                out.append(ms)
        return out
    sample_ms = launches(b1, 1)
    one_ms = launches(one, 1)
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
    rows = [("exact_paired_compare, n_z = 0", timed(lambda: b1.compare_exact_paired(b2, []), lambda: b1.compare_ms()[1])),
            ("exact_paired_compare, n_z = 4", timed(lambda: b1.compare_exact_paired(b2, z4), lambda: b1.compare_ms()[1])),
            ("compare_kernel (KDE, smoothing 0.3)", timed(lambda: b1.compare(b2, 0.3), lambda: b1.compare_ms()[0])),
            ("exact_paired_sample (sample 1's launch)", sample_ms),
            ("exact_paired_sample, one row (posterior stage)", one_ms)]
    probe = range(0, a.events, max(1, a.events // 1000))
    n_pairs = sum(b1.exact_comparison(i) is not None for i in probe)
    for name, ms in rows:
        lines.append("%-46s kernel ms min %.3f median %.3f max %.3f (%d runs) | %.0f pairs/s at the minimum"
                     % (name, min(ms), sorted(ms)[len(ms) // 2], max(ms), len(ms), a.events / (min(ms) * 1e-3)))
    x0, x4, kde, smp, stage = (min(ms) for _, ms in rows)
    lines.append("exact_paired_compare: windows and tables of three densities %.3f ms = %.2f x the one-row posterior stage "
                 "(%.2f x the exact_paired_sample launch of S rows), %.3f ms per delta psi point; at n_z = 4 / KDE comparison: %.1f x"
                 % (x0, x0 / stage, x0 / smp, (x4 - x0) / 4, x4 / kde))
    lines.append("every sampled pair comparable: %s; batches built and uploaded in %.1f s" % (n_pairs == len(probe), t_build))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
