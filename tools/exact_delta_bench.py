"""The quantiles of delta psi from the exact CDF against their yardsticks, on the shapes of
tools/exact_compare_bench.py and tools/exact_paired_compare_bench.py -- bench.py's two-isoform shapes as TWO samples, 40 000
events x 1000 reads (single-end) or read pairs (paired-end), 7500 iterations, 2500 of them burn-in, one chain: S = 5000 rows
per event and sample --, both kinds in one process, each kind's batches built by that tool's own function:

    exact_delta_quantiles / exact_paired_delta_quantiles at p = (0.5, 0.025, 0.975)    miso_batch_exact_delta_ms,
    exact_compare / exact_paired_compare at n_z = 0 and n_z = 4                         miso_batch_compare_ms,
    compare_pairs at S = 5000 (the sampled delta psi over all pairs)                    miso_batch_compare_pairs_ms,

HIP-event kernel times, each the minimum of `--steps` after a warm-up.

    python tools/exact_delta_bench.py [--events 40000] [--reads 1000] [--iters 7500 --burn 2500 --lag 1 --chains 1]
                                      [--steps 5] [--kinds single paired] [--out profiles/exact_delta.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PROBS = (0.5, 0.025, 0.975)
EVALUATIONS = 1 + 8 + 32 * len(PROBS)      # of H per pair


def measure(kind, a, lines):
    import exact_compare_bench
    import exact_paired_compare_bench
    shape = dict(iters=a.iters, burn=a.burn, lag=a.lag, chains=a.chains)
    t0 = time.time()
    if kind == "single":
        b1, b2 = exact_compare_bench.build_pair(a.events, a.reads, **shape)
    else:
        b1, b2 = (exact_paired_compare_bench.build_sample(s, a.events, a.reads, **shape) for s in (0, 1))
    for s, b in enumerate((b1, b2)):
        b.upload(0)
        b.launch(seed=1 + s, first_event_id=0)
        b.sync()
    t_build = time.time() - t0
    compare = b1.compare_exact if kind == "single" else b1.compare_exact_paired
    names = ("exact_compare", "exact_delta_quantiles") if kind == "single" else ("exact_paired_compare", "exact_paired_delta_quantiles")

    def timed(call, pick):
        out = []
        for step in range(a.steps + 1):
            call()
            if step:
                out.append(pick())
        return out
    z4 = [0.1, -0.1, 0.2, -0.2]
    rows = [("%s, n_z = 0" % names[0], timed(lambda: compare(b2, []), lambda: b1.compare_ms()[1])),
            ("%s, n_z = 4" % names[0], timed(lambda: compare(b2, z4), lambda: b1.compare_ms()[1])),
            ("%s, n_p = 3" % names[1], timed(lambda: b1.exact_delta_quantiles(b2, PROBS), b1.exact_delta_ms)),
            ("compare_pairs (all pairs of the draws)", timed(lambda: b1.compare_pairs(b2, 0.95, (0.1, 0.2)), b1.compare_pairs_ms))]
    probe = range(0, a.events, max(1, a.events // 1000))
    n_pairs = sum(b1.exact_delta(i) is not None for i in probe)
    for name, ms in rows:
        lines.append("%-46s kernel ms min %.3f median %.3f max %.3f (%d runs) | %.0f pairs/s at the minimum"
                     % (name, min(ms), sorted(ms)[len(ms) // 2], max(ms), len(ms), a.events / (min(ms) * 1e-3)))
    x0, x4, dq, cp = (min(ms) for _, ms in rows)
    per_point = (x4 - x0) / 4
    lines.append("%s: %.3f ms = %.2f x %s at n_z = 4, %.2f x compare_pairs; %s costs %.3f ms per delta psi point, so %d evaluations "
                 "of H one at a time would take %.1f ms: the eight-wide sweeps take %.2f x that (tables included)"
                 % (names[1], dq, dq / x4, names[0], dq / cp, names[0], per_point, EVALUATIONS, EVALUATIONS * per_point,
                    dq / (EVALUATIONS * per_point)))
    lines.append("%s: every sampled pair comparable: %s; batches built, uploaded and sampled in %.1f s"
                 % (kind, n_pairs == len(probe), t_build))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=40000)
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=7500)
    ap.add_argument("--burn", type=int, default=2500)
    ap.add_argument("--lag", type=int, default=1)
    ap.add_argument("--chains", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--kinds", nargs="+", default=["single", "paired"], choices=["single", "paired"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_delta.txt"))
    a = ap.parse_args()
    from miso_amd import capi
    if capi.device_count() < 1:
        print("exact_delta_bench: no HIP device -- nothing is measured without one")
        return 1
    S = a.chains * (a.iters - a.burn) // a.lag
    lines = ["exact_delta_bench: two samples of %d events x %d reads (single-end) or read pairs (paired-end), %d iterations "
             "(%d burn-in, lag %d), %d chain(s): S = %d rows per event and sample; p = %s, %d evaluations of H per pair"
             % (a.events, a.reads, a.iters, a.burn, a.lag, a.chains, S, PROBS, EVALUATIONS)]
    for kind in a.kinds:
        measure(kind, a, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
