"""The isoform-group passes (part-level psi) beside the per-isoform passes they stand next to, on a whole-gene
batch of the shape bench.py's `pe_mix` row uses (paired-end, 3 - 20 isoforms per gene; fewer genes) at MISO's default
sampler settings (5000 iterations, 500 of them burn-in, lag 10, 6 chains: S = 2700 rows per event), as TWO samples, in one
process:

    summarize_isoform_groups        kernel time (HIP events) and the call's wall time from Python, one group per exon of
                                    every gene that some isoforms hold and some do not, every mask of a gene once
    summarize                       miso_batch_summarize of the same batch, one column per isoform
    compare_pairs_isoform_groups    the same groups over both samples, two thresholds: kernel and wall time
    compare_pairs                   miso_batch_compare_pairs of the same two batches, two thresholds

each the minimum of `--steps` after a warm-up.  Measured once; nothing is tuned against the numbers.

    python tools/part_psi_bench.py [--events 2048] [--reads 1000] [--steps 5] [--out profiles/part_psi.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K_RANGE = (3, 20)


def exon_groups(first_event_id, n_events):
    """(event, mask) per exon of every gene that some of its isoforms hold and some do not, every mask of a gene once"""
    from miso_amd import workload
    groups, n_iso = [], 0
    for i in range(n_events):
        ev = first_event_id + i
        exons, isoforms, _ = workload.event_gene(ev, workload.mixed_k(ev, K_RANGE), min_len=400, max_len=800, gap=300)
        n_iso += len(isoforms)
        seen = set()
        for j in range(len(exons)):
            mask = sum(1 << k for k, iso in enumerate(isoforms) if j in iso)
            if mask and mask != (1 << len(isoforms)) - 1 and mask not in seen:
                seen.add(mask)
                groups.append((i, mask))
    return groups, n_iso


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=2048)
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=5000)
    ap.add_argument("--burn", type=int, default=500)
    ap.add_argument("--lag", type=int, default=10)
    ap.add_argument("--chains", type=int, default=6)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "part_psi.txt"))
    a = ap.parse_args()
    from miso_amd import capi, workload
    if capi.device_count() < 1:
        print("part_psi_bench: no HIP device -- nothing is measured without one")
        return 1
    S = a.chains * (a.iters - a.burn) // a.lag
    t0 = time.time()
    batches = []
    for s in range(2):
        b = workload.build_batch(0, a.events, K=K_RANGE, n_reads=a.reads, iters=a.iters, burn=a.burn, lag=a.lag, chains=a.chains,
                                 paired=True)
        b.upload(0)
        b.launch(seed=1 + s, first_event_id=0)
        b.sync()
        batches.append(b)
    b1, b2 = batches
    t_build = time.time() - t0
    groups, n_iso = exon_groups(0, a.events)
    lines = ["part_psi_bench: two samples of %d paired-end genes of %d - %d isoforms x %d reads, %d iterations (%d burn-in, lag %d), "
             "%d chains: S = %d rows per event; %d isoform columns, %d isoform groups (exons with distinct masks)"
             % (a.events, K_RANGE[0], K_RANGE[1], a.reads, a.iters, a.burn, a.lag, a.chains, S, n_iso, len(groups))]

    def timed(call, kernel_ms):
        """[(kernel ms, wall ms)] of `steps` calls after one warm-up"""
        out = []
        for step in range(a.steps + 1):
            t = time.perf_counter()
            r = call()
            wall = (time.perf_counter() - t) * 1e3
            if step:
                out.append((kernel_ms(r), wall))
        return out
    rows = [("summarize_isoform_groups", len(groups), timed(lambda: b1.summarize_isoform_groups(groups, 0.95, as_text=True),
                                                            lambda r: r.kernel_ms)),
            ("summarize (as_text)", n_iso, timed(lambda: b1.summarize(0.95, as_text=True), lambda r: b1.pass_ms()[0])),
            ("compare_pairs_isoform_groups", len(groups),
             timed(lambda: capi.compare_pairs_isoform_groups(b1, b2, groups, 0.95, (0.1, 0.2), as_text=True), lambda r: r.kernel_ms)),
            ("compare_pairs (as_text)", n_iso, timed(lambda: b1.compare_pairs(b2, 0.95, (0.1, 0.2), as_text=True),
                                                     lambda r: b1.compare_pairs_ms()))]
    for name, n_cols, t in rows:
        k, w = min(x[0] for x in t), min(x[1] for x in t)
        lines.append("%-30s %7d columns | kernel ms min %.3f median %.3f | call wall ms min %.3f | %.2f us per column (kernel)"
                     % (name, n_cols, k, sorted(x[0] for x in t)[len(t) // 2], w, 1e3 * k / max(n_cols, 1)))
    got = b1.summarize_isoform_groups(groups[:1], 0.95, as_text=True)
    lines.append("group 0 (event %d, mask %#x): mean %.6f, interval [%.6f, %.6f]; batches built and sampled in %.1f s"
                 % (groups[0][0], groups[0][1], got.mean[0], got.ci_low[0], got.ci_high[0], t_build))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
