"""The pooled quantiles of delta psi of two groups of PAIRED-END replicates from the exact posteriors against
what the pairwise pass must do for the same pairs, in one process: DESIGN.md 19a's / 20a's workload made paired-end -- 8 000
two-isoform events x 1000 read pairs as 3 + 3 replicates, built like tools/exact_paired_compare_bench.py's samples --,

    exact_paired_delta_groups at p = (0.5, 0.025, 0.975), n_z = 0 and n_z = 4    miso_batch_exact_paired_delta_groups' kernel_ms,
    nine exact_paired_delta_quantiles launches, one per pair of replicates       the sum of miso_batch_exact_delta_ms,
    compare_pairs_groups at `--rows` draws per replicate (the sampled pooled pass)  its kernel_ms,

HIP-event kernel times, each the minimum of `--steps` after a warm-up, the first two alternated step by step.

    python tools/exact_paired_delta_groups_bench.py [--events 8000] [--pairs 1000] [--rows 2700 5000] [--steps 5]
                                                    [--note TEXT ...] [--out profiles/exact_paired_delta_groups.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROBS = (0.5, 0.025, 0.975)
Z4 = (0.1, -0.1, 0.2, -0.2)
N1 = N2 = 3
VARS = (900.0, 1600.0, 1225.0)      # the replicates' fragment-length variances, the same three in either group


def build_groups(events, pairs, rows):
    """3 + 3 paired exact batches over the same genes: group 2 with the isoforms' expression swapped, other read pairs and
    another fragment-length law in every replicate of a group"""
    from miso_amd import capi, workload
    bs = [capi.Batch(36, paired=True, mean=250.0, var=VARS[s % N1], exact_paired=True, iters=rows, burn=0, lag=1, chains=1)
          for s in range(N1 + N2)]
    for e in range(events):
        exons, isoforms, expr = workload.event_gene(e, 2, min_len=400, max_len=800, gap=300)
        g = capi.Gene(exons, isoforms)
        for s, b in enumerate(bs):
            b.add_simulated(g, expr if s < N1 else expr[::-1].copy(), workload.event_n_reads(e, pairs), workload.GEN_SEED + e + s * events)
    for s, b in enumerate(bs):
        b.upload(0)
        b.launch(seed=1 + s, first_event_id=0)
        b.sync()
    return bs[:N1], bs[N1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=8000)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--rows", type=int, nargs="+", default=[2700, 5000])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--note", action="append", default=[], metavar="TEXT",
                    help="a line to keep at the end of the record, e.g. bench.py's headline from a run of its own on the same "
                         "tree (may be given more than once)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_paired_delta_groups.txt"))
    a = ap.parse_args()
    from miso_amd import capi
    if capi.device_count() < 1:
        print("exact_paired_delta_groups_bench: no HIP device -- nothing is measured without one")
        return 1
    lines = ["exact_paired_delta_groups_bench: %d events x %d read pairs as %d + %d replicates; p = %s" % (a.events, a.pairs, N1, N2, PROBS)]
    for r, rows in enumerate(a.rows):
        t0 = time.time()
        g1, g2 = build_groups(a.events, a.pairs, rows)
        lines.append("%d rows per replicate: batches built, uploaded and sampled in %.1f s" % (rows, time.time() - t0))
        if r == 0:
            # (the pairwise quantiles need a stored exact comparison of their pair: made before each, not timed)
            grp0, grp4, nine = [], [], []
            for step in range(a.steps + 1):
                res0 = capi.exact_paired_delta_groups_batches(g1, g2, PROBS)
                res4 = capi.exact_paired_delta_groups_batches(g1, g2, PROBS, Z4)
                total = 0.0
                for x in g1:
                    for y in g2:
                        x.compare_exact_paired(y)
                        x.exact_delta_quantiles(y, PROBS)
                        total += x.exact_delta_ms()
                if step:
                    grp0.append(res0.kernel_ms); grp4.append(res4.kernel_ms); nine.append(total)
            for name, ms in (("exact_paired_delta_groups, n_p = 3, n_z = 0", grp0), ("exact_paired_delta_groups, n_p = 3, n_z = 4", grp4),
                             ("nine exact_paired_delta_quantiles launches, n_p = 3", nine)):
                lines.append("%-52s kernel ms min %.3f median %.3f max %.3f (%d runs)"
                             % (name, min(ms), sorted(ms)[len(ms) // 2], max(ms), len(ms)))
            lines.append("comparable events: %d of %d; exact_paired_delta_groups / nine launches = %.3f (n_z = 0), %.3f (n_z = 4)"
                         % (int(res0.was_exact.sum()), a.events, min(grp0) / min(nine), min(grp4) / min(nine)))
        pooled = []
        for step in range(a.steps + 1):
            res = capi.compare_pairs_groups(g1, g2, 0.95, (0.1, 0.2))
            if step:
                pooled.append(res.kernel_ms)
        lines.append("%-52s kernel ms min %.3f median %.3f max %.3f (%d runs)"
                     % ("compare_pairs_groups at %d rows (sampled)" % rows, min(pooled), sorted(pooled)[len(pooled) // 2],
                        max(pooled), len(pooled)))
        del g1, g2
    text = "\n".join(lines + a.note) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
