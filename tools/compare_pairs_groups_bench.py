"""The pooled comparison of two replicate groups (capi.compare_pairs_groups) against the parent's only way to
the pairwise counts, on tools/compare_pairs_bench.py's workload as n + n replicates: single-end two-isoform events x 1000
reads, every sample drawn with exact=True (another seed per replicate, the isoforms' expression swapped in group 2), in one
process and per row count S of `--rows`:

    compare_pairs_groups at n_tau = 0 and n_tau = 2     the HIP-event time of the call's launches,
    n * n compare_pairs launches, n_tau = 2             the sum of miso_batch_compare_pairs_ms over every (i, j),

each the minimum of `--steps` after a warm-up; that the pooled counts are the sums of the pairwise ones on these batches;
then the workgroups resident per CU at that shape, from the dynamic LDS the pass asks for (max(N1, N2) * 8 bytes, plus the
kernel's static LDS as the build's kept assembly states it) against a CU's 160 KiB, and the kernel's register and scratch
figures from the same file.

    python tools/compare_pairs_groups_bench.py [--events 8000] [--reads 1000] [--group 3] [--rows 2700 5000] [--burn 2500]
                                               [--steps 5] [--out profiles/compare_pairs_groups.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LDS_PER_CU = 160 * 1024
WORK_BYTES = 256 << 20          # kernels_compare_pairs_groups.hip PAIRS_GROUP_WORK_BYTES
ISA = os.path.join(ROOT, "miso_amd", "csrc", ".isa", "kernels_compare_pairs_groups.s")


def kernel_figures():
    """compare_pairs_groups_kernel's figures as the build kept them (the unit's assembly); None without that file"""
    import re
    if not os.path.isfile(ISA):
        return None
    text = open(ISA).read()
    at = text.find("compare_pairs_groups_kernel", text.find("amdhsa.kernels"))
    start = text.rfind("  - .agpr_count", 0, at)
    block = text[start if start >= 0 else 0:]
    block = block[:block.find("\n  - ", 8)] if block.find("\n  - ", 8) >= 0 else block
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}


def build_groups(events, reads, n, **kw):
    """2 n exact batches over the same genes: group 2 with the isoforms' expression swapped, other reads per replicate"""
    from miso_amd import capi, workload
    bs = [capi.Batch(36, exact=True, **kw) for _ in range(2 * n)]
    for e in range(events):
        exons, isoforms, expr = workload.event_gene(e, 2)
        g = capi.Gene(exons, isoforms)
        for s, b in enumerate(bs):
            b.add_simulated(g, expr if s < n else expr[::-1].copy(), workload.event_n_reads(e, reads),
                            workload.GEN_SEED + e + s * events)
    return bs[:n], bs[n:]


def measure(a, S, fig):
    from miso_amd import capi
    n = a.group
    lines = ["S = %d rows per event and sample: %d + %d samples of %d events x %d reads, N1 = N2 = %d pooled draws, %d columns of "
             "%d differences" % (S, n, n, a.events, a.reads, n * S, 2 * a.events, (n * S) ** 2)]
    t0 = time.time()
    g1, g2 = build_groups(a.events, a.reads, n, iters=a.burn + S, burn=a.burn, lag=1, chains=1)
    for s, b in enumerate(g1 + g2):
        b.upload(0)
        b.launch(seed=1 + s, first_event_id=0)
        b.sync()
    t_build = time.time() - t0
    noiso = [2] * a.events

    def timed(call):
        out = []
        for step in range(a.steps + 1):
            ms = call()
            if step:
                out.append(ms)
        return out
    last = {}

    def pooled(taus):
        last["g"] = capi.compare_pairs_groups(g1, g2, 0.95, taus, noiso=noiso)
        return last["g"].kernel_ms

    def pairwise(taus):
        ms = 0.0
        for x in g1:
            for y in g2:
                x.compare_pairs(y, 0.95, taus)
                ms += x.compare_pairs_ms()
        return ms
    rows = [("compare_pairs_groups, n_tau = 0", timed(lambda: pooled(()))),
            ("compare_pairs_groups, n_tau = 2", timed(lambda: pooled((0.1, 0.2)))),
            ("%d compare_pairs launches, n_tau = 2" % (n * n), timed(lambda: pairwise((0.1, 0.2))))]
    for name, ms in rows:
        lines.append("%-38s kernel ms min %.3f median %.3f max %.3f (%d runs) | %.0f events/s at the minimum"
                     % (name, min(ms), sorted(ms)[len(ms) // 2], max(ms), len(ms), a.events / (min(ms) * 1e-3)))
    p0, p2, pw = (min(ms) for _, ms in rows)
    lines.append("pooled / pairwise launches: %.2f x at n_tau = 2; two thresholds cost %.3f ms" % (p2 / pw, p2 - p0))
    # the pooled counts are the sums of the pairwise ones (event 0 and the last event)
    g = last["g"]
    for e in (0, a.events - 1):
        gt = lt = 0
        ge = 0
        for x in g1:
            for y in g2:
                x.compare_pairs(y, 0.95, (0.1, 0.2))
                r = x.pair_comparison(e)
                gt, lt, ge = gt + r[3], lt + r[4], ge + r[5]
        r = g.pair_comparison(e)
        same = (r[3] == gt).all() and (r[4] == lt).all() and (r[5] == ge).all()
        lines.append("event %d: pooled counts %s the sums of the %d pairwise passes' counts" % (e, "ARE" if same else "ARE NOT", n * n))
    static_lds = fig["group_segment_fixed_size"] if fig else 0
    dyn = n * S * 8
    lds = dyn + static_lds
    per_launch = max(1, WORK_BYTES // (2 * n * S * 8))
    lines.append("LDS per workgroup %d bytes (%d dynamic + %s static): %d workgroup(s) resident per CU of %d bytes -- the LDS "
                 "bounds them" % (lds, dyn, static_lds if fig else "unknown (no kept assembly)", LDS_PER_CU // lds, LDS_PER_CU))
    lines.append("workspace: %d bytes a column, %d events a launch, %d launch(es)"
                 % (n * S * 8, min(per_launch, a.events), -(-a.events // per_launch)))
    med, lo, hi, gt, lt, ge, fin, M = g.pair_comparison(0)
    lines.append("event 0: median %.6f, interval [%.6f, %.6f], P(> 0) %.6f, P(|d| >= 0.1) %.6f, P(|d| >= 0.2) %.6f; "
                 "batches built and sampled in %.1f s"
                 % (med[0], lo[0], hi[0], gt[0] / M, ge[0, 0] / M, ge[0, 1] / M, t_build))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=8000)
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--group", type=int, default=3)
    ap.add_argument("--rows", type=int, nargs="+", default=[2700, 5000])
    ap.add_argument("--burn", type=int, default=2500)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare_pairs_groups.txt"))
    a = ap.parse_args()
    from miso_amd import capi
    if capi.device_count() < 1:
        print("compare_pairs_groups_bench: no HIP device -- nothing is measured without one")
        return 1
    fig = kernel_figures()
    lines = ["compare_pairs_groups_bench: HIP-event kernel times, the minimum of %d after a warm-up, one process" % a.steps]
    if fig:
        lines.append("compare_pairs_groups_kernel as built: %d VGPRs, %d SGPRs, %d bytes of scratch, %d + %d spilled registers"
                     % (fig["vgpr_count"], fig["sgpr_count"], fig["private_segment_fixed_size"], fig["vgpr_spill_count"],
                        fig["sgpr_spill_count"]))
    for S in a.rows:
        lines.append("")
        lines += measure(a, S, fig)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
