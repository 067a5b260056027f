"""The all-pairs comparison against its yardstick on tools/exact_compare_bench.py's workload as TWO samples (bench.py's
BASE_SHAPE: 40 000 single-end two-isoform events x 1000 reads, 7500 iterations, 2500 of them burn-in, one chain: S = 5000
rows per event and sample, both samples drawn with exact=True), in one process:

    compare_pairs at n_tau = 0 and n_tau = 2    the HIP-event time of the kernel (miso_batch_compare_pairs_ms),
    compare_kernel                               the index-paired (KDE) comparison miso_batch_compare of the same two batches,

each the minimum of `--steps` after a warm-up; then the workgroups of compare_pairs resident per CU at that shape, from the
dynamic LDS the pass asks for ((S1 + S2) * 8 bytes, plus the kernel's static LDS as the build's kept assembly states it)
against a CU's 160 KiB, and the kernel's register and scratch figures from the same file.

    python tools/compare_pairs_bench.py [--events 40000] [--reads 1000] [--iters 7500 --burn 2500 --lag 1 --chains 1]
                                        [--steps 5] [--out profiles/compare_pairs.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LDS_PER_CU = 160 * 1024
ISA = os.path.join(ROOT, "miso_amd", "csrc", ".isa", "kernels_compare_pairs.s")


def kernel_figures():
    """compare_pairs_kernel's figures as the build kept them beside the library (the unit's assembly, miso_amd/csrc/Makefile):
    {vgpr_count, sgpr_count, private_segment_fixed_size, group_segment_fixed_size, ...}; None without that file"""
    import re
    if not os.path.isfile(ISA):
        return None
    text = open(ISA).read()
    at = text.find("compare_pairs_kernel", text.find("amdhsa.kernels"))
    block = text[text.rfind("  - .agpr_count", 0, at) if text.rfind("  - .agpr_count", 0, at) >= 0 else 0:]
    block = block[:block.find("\n  - ", 8)] if block.find("\n  - ", 8) >= 0 else block
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=40000)
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=7500)
    ap.add_argument("--burn", type=int, default=2500)
    ap.add_argument("--lag", type=int, default=1)
    ap.add_argument("--chains", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compare_pairs.txt"))
    a = ap.parse_args()
    from exact_compare_bench import build_pair
    from miso_amd import capi
    if capi.device_count() < 1:
        print("compare_pairs_bench: no HIP device -- nothing is measured without one")
        return 1
    S = a.chains * (a.iters - a.burn) // a.lag
    lines = ["compare_pairs_bench: two samples of %d events x %d reads, %d iterations (%d burn-in, lag %d), %d chain(s): "
             "S = %d rows per event and sample, %d column pairs of %d differences"
             % (a.events, a.reads, a.iters, a.burn, a.lag, a.chains, S, 2 * a.events, S * S)]
    t0 = time.time()
    b1, b2 = build_pair(a.events, a.reads, iters=a.iters, burn=a.burn, lag=a.lag, chains=a.chains)
    for s, b in enumerate((b1, b2)):
        b.upload(0)
        b.launch(seed=1 + s, first_event_id=0)
        b.sync()
    t_build = time.time() - t0

    def timed(call, pick):
        out = []
        for step in range(a.steps + 1):
            call()
            if step:
                out.append(pick())
        return out
    rows = [("compare_pairs, n_tau = 0", timed(lambda: b1.compare_pairs(b2, 0.95, ()), b1.compare_pairs_ms)),
            ("compare_pairs, n_tau = 2", timed(lambda: b1.compare_pairs(b2, 0.95, (0.1, 0.2)), b1.compare_pairs_ms)),
            ("compare_kernel (KDE, smoothing 0.3)", timed(lambda: b1.compare(b2, 0.3), lambda: b1.compare_ms()[0]))]
    for name, ms in rows:
        lines.append("%-38s kernel ms min %.3f median %.3f max %.3f (%d runs) | %.0f events/s at the minimum"
                     % (name, min(ms), sorted(ms)[len(ms) // 2], max(ms), len(ms), a.events / (min(ms) * 1e-3)))
    p0, p2, kde = (min(ms) for _, ms in rows)
    fig = kernel_figures()
    static_lds = fig["group_segment_fixed_size"] if fig else 0
    lds = 2 * S * 8 + static_lds
    lines.append("compare_pairs / compare_kernel: %.1f x at n_tau = 0, %.1f x at n_tau = 2; two thresholds cost %.3f ms"
                 % (p0 / kde, p2 / kde, p2 - p0))
    lines.append("LDS per workgroup %d bytes (%d dynamic + %s static): %d workgroup(s) resident per CU of %d bytes"
                 % (lds, 2 * S * 8, static_lds if fig else "unknown (no kept assembly)", LDS_PER_CU // lds, LDS_PER_CU))
    if fig:
        lines.append("compare_pairs_kernel as built: %d VGPRs, %d SGPRs, %d bytes of scratch, %d + %d spilled registers"
                     % (fig["vgpr_count"], fig["sgpr_count"], fig["private_segment_fixed_size"], fig["vgpr_spill_count"],
                        fig["sgpr_spill_count"]))
    med, lo, hi, gt, lt, ge, fin, M = b1.pair_comparison(0)
    lines.append("event 0: median %.6f, interval [%.6f, %.6f], P(> 0) %.6f, P(|d| >= 0.1) %.6f, P(|d| >= 0.2) %.6f; "
                 "batches built and sampled in %.1f s"
                 % (med[0], lo[0], hi[0], gt[0] / M, ge[0, 0] / M, ge[0, 1] / M, t_build))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
