"""Time the posterior predictive model check on the flagship shapes and print what profiles/model_check.txt
records: per shape the pass's kernel time and the call's wall time, miso_batch_diagnose's kernel time on the same batch for
scale, the sampler's own time, and the share of the pass's binomial draws that fall into the BTRS regime.

    python tools/model_check_bench.py [--events 40000] [--repeat 3]

The BTRS share is an estimate from the class tables at the posterior mean: a draw Binomial(rem, r) takes BTRS when
rem min(r, 1 - r) >= 10 (include/miso_binomial.h), evaluated with rem = N T_c / T_0 and r = w_c / T_c at the event's mean psi."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from miso_amd import capi, workload  # noqa: E402


def build(n_events, n_reads, first_id=0):
    """workload.build_batch's events (two isoforms, simulated reads) in a batch with MISO's default schedule -- 6 chains of
    5000 iterations, 500 burnt, every tenth kept: 2700 rows -- and the model check switched on"""
    b = capi.Batch(36, iters=5000, burn=500, lag=10, chains=6, model_check=True)
    for i in range(n_events):
        gid = first_id + i
        exons, isoforms, expr = workload.event_gene(gid, workload.mixed_k(gid, 2))
        b.add_simulated(capi.Gene(exons, isoforms), expr, workload.event_n_reads(gid, n_reads), workload.GEN_SEED + gid)
    return b


def btrs_share(b, n_events):
    b.summarize()
    draws = btrs = 0
    for i in range(n_events):
        t = b.model_check_table(i)
        if t["status"] != "ok" or t["num_reads"] == 0:
            continue
        psi = b.summary(i)[0]
        w = np.array([m * sum(psi[k] for k in range(len(psi)) if (int(p) >> k) & 1) for p, m in zip(t["pattern"], t["m"])])
        T = np.cumsum(w[::-1])[::-1]
        for c in range(len(w) - 1):
            if T[c] <= 0:
                continue
            rem, r = t["num_reads"] * T[c] / T[0], w[c] / T[c]
            draws += 1
            btrs += rem * min(r, 1 - r) >= 10
    return btrs / max(draws, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=40000)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    capi.set_device(0)
    for name, n_reads in (("1000 reads per event", 1000), ("hg19-like read counts", workload.HG19_LIKE)):
        t0 = time.time()
        b = build(a.events, n_reads)
        t_build = time.time() - t0
        print("%s: batch of %d events built in %.1f s" % (name, a.events, t_build), flush=True)
        b.upload(0)
        b.launch(seed=1, first_event_id=0)
        sample_ms = b.sync()
        kernel, wall = [], []
        for _ in range(a.repeat):
            t0 = time.time()
            b.model_check(seed=1)
            wall.append(1e3 * (time.time() - t0))
            kernel.append(b.model_check_ms())
        b.diagnose()
        fits = b.model_fit_many(range(a.events))
        ok = [f for f in fits if f.ok]
        p = np.array([f.pvalue for f in ok])
        print("%s: %d events x %d rows" % (name, a.events, fits[0].rows + fits[0].bad_rows))
        print("  sampler kernels            %9.2f ms" % sample_ms)
        print("  model check kernel         %9.2f ms  (runs: %s)" % (min(kernel), ", ".join("%.2f" % x for x in kernel)))
        print("  model check call, wall     %9.2f ms  (runs: %s)" % (min(wall), ", ".join("%.1f" % x for x in wall)))
        print("  diagnose kernel, for scale %9.2f ms" % b.pass_ms()[1])
        print("  binomial draws in the BTRS regime (estimate at the posterior mean): %.1f %%" % (100 * btrs_share(b, a.events)))
        print("  events ok %d of %d; fit_pvalue: mean %.3f, share <= 0.01 %.4f, share >= 0.99 %.4f"
              % (len(ok), a.events, p.mean(), (p <= 0.01).mean(), (p >= 0.99).mean()), flush=True)
        del b


if __name__ == "__main__":
    main()
