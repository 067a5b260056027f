"""Times the chain-diagnostics passes (miso_batch_diagnose; miso_batch_diagnose_rank) against the
summary pass on the same resident batch.

    python tools/diagnostics_bench.py [--events 40000] [--reads 200] [--out profiles/diagnostics_rank.txt]

Two pools, both sampled here so the columns are the sampler's own:
  headline  40 000 two-isoform events, one chain, 7500 iterations, burn-in 2500, lag 2: S = 2500
  defaults  the same events at MISO's defaults: six chains, 5000 iterations, burn-in 500, lag 10: S = 2700
Per pool: kernel time (HIP events, capi.Batch.pass_ms and rank_pass_ms) of summarize, of diagnose and of diagnose_rank, best
of `--repeat` runs, and the rank pass over the classic one; the mean lag at which Geyer's sequence was cut and the share of
columns cut at each lag; the sample bytes of the pool divided by the time; the medians of the rank pass's outputs.
The reads per event only set how long the sampling before the measurement takes.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from miso_amd import capi, workload  # noqa: E402

POOLS = [("headline", dict(chains=1, iters=7500, burn=2500, lag=2)),
         ("defaults", dict(chains=6, iters=5000, burn=500, lag=10))]


def measure(name, kw, n_events, reads, repeat, device):
    b = workload.build_batch(0, n_events, K=2, n_reads=reads, **kw)
    b.upload(device)
    b.set_clock_probe(True)         # the shader clock of the sampling launch, just before the passes
    b.launch(seed=1, first_event_id=0)
    sample_ms = b.sync()
    ghz = b.last_clock()[0]
    S = kw["chains"] * (kw["iters"] - kw["burn"]) // kw["lag"]
    nbytes = 8.0 * 2 * S * n_events
    best = [float("inf"), float("inf"), float("inf")]
    for _ in range(repeat):
        b.summarize(0.95)
        b.diagnose()
        b.diagnose_rank(None, 0.95)
        ms = b.pass_ms() + (b.rank_pass_ms(),)
        best = [min(a, c) for a, c in zip(best, ms)]
    d = b.diagnostics_many(range(n_events), [2] * n_events)
    lag = np.array([r[3][0] for r in d])
    rhat = np.array([r[0][0] for r in d])
    ess = np.array([r[1][0] for r in d])
    ok = np.isfinite(rhat)
    rk = b.rank_diagnostics_many(range(n_events), [2] * n_events)
    rank_rhat = np.array([max(r[0][0], r[1][0]) for r in rk])
    ess_bulk = np.array([r[2][0] for r in rk])
    ess_tail = np.array([min(r[3][0], r[4][0]) for r in rk])
    distinct = np.array([r[5][0] for r in rk])
    rok = np.isfinite(rank_rhat) & np.isfinite(ess_tail)
    cuts = ", ".join("lag %d: %.1f %%" % (v, 100.0 * c / ok.sum()) for v, c in zip(*np.unique(lag[ok], return_counts=True)) if c / ok.sum() >= 0.01)
    lines = ["%s: %d events, K = 2, %d chains, S = %d (%d reads per event; sampling %.1f ms, shader clock %s)"
             % (name, n_events, kw["chains"], S, reads, sample_ms, "%.2f GHz" % ghz if ghz > 0 else "not measured"),
             "  summarize %.3f ms (%.0f GB/s of samples)   diagnose %.3f ms (%.0f GB/s)   ratio %.2f"
             % (best[0], nbytes / best[0] / 1e6, best[1], nbytes / best[1] / 1e6, best[1] / best[0]),
             "  columns diagnosed %d, degenerate %d; mean lag %.2f, max %d (%s)" % (ok.sum(), (~ok).sum(), lag[ok].mean(), lag[ok].max(), cuts),
             "  rhat median %.4f, 99th percentile %.4f; ess median %.0f, 1st percentile %.0f of %d"
             % (np.median(rhat[ok]), np.percentile(rhat[ok], 99), np.median(ess[ok]), np.percentile(ess[ok], 1), 2 * kw["chains"] * ((S // kw["chains"]) // 2)),
             "  diagnose_rank %.3f ms (%.0f GB/s)   ratio to diagnose %.2f" % (best[2], nbytes / best[2] / 1e6, best[2] / best[1]),
             "  rank columns %d; rank rhat median %.4f, 99th percentile %.4f; bulk ess median %.0f; tail ess median %.0f, 1st "
             "percentile %.0f; distinct draws median %d"
             % (rok.sum(), np.median(rank_rhat[rok]), np.percentile(rank_rhat[rok], 99), np.median(ess_bulk[rok]),
                np.median(ess_tail[rok]), np.percentile(ess_tail[rok], 1), np.median(distinct[rok]))]
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--events", type=int, default=40000)
    ap.add_argument("--reads", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args(argv)
    if capi.device_count() < 1:
        raise SystemExit("diagnostics_bench: no HIP device")
    lines = ["diagnostics_bench %s: best of %d runs per pass, kernel time from HIP events" % (time.strftime("%Y-%m-%d"), a.repeat)]
    for name, kw in POOLS:
        lines += measure(name, kw, a.events, a.reads, a.repeat, a.device)
        print("\n".join(lines[-6:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
