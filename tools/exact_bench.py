"""The exact-posterior mode against the default sampler on the headline workload (bench.py's BASE_SHAPE: 40 000 single-end
two-isoform events x 1000 reads, 7500 iterations, 2500 of them burn-in, one chain: S = 5000 rows per event), in one
process: the same events once in the default mode and once with exact=True, `--steps` timed launches each after a
warm-up.  Kernel time is the HIP-event time of the launch (miso_batch_sync); the shader clock of every mode's last
launch comes from miso_batch_set_clock_probe.  The exact kernel's two stages are told apart by a third batch of the same
events with ONE row per event: its kernel time is the posterior stage (mode, window, 2049-point table) plus one draw,
and the difference to the full launch is the draw / write stage.

    python tools/exact_bench.py [--events 40000] [--reads 1000] [--iters 7500 --burn 2500 --lag 1 --chains 1]
                                [--steps 5] [--out profiles/exact.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(batch, steps, seed=1):
    """kernel ms of `steps` launches after a warm-up one, then (clock GHz, probe window ms) of one more"""
    batch.launch(seed=seed, first_event_id=0)
    batch.sync()
    ms = []
    for _ in range(steps):
        batch.launch(seed=seed, first_event_id=0)
        ms.append(batch.sync())
    batch.set_clock_probe(True)
    batch.launch(seed=seed, first_event_id=0)
    probe_ms = batch.sync()
    ghz, window = batch.last_clock()
    batch.set_clock_probe(False)
    return ms, (ghz, window, probe_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=40000)
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=7500)
    ap.add_argument("--burn", type=int, default=2500)
    ap.add_argument("--lag", type=int, default=1)
    ap.add_argument("--chains", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact.txt"))
    a = ap.parse_args()
    from miso_amd import capi, workload
    if capi.device_count() < 1:
        print("exact_bench: no HIP device -- nothing is measured without one")
        return 1
    S = a.chains * (a.iters - a.burn) // a.lag
    lines = ["exact_bench: %d events x %d reads, %d iterations (%d burn-in, lag %d), %d chain(s): S = %d rows per event"
             % (a.events, a.reads, a.iters, a.burn, a.lag, a.chains, S)]
    shape = dict(K=2, n_reads=a.reads, lag=a.lag, chains=a.chains)
    rows = {}
    for name, kw in (("default", dict(iters=a.iters, burn=a.burn)),
                     ("exact", dict(iters=a.iters, burn=a.burn, exact=True)),
                     ("exact, one row per event", dict(iters=a.burn + a.lag, burn=a.burn, exact=True))):
        t0 = time.time()
        b = workload.build_batch(0, a.events, **shape, **kw)
        b.upload(0)
        t_build = time.time() - t0
        ms, (ghz, window, probe_ms) = timed(b, a.steps)
        best, med = min(ms), sorted(ms)[len(ms) // 2]
        rows[name] = best
        lines.append("%-26s %-26s kernel ms min %.3f median %.3f max %.3f (%d launches) | %.0f events/s at the minimum | "
                     "shader clock %s | batch built in %.1f s"
                     % (name, b.last_kernels(), best, med, max(ms), len(ms), a.events / (best * 1e-3),
                        "%.3f GHz over a %.3f ms window (that launch: %.3f ms)" % (ghz, window, probe_ms) if ghz > 0
                        else "not measured (the probe's window did not cover a launch of %.3f ms)" % probe_ms, t_build))
        del b
    full, post = rows["exact"], rows["exact, one row per event"]
    out_bytes = a.events * S * (2 + 1) * 8.0
    lines.append("exact kernel: posterior stage (+ one draw) %.3f ms, draw / write stage %.3f ms; it writes %.3f GB of samples "
                 "and log scores: %.2f TB/s over the whole kernel, %.2f TB/s over the draw / write stage"
                 % (post, full - post, out_bytes / 1e9, out_bytes / (full * 1e-3) / 1e12,
                    out_bytes / (max(full - post, 1e-9) * 1e-3) / 1e12))
    lines.append("default / exact kernel time: %.1f x" % (rows["default"] / full))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
