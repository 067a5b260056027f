#!/usr/bin/env python3
"""Share of the two-isoform step's exp / log calls that take the FULL route (csrc/detmath_n.hpp det_exp_r / det_log_r) on a
benchmark batch -- needs the diagnostic build of the headline's unit:

    tools/build_variant.sh routecount "-DMISO_K2_ROUTE_COUNT" kernels_k2m_m0w8
    MISO_AMD_LIB=tools/_build/libmiso_routecount.so python tools/k2_route_share.py [--reads-dist hg19] [--events N]

In that build ChainStats::hw_id of a chain carries its WAVEFRONT's counters instead of the hardware id: full-route calls in
the high half-word (saturating at 65535), calls / 256 in the low one.  Chains that share a wavefront report the same pair,
and the sums below run over every chain's copy: numerator and denominator both count a wavefront once per chain it holds, so
the ratio is the share of wavefront-calls weighted by chains per wavefront -- "a wavefront-call took the full route" is
charged to every chain of the wavefront."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=40000)
    ap.add_argument("--reads-dist", default="fixed", choices=("fixed", "hg19"))
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    sh = dict(bench.BASE_SHAPE)
    if a.reads_dist == "hg19":
        sh["reads"] = "hg19"
    batch = bench.build(0, a.events, sh)
    batch.upload(0)
    batch.launch(seed=a.seed, first_event_id=0)
    batch.sync()
    batch.download()
    print("kernels:", batch.last_kernels())
    full = calls = 0
    chains_full = chains = saturated = 0
    for i in range(a.events):
        w = batch.placement(i)
        f, c = (w >> 16).astype(np.int64), (w & 0xFFFF).astype(np.int64) * 256
        full += int(f.sum()); calls += int(c.sum())
        chains += len(w); chains_full += int((f > 0).sum()); saturated += int((f == 0xFFFF).sum())
    print("chains %d, of which in a wavefront with any full-route call: %d (%d saturated)" % (chains, chains_full, saturated))
    print("wavefront-calls (per chain, counters in units of 256 calls): %d, full route: %d, share %.4f %%"
          % (calls, full, 100.0 * full / max(calls, 1)))


if __name__ == "__main__":
    main()
