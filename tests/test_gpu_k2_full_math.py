"""GPU: the two-isoform Metropolis-Hastings step down both routes of its exp / log (miso_amd/csrc/detmath_n.hpp det_exp_r /
det_log_r; kernels_k2.inl k2_exp / k2_log).

MISO_K2_FULL_MATH makes every call take the full routines; without it a wavefront takes the routines without special
cases whenever all its arguments allow.  The same batch must give the same samples, log scores, assignments, accept
counts and count hashes either way -- the checker's, bit for bit.

Only sampler_k2_multi<0, 8> (kernels_k2m_m0w8.hip) has the two routes, and it runs the planner's launches alone: a forced
MISO_LANES_PER_CHAIN goes to sampler_k2 (kernels_k2.hip), which has one route and ignores the hook.  So the widths are driven
the way tests/test_gpu_k2_read_loop.py drives them, by MISO_K2_TARGET, the bound on a wavefront's step: a large bound puts
every chain on one lane, smaller ones give wider chains.  TARGETS are chosen from the planner's cost model (plan.hpp
k2_cost_single: step 1750 / 1170 / 840 / 720 issue slots at 1 / 2 / 3 / >= 4 lanes, 54 per block of eight reads) for events of
50 .. 400 drawing reads; which widths they give is read from the planner itself (miso_plan_lanes, the same routine with the
same bound), asserted to contain 1, 2, 3, 4 and 8 -- without a GPU too -- and tied to the launch by the kernel's name and by
the number of wavefronts the launch reports.  The forced single-width launches run as well: there the hook must change
nothing.

What leaves the fast routines' domain without the hook, and what does not:

* exp: a prior of 10^13 to 1 on isoform 0 makes the acceptance test's exponent huge from the first iteration on: it
  contains (10^13 - 1) (log psi_0' - log psi_0), and every other term of it is bounded by the reads (counts times a change of
  log psi of at most sd |z|, a few hundred in all; the two proposal terms cancel to rounding).  An accepted move whose prior
  term exceeds 1000 therefore called exp on an argument above 700.  That such moves exist is asserted from the checker's
  samples.  (Event SKEWED of the 64-event batch.)
* log: a proposal whose psi_0 rounds to 1 has psi_1 = 0: log 0, and log of psi_0 / (1 - psi_0) = inf.  psi = (1, 0) itself is
  never a sample -- its score is not finite, the proposal is rejected -- so the chain would have to stand just below:
  alpha' > 37.43 = 54 log 2.  No batch gets a chain there.  The proposal's width is the model's (sd = sqrt 0.05) and a chain
  starts at alpha = 0, so only a prior (or as many one-isoform reads, ~10^16) can push it, and a prior strong enough to hold
  psi_1 near 2^-53 (10^16 to 1 and more) brings its own normalising constant into the joint score: lgamma(10^17) = 3.8 10^18
  has an ulp of 512, lgamma(10^20) one of 524288, and the prior's gradient, hyper x (change of psi_1), drops below that
  quantum once psi_1 is about 10^-14 whatever the prior.  From there the score no longer sees psi_0 move, the proposal's
  Jacobian term log(psi_1' / psi_1) pulls the chain back, and it wanders at alpha = 32: over 3000 iterations the smallest
  psi_1 under priors of 10^13, 10^17 and 10^20 to 1 is 4.0 10^-13, 8.4 10^-15 and 8.7 10^-15, 36 ulps of 1 and more
  (test_no_prior_brings_psi_to_the_edge asserts it from the checker, whose arithmetic is the device's).  The other arguments
  of log are never outside its domain either: the sum of the two exponentials is at least 1, and the proposal densities
  are exp(-z^2 / 2) times finite factors.  So in the sampler the route TEST of log never says "full" on any input; the full
  log itself runs in the kernel under the hook, on every width, and the test's choice of the full route for a wavefront with
  one zero, subnormal, negative, infinite or NaN argument is covered by tests/test_gpu_fast_detmath.py alone."""
import os

import numpy as np
import pytest

import miso_amd
from _libs import OrcLib
from test_gpu_k2_read_loop import _drawing_reads, _event
from test_plan import plan

LANES = (1, 2, 3, 4, 8)
TARGETS = (5000.0, 2200.0, 1500.0, 1200.0)
KERNEL = "sampler_k2_multi<0, 8>"
NAMES = ("MISO_LANES_PER_CHAIN", "MISO_K2_FULL_MATH", "MISO_K2_SETTLE_ALL", "MISO_K2_TARGET")
N_EVENTS = 64
N_DRAW = [50 + (350 * i) // (N_EVENTS - 1) for i in range(N_EVENTS)]      # 50 .. 400 drawing reads
KW = dict(iters=200, burn=0, lag=1, chains=2)      # every iteration's psi is a sample
SKEWED = 17                                        # the event with the prior
SKEWED_HYPER = [1e13, 1.0]
EDGE_HYPERS = (1e13, 1e17, 1e20)                   # priors on isoform 0 that a chain follows towards psi = (1, 0)
EDGE_ITERS = 3000


def _widths(draws, chains, target):
    """{lanes per chain: wavefronts} of the planner's runs for the bound `target` (the launch's list: most reads first)"""
    runs, _ = plan(sorted(draws, reverse=True), chains=chains, target=target)
    out = {}
    for r in runs:
        cpw = 64 // r["lanes"]
        out[r["lanes"]] = out.get(r["lanes"], 0) + -(-r["events"] * chains // cpw)
    return out


def test_targets_reach_every_width():
    """no GPU: the bounds give one, two, three, four and eight lanes per chain on the batch's drawing-read counts"""
    seen = set()
    for t in TARGETS:
        seen |= set(_widths(N_DRAW, KW["chains"], t))
    assert set(LANES) <= seen and max(seen) <= 64, sorted(seen)
    assert set(_widths(N_DRAW, KW["chains"], TARGETS[0])) == {1}


def _run_both_routes(b, cpu, draws, seed, first_id):
    """{the planner's own launch, every bound of TARGETS, every forced width} x {routes chosen per wavefront, full routines}:
    all outputs the checker's; returns the widths the two-route kernel ran, from the plans behind its launches"""
    saved = {k: os.environ.pop(k, None) for k in NAMES}
    chains, ran = b.params.noChains, set()
    layouts = [dict()] + [dict(MISO_K2_TARGET=repr(t)) for t in TARGETS] + [dict(MISO_LANES_PER_CHAIN=str(w)) for w in LANES]
    try:
        for env in layouts:
            for full in (False, True):
                for k in NAMES:
                    os.environ.pop(k, None)
                os.environ.update(env)
                if full:
                    os.environ["MISO_K2_FULL_MATH"] = "1"
                b.run(seed=seed, first_event_id=first_id)
                what = (env, full)
                if "MISO_LANES_PER_CHAIN" not in env:      # the kernel with the two routes, and nothing else
                    assert b.last_kernels() == KERNEL, (what, b.last_kernels())
                else:
                    assert KERNEL not in b.last_kernels(), (what, b.last_kernels())
                if "MISO_K2_TARGET" in env:                # the launch has the plan's wavefronts: these widths ran
                    want = _widths(draws, chains, float(env["MISO_K2_TARGET"]))
                    st = b.launch_stats()["kernels"]
                    assert len(st) == 1 and st[0]["name"] == KERNEL, (what, st)
                    assert (st[0]["waves"], st[0]["chains"]) == (sum(want.values()), len(draws) * chains), (what, st, want)
                    ran |= set(want)
                for i in range(len(draws)):
                    got, what = b.result(i), (env, full, i)
                    assert np.array_equal(got.samples, cpu[i].samples), what
                    assert np.array_equal(got.loglik, cpu[i].loglik), what
                    assert np.array_equal(got.assignment, cpu[i].assignment), what
                    assert np.array_equal(got.counts_hash, cpu[i].trace["counts_hash"]), what
                    assert (got.rundata.noAccepted, got.rundata.noRejected) == (cpu[i].accepted, cpu[i].rejected), what
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    assert set(LANES) <= ran, sorted(ran)
    return ran


def _batch(orc, draws, hypers, seed0, kw):
    b = miso_amd.Batch(36, **kw)
    keep = []
    for i, (n, hy) in enumerate(zip(draws, hypers)):
        exons, isoforms, g, pos, cig = _event(orc, n, seed=seed0 + i)
        b.add_event(miso_amd.Gene(exons, isoforms), pos, cig, hyper=hy)
        keep.append((g, pos, cig, hy))
    assert [_drawing_reads(b, i) for i in range(len(draws))] == list(draws)
    return b, keep


@pytest.mark.gpu
def test_both_routes_give_the_checkers_outputs(orc):
    b, keep = _batch(orc, N_DRAW, [SKEWED_HYPER if i == SKEWED else None for i in range(N_EVENTS)], 7100, KW)
    cpu = [orc.miso(g, pos, cig, 36, mode=OrcLib.COUNTER, seed=91, event_id=1100 + i, trace=True, hyper=hy, **KW)
           for i, (g, pos, cig, hy) in enumerate(keep)]
    assert all(c.rc == 0 for c in cpu)
    # the skewed event's accepted moves whose prior term alone puts the test's exponent above 700 (see the module's text)
    lx0 = np.log(cpu[SKEWED].samples.reshape(-1, KW["chains"], 2)[:, :, 0])
    prior_term = (SKEWED_HYPER[0] - 1.0) * np.diff(lx0, axis=0)
    assert (prior_term > 1000.0).sum() > 50, (prior_term > 1000.0).sum()
    for i in range(N_EVENTS):
        if i != SKEWED:
            o = cpu[i].samples
            assert ((o > 1e-6) & (o < 1.0 - 1e-6)).all(), i
    _run_both_routes(b, cpu, N_DRAW, seed=91, first_id=1100)


def test_no_prior_brings_psi_to_the_edge(orc):
    """no GPU: however strong the prior, the chains stop some 10^-14 short of psi_0 = 1 (the module's text says why), so
    no proposal rounds psi_0 to 1 and log's route test never leaves the fast route in the sampler"""
    kw = dict(KW, iters=EDGE_ITERS)
    for n, seed in ((50, 7300), (400, 7301)):
        exons, isoforms, g, pos, cig = _event(orc, n, seed=seed)
        for hy in EDGE_HYPERS:
            c = orc.miso(g, pos, cig, 36, mode=OrcLib.COUNTER, seed=92, event_id=1300, trace=True, hyper=[hy, 1.0], **kw)
            assert c.rc == 0
            x1 = c.samples.reshape(-1, 2)[:, 1]
            # a proposal rounds psi_0 to 1 from 37.43 - sd |z| on: within 2 units of alpha for any z that occurs, a factor
            # e^2 in psi_1 above 2^-54; the chains keep 2^-50 away, sixteen times that
            assert x1.min() > 2.0 ** -50 and x1.min() < 1e-11, (n, hy, x1.min())
