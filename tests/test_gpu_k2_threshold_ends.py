"""The single-end two-isoform read loop with the threshold's high half at both ends of its range (miso_amd/csrc/kernels_k2.inl
gibbs(), csrc/k2_count.hpp): th = 0 (nothing is below, a half of 0 is on the threshold), th = 0xFFFE (the largest th whose
th + 1 fits a half), th = 0xFFFF (it does not: the lane finishes by the header's rule or counts its reads directly) and
t = 2^32 (closed form).  Events of 1500 - 2500 drawing reads with psi pinned to an end of [0, 1] by a prior of 10^13 to 1 (the
recipe of the skewed events of tests/test_gpu_k2_read_loop.py), so that steps at the ends meet halves on and next to the
threshold; bit for bit against the checker's counter mode on every forced lane layout and in the planner's own launch, with
and without the forced rescan.  Which thresholds and halves occurred is computed from the checker's psi samples and draws
and asserted."""
import os

import numpy as np
import pytest

import miso_amd
from _libs import OrcLib
from test_gpu_k2_read_loop import _drawing_reads, _event, _pred

KW = dict(iters=1500, burn=0, lag=1, chains=2)
SEED, FIRST_ID = 91, 600
# (drawing reads, prior): psi -> 1 (t = 2^32, th = 0xFFFF and 0xFFFE on the way there), an ordinary event in the same
# wavefronts, psi -> 1 less tightly (th = 0xFFFE for most of the run), psi -> 0 (th = 0)
EVENTS = [(1501, [1e13, 1.0]), (250, None), (2499, [1e7, 1.0]), (2003, [1.0, 1e13])]
WIDTHS = (1, 2, 3, 4, 8, 64)
ENV_NAMES = ("MISO_LANES_PER_CHAIN", "MISO_K2_SETTLE_ALL", "MISO_K2_TARGET")


def _steps(cpu):
    """per chain-step (row m * chains + chain: sample m is the psi gibbs(m) draws with, burn = 0 and lag = 1) which end the
    threshold sits at: the test u < t is monotone in u, so t > u exactly where it holds at u"""
    s = cpu.samples.reshape(-1, 2)
    p = lambda u: _pred(float(u), s[:, 0], s[:, 1])
    closed = p(0xFFFFFFFF)
    return {"t = 2^32": closed, "th = 0xFFFF": p(0xFFFEFFFF) & ~closed, "th = 0xFFFE": p(0xFFFDFFFF) & ~p(0xFFFEFFFF),
            "th = 0": ~p(0xFFFF)}


def _high_halves(orc, event_id, chain, m, n_draw):
    """the high half-words of the event's drawing reads at iteration m (include/miso_philox.h: site 2, half h of block
    r / 8 = bits 16 (h & 1) .. of word h / 2)"""
    out = []
    for q in range((n_draw + 7) >> 3):
        w = orc.philox((q, m, 2 | (chain << 8), event_id), (SEED & 0xFFFFFFFF, SEED >> 32))
        out.append(np.stack([w & 0xFFFF, w >> 16], axis=1).ravel())
    return np.concatenate(out)[:n_draw]


def _coverage(orc, cpu, draws):
    """the counts the test asserts, from the checker alone"""
    seen = {k: 0 for k in ("t = 2^32", "th = 0xFFFF", "th = 0xFFFE", "th = 0", "0xFFFF at th = 0xFFFF", "0xFFFE at th = 0xFFFF",
                           "0 at th = 0")}
    for i, c in enumerate(cpu):
        st = _steps(c)
        for k, v in st.items():
            seen[k] += int(v.sum())
        for name, want, keys in (("th = 0xFFFF", (0xFFFF, 0xFFFE), ("0xFFFF at th = 0xFFFF", "0xFFFE at th = 0xFFFF")),
                                 ("th = 0", (0,), ("0 at th = 0",))):
            for row in np.flatnonzero(st[name])[:400]:
                if all(seen[k] >= 3 for k in keys):
                    break
                m, ch = divmod(int(row), KW["chains"])
                hi = _high_halves(orc, FIRST_ID + i, ch, m, draws[i])
                for v, k in zip(want, keys):
                    seen[k] += int(np.any(hi == v))
    return seen


@pytest.fixture(scope="module")
def problem(orc):
    b = miso_amd.Batch(36, counts_trace=True, **KW)
    keep = []
    for i, (n, hy) in enumerate(EVENTS):
        exons, isoforms, g, pos, cig = _event(orc, n, seed=7300 + i)
        b.add_event(miso_amd.Gene(exons, isoforms), pos, cig, hyper=hy)
        keep.append((g, pos, cig, hy))
    draws = [_drawing_reads(b, i) for i in range(len(EVENTS))]
    assert draws == [n for n, _ in EVENTS], draws
    cpu = [orc.miso(g, pos, cig, 36, mode=OrcLib.COUNTER, seed=SEED, event_id=FIRST_ID + i, trace=True, hyper=hy, **KW)
           for i, (g, pos, cig, hy) in enumerate(keep)]
    assert all(c.rc == 0 for c in cpu)
    return b, cpu, draws


def test_the_checker_alone_meets_every_end(orc, problem):
    """(needs no device) at least ten chain-steps at each end, and among the th = 0xFFFF steps three with a half of 0xFFFF
    and three with a half of 0xFFFE; the generator's address restated here is the checker's own"""
    _, cpu, draws = problem
    hi = _high_halves(orc, FIRST_ID, 1, 7, 24)
    assert [int(x) for x in hi] == [orc.split_word(SEED, FIRST_ID, 1, 7, r) >> 16 for r in range(24)]
    seen = _coverage(orc, cpu, draws)
    print(seen)
    for k in ("t = 2^32", "th = 0xFFFF", "th = 0xFFFE", "th = 0"):
        assert seen[k] >= 10, seen
    for k in ("0xFFFF at th = 0xFFFF", "0xFFFE at th = 0xFFFF", "0 at th = 0"):
        assert seen[k] >= 3, seen


def _layouts():
    envs = [dict()] + [dict(MISO_LANES_PER_CHAIN=str(w)) for w in WIDTHS]
    return [dict(e, **s) for e in envs for s in (dict(), dict(MISO_K2_SETTLE_ALL="1"))]


@pytest.mark.gpu
@pytest.mark.parametrize("env", _layouts(), ids=lambda e: ",".join("%s=%s" % kv for kv in sorted(e.items())) or "planner")
def test_threshold_ends_bit_for_bit(problem, env):
    b, cpu, _ = problem
    saved = {k: os.environ.pop(k, None) for k in ENV_NAMES}
    try:
        os.environ.update(env)
        b.run(seed=SEED, first_event_id=FIRST_ID)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    kernels = b.last_kernels()
    assert "sampler_k2" in kernels, kernels
    if "MISO_LANES_PER_CHAIN" not in env:
        assert "sampler_k2_multi<0" in kernels, kernels
    for i in range(len(EVENTS)):
        got = b.result(i, trace=True)
        assert np.array_equal(got.counts_trace, cpu[i].trace["counts_trace"]), (kernels, env, i)
        assert np.array_equal(got.samples, cpu[i].samples), (kernels, env, i)
        assert np.array_equal(got.loglik, cpu[i].loglik), (kernels, env, i)
        assert np.array_equal(got.assignment, cpu[i].assignment), (kernels, env, i)
        assert got.rundata.noAccepted == cpu[i].accepted, (kernels, env, i)
        assert np.array_equal(got.counts_hash, cpu[i].trace["counts_hash"]), (kernels, env, i)
