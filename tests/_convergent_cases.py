"""Batches for the tests of stop = CONVERGENT_MEAN (tests/test_convergent_cases.py on the checker alone,
tests/test_gpu_convergent.py and tests/test_gpu_convergent_layouts.py against the device).

A case is a batch of events with a schedule; its reference is the CPU checker's run of every event alone, computed
once per process and shared by every test that uses the case.  Plain Python, no fixtures: the tests pass the session's
checker in.  Events are made the way tests/test_gpu_heavy_tail.py makes its own: _problems.se_gene, the checker's
restatement of the reference simulators, fixed seeds.

Rounds.  The reference's schedule under the rule is (N, B) -> (3 N - 2 B, N) (miso.c:921-924) while N < maxIterations
and the chains have not converged.  The checker's rundata keeps the FIRST round's noIterations, so the rounds an event
took are recovered from its accept counts (rounds_of): every chain accepts or rejects once per iteration, the
single-end loop restarts both counts every round (miso.c:847) and the paired-end loop never does (miso_paired.c:345)."""
import numpy as np

from _libs import OrcLib
from _problems import expr_for, flat, se_gene

MEAN, VAR = 250.0, 900.0


class Event:
    def __init__(self, K, n, exons, isoforms, g, pos, cig, mode):
        self.K, self.n, self.exons, self.isoforms, self.g, self.pos, self.cig, self.mode = K, n, exons, isoforms, g, pos, cig, mode


class Case:
    def __init__(self, name, paired, kw, seed, first_id, events, collapsed=False):
        self.name, self.paired, self.kw, self.seed, self.first_id, self.events = name, paired, dict(kw), seed, first_id, events
        self.collapsed = collapsed
        self._cpu = None

    def reference(self, orc):
        """the checker's run of every event alone, once (read-only afterwards)"""
        if self._cpu is None:
            self._cpu = [run_checker(orc, self, i) for i in range(len(self.events))]
        return self._cpu

    def rounds(self, orc):
        return [rounds_of(self, r) for r in self.reference(orc)]


def run_checker(orc, case, i, **override):
    e = case.events[i]
    kw = dict(case.kw, **override)
    if case.paired:
        r = orc.miso_paired(e.g, e.pos, e.cig, 36, MEAN, VAR, mode=e.mode, seed=case.seed, event_id=case.first_id + i, **kw)
    else:
        r = orc.miso(e.g, e.pos, e.cig, 36, mode=e.mode, seed=case.seed, event_id=case.first_id + i, **kw)
    assert r.rc == 0, (case.name, i, r.rc)
    return r


def schedule(kw, rounds):
    """[(N, B)] of the first `rounds` rounds of the batch's schedule (miso.c:921-924)"""
    N, B, out = kw["iters"], kw["burn"], []
    for _ in range(rounds):
        out.append((N, B))
        N, B = 3 * N - 2 * B, N
    return out


def rounds_of(case, cpu, limit=64):
    """The rounds the checker ran for an event, from its accept counts: (accepted + rejected) / chains is the last
    round's N for a single-end event and the sum of all rounds' N for a paired-end one."""
    total = cpu.accepted + cpu.rejected
    C = case.kw["chains"]
    assert total % C == 0, (case.name, total, C)
    per_chain, run = total // C, 0
    for r, (N, B) in enumerate(schedule(case.kw, limit), 1):
        run += N
        if per_chain == (run if case.paired else N):
            return r
        if N == B and not case.paired:       # burn = iters: the schedule does not move, one round (no kept samples)
            break
    raise AssertionError("%s: %d iterations per chain fit no round of %r" % (case.name, per_chain, case.kw))


def _event(orc, K, n, paired, sim_seed, exlen, gap, expr=None, mode=OrcLib.COUNTER):
    exons, isoforms = se_gene(K, exlen=exlen, gap=gap)
    g = orc.gene(flat(exons), isoforms)
    orc.rng_seed(sim_seed)
    expr = expr_for(K) if expr is None else np.asarray(expr, np.float64) / np.sum(expr)
    if paired:
        rc, _, pos, cig = orc.simulate_paired_reads(g, expr, max(n, 1), 36, MEAN, VAR)
        pos, cig = pos[:2 * n], cig[:2 * n]
    else:
        rc, _, pos, cig = orc.simulate_reads(g, expr, max(n, 1), 36)
        pos, cig = pos[:n], cig[:n]
    assert rc == 0
    return Event(K, n, exons, isoforms, g, pos, cig, mode)


# ---- depth -----------------------------------------------------------------------------------------------------------------
DEEP_SCHEDULES = {"10_9": dict(iters=10, burn=9, lag=1, chains=2), "8_6": dict(iters=8, burn=6, lag=1, chains=2)}
DEEP_READS = [0, 1, 20, 60, 300]
DEEP_NAMES = ["deep_%s_%s" % (end, s) for end in ("se", "pe") for s in DEEP_SCHEDULES]


def _deep(orc, name):
    _, end, sched = name.split("_", 2)
    paired = end == "pe"
    evs = []
    for K in (2, 3, 5):
        for j, n in enumerate(DEEP_READS):
            evs.append(_event(orc, K, n, paired, 8000 + 10 * K + j, 500 if paired else 120, 300 if paired else 100))
    kw = dict(DEEP_SCHEDULES[sched], stop=1, max_iters=10 ** 7)
    return Case(name, paired, kw, seed=11, first_id=2000, events=evs)


# ---- a lag that does not divide the kept window ----------------------------------------------------------------------------
LAG_NAMES = ["lag3", "lag7"]


def _lag(orc, name):
    lag = int(name[3:])
    evs = []
    for j in range(10):
        K = 2 + j % 5
        n = [0, 800, 30, 200, 7, 450, 90, 3, 600, 120][j]
        evs.append(_event(orc, K, n, False, 8200 + j, 120, 100))
    kw = dict(iters=24, burn=8, lag=lag, chains=3, stop=1, max_iters=1500)
    return Case(name, False, kw, seed=19, first_id=3000, events=evs)


def unfilled_rows(kw, r):
    """rows of round r's sample matrix (1-based) that no iteration fills: noSamples = C (N - B) / lag rows are allocated
    (miso.c:728), every chain fills (N - B) / lag of them, both divisions rounding down"""
    N, B = schedule(kw, r)[-1]
    return kw["chains"] * (N - B) // kw["lag"] - kw["chains"] * ((N - B) // kw["lag"])


# ---- schedule edges --------------------------------------------------------------------------------------------------------
EDGE_EVENTS = ["se_k2", "se_k3", "pe_k2"]
EDGE_SCHEDULES = {
    "burn0": dict(iters=12, burn=0, lag=1, chains=3, max_iters=2000),
    "burn_is_iters": dict(iters=12, burn=12, lag=1, chains=3, max_iters=2000),
    "max_is_second_N": dict(iters=12, burn=4, lag=1, chains=3, max_iters=3 * 12 - 2 * 4),
    "max_is_second_N_plus_1": dict(iters=12, burn=4, lag=1, chains=3, max_iters=3 * 12 - 2 * 4 + 1),
    "chains2": dict(iters=12, burn=4, lag=1, chains=2, max_iters=2000),
    "chains6": dict(iters=12, burn=4, lag=1, chains=6, max_iters=2000),
}
EDGE_NAMES = ["edge_%s_%s" % (e, s) for e in EDGE_EVENTS for s in EDGE_SCHEDULES]


def _edge(orc, name):
    _, end, k, sched = name.split("_", 3)
    paired, K = end == "pe", int(k[1:])
    ev = _event(orc, K, 40, paired, 8300 + K + 10 * paired, 500 if paired else 120, 300 if paired else 100)
    return Case(name, paired, dict(EDGE_SCHEDULES[sched], stop=1), seed=23, first_id=3500, events=[ev])


# ---- breadth: a batch per kernel family ------------------------------------------------------------------------------------
# (32, 8) -> (80, 32) -> (176, 80) -> (368, 176): max_iters = 368 lets the checker run four rounds at the most, which bounds
# its time on the events of thousands of reads
SHORT = dict(iters=32, burn=8, lag=2, stop=1, max_iters=368)
K2_SIZES = [20, 20000, 300, 5, 0, 2500, 40, 1000, 150, 7000, 64, 3, 511]
FLAT_SIZES = [20, 6000, 300, 5, 0, 2500, 40, 1000, 150, 64, 3, 511]
GRP_SIZES = [30, 5000, 200, 5, 0, 1800, 60, 700, 120, 90, 35, 400]
COLLAPSED_SIZES = [700, 20000, 20, 0, 3, 150, 45, 1000, 64, 65, 31, 1, 333]
LAYOUT_NAMES = (["k2_se", "k2_pe"] + ["flat_%d" % K for K in (3, 5, 10, 18)] + ["grp_pe_%d" % K for K in (3, 5, 10)] +
                ["grp_all", "wave_se", "wave_pe", "big_se", "collapsed_k2", "collapsed_mix"])


def _small(orc, K, paired):
    """Three genes of three isoforms beside a batch of K > 3: chains of five and more isoforms do not converge in a schedule
    this short, so these are the events that leave the batch between its rounds"""
    if K <= 3:
        return []
    return [_event(orc, 3, n, paired, 5100 + j, 500 if paired else 130, 300 if paired else 100) for j, n in enumerate([150, 20, 600])]


def _layout(orc, name):
    if name in ("k2_se", "k2_pe"):       # tests/test_gpu_heavy_tail.py _events
        paired = name == "k2_pe"
        evs = []
        for j, n in enumerate(K2_SIZES):
            evs.append(_event(orc, 2, n // 2 if paired else n, paired, 4000 + j, 500 if paired else 90 + 7 * j, 300 if paired else 100,
                              expr=[0.2 + 0.05 * (j % 12), 1.0]))
        return Case(name, paired, dict(SHORT, chains=2 if paired else 3), seed=11, first_id=700, events=evs)
    if name.startswith("flat_"):
        K = int(name[5:])
        evs = [_event(orc, K, n, False, 5000 + j, 90 + 7 * j, 100) for j, n in enumerate(FLAT_SIZES)] + _small(orc, K, False)
        return Case(name, False, dict(SHORT, chains=2), seed=13, first_id=900, events=evs)
    if name.startswith("grp_pe_"):
        K = int(name[7:])
        evs = [_event(orc, K, n, True, 7000 + j, 500 + 11 * j, 300) for j, n in enumerate(GRP_SIZES)] + _small(orc, K, True)
        return Case(name, True, dict(SHORT, chains=2), seed=17, first_id=300, events=evs)
    if name == "grp_all":                # two isoform-count classes, like-sized genes
        counts = [3, 10, 4, 12, 3, 9, 4, 11, 3, 10]
        sizes = [300, 260, 200, 350, 220, 180, 0, 260, 400, 320]
        evs = [_event(orc, K, n, True, 7100 + j, 500 + 11 * j, 300) for j, (K, n) in enumerate(zip(counts, sizes))]
        return Case(name, True, dict(SHORT, chains=2), seed=23, first_id=900, events=evs)
    if name in ("wave_se", "wave_pe", "big_se"):
        paired, K = name == "wave_pe", 70 if name == "big_se" else 40
        evs = []
        for j, (k, n) in enumerate([(K, 400), (5, 300), (K, 90), (2, 200)]):
            evs.append(_event(orc, k, n, paired, 700 + j, 420 if paired else 60, 250 if paired else 50))
        return Case(name, paired, dict(SHORT, chains=2), seed=42, first_id=40, events=evs)
    if name == "collapsed_k2":           # tests/test_gpu_collapsed.py _events
        evs = []
        for j, n in enumerate(COLLAPSED_SIZES):
            evs.append(_event(orc, 2, n, False, 4000 + j, 300 + 17 * j, 100, expr=None if j % 3 else [0.03, 0.97], mode=OrcLib.COLLAPSED))
        return Case(name, False, dict(SHORT, chains=3), seed=10, first_id=1200, events=evs, collapsed=True)
    if name == "collapsed_mix":          # level 2: sampler_lane_k for 3 and 5 isoforms, the gene of 40 per read (sampler_wave)
        evs = []
        for j, (K, n) in enumerate([(3, 400), (40, 300), (5, 900), (3, 0), (5, 60), (3, 1500), (5, 12), (3, 150), (3, 20), (3, 1), (4, 64)]):
            evs.append(_event(orc, K, n, False, 8100 + j, 220 + 7 * j, 100, mode=OrcLib.COUNTER if K > 32 else OrcLib.COLLAPSED))
        return Case(name, False, dict(SHORT, chains=2), seed=1, first_id=300, events=evs, collapsed=2)
    raise KeyError(name)


def ambiguous_reads(cpu):
    """reads of a checker result that more than one isoform explains (the ones a Gibbs step draws)"""
    return int(((cpu.match != 0).sum(1) > 1).sum())


_cases = {}


def case(orc, name):
    """the named batch, built once per process"""
    if name not in _cases:
        make = _deep if name.startswith("deep_") else _lag if name.startswith("lag") else _edge if name.startswith("edge_") else _layout
        _cases[name] = make(orc, name)
    return _cases[name]


def run_device(case, device_match=False):
    """the batch on the GPU (the environment's layout switches are read during run(): set them around this call)"""
    import miso_amd
    b = miso_amd.Batch(36, paired=case.paired, mean=MEAN if case.paired else 0.0, var=VAR if case.paired else 0.0,
                       device_match=device_match, collapsed=case.collapsed, **case.kw)
    for e in case.events:
        b.add_event(miso_amd.Gene(e.exons, e.isoforms), e.pos, e.cig)
    b.upload(0)
    b.launch(seed=case.seed, first_event_id=case.first_id)
    b.first_kernels = b.last_kernels()      # sync() appends the later rounds' kernels behind a comma
    b.sync()
    b.download()
    return b


def later_kernels(b):
    """the kernels of the rounds after the first ('' when there was none)"""
    names = b.last_kernels()
    assert names.startswith(b.first_kernels), (names, b.first_kernels)
    return names[len(b.first_kernels) + 1:]
