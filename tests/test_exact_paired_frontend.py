"""CPU: the paired-end exact-posterior mode's switches reach the batch -- `miso --run ... --paired-end M SD --exact-paired`,
run_miso's --exact-paired, the settings key `exact_paired` under [sampler], the environment variable the sampler names
(miso_sampler.EXACT_PAIRED_ENV) and params["exact_paired"]
all end in capi.Batch(exact_paired=True), never on a single-end run -- the argument errors are raised, and without a device
the calls fail with ENODEVICE like every other (no CPU path)."""
import os
import sys

import numpy as np
import pytest

import miso_amd
from miso_amd import capi, run_miso, workload
from miso_amd import miso as miso_cli
from miso_amd.settings import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "miso_amd"))


class _Recorded(Exception):
    pass


@pytest.fixture
def batch_kwargs(monkeypatch):
    """capi.Batch replaced by a recorder: the keyword arguments of the batch a front end would have made"""
    seen = []

    def fake(*a, **kw):
        seen.append(kw)
        raise _Recorded()
    monkeypatch.setattr(run_miso.miso.capi, "Batch", fake)     # (miso_sampler's flat import of capi.py)
    return seen


def _prepare(params_extra, paired=True):
    miso_sampler = run_miso.miso          # (the flat module run_miso itself drives)
    if paired:
        params = miso_sampler.get_paired_end_sampler_params(2, 250, 900, 36, overhang_len=1)
    else:
        params = miso_sampler.get_single_end_sampler_params(2, 36, 1)
    params.update(params_extra)
    s = miso_sampler.MISOSampler(params, paired_end=paired, log_dir=None)
    with pytest.raises(_Recorded):
        s.prepare_batch(100, [], num_chains=2, burn_in=10, lag=1)


def test_params_and_environment_reach_the_batch(batch_kwargs, monkeypatch):
    env_name = run_miso.miso.EXACT_PAIRED_ENV
    monkeypatch.delenv(env_name, raising=False)
    monkeypatch.delenv("MISO_EXACT", raising=False)
    _prepare({})
    _prepare({"exact_paired": 1})
    _prepare({"exact_paired": 1}, paired=False)      # never on a single-end run
    monkeypatch.setenv(env_name, "1")
    _prepare({})
    _prepare({"exact_paired": 0})                    # the parameter wins over the environment
    _prepare({}, paired=False)
    assert [kw["exact_paired"] for kw in batch_kwargs] == [False, True, False, True, False, False]
    assert not any(kw["exact"] for kw in batch_kwargs)         # the single-end switch is another one
    monkeypatch.setenv("MISO_EXACT", "1")
    _prepare({"exact": 1, "exact_paired": 1})
    assert (batch_kwargs[-1]["exact"], batch_kwargs[-1]["exact_paired"]) == (False, True)


def test_build_batch_keyword(monkeypatch):
    seen = []
    monkeypatch.setattr(workload.capi, "Batch", lambda *a, **kw: seen.append(kw) or (_ for _ in ()).throw(_Recorded()))
    for kw in ({}, {"exact_paired": True}):
        with pytest.raises(_Recorded):
            workload.build_batch(0, 1, paired=True, **kw)
    assert [kw["exact_paired"] for kw in seen] == [False, True]


def test_flag_and_settings_key_reach_the_workers(tmp_path, monkeypatch):
    calls = []
    monkeypatch.setattr(run_miso, "compute_gene_psi", lambda *a, **kw: calls.append(kw))
    genes, bam = tmp_path / "genes.txt", tmp_path / "reads.bam"
    genes.write_text("g1\t/nowhere/g1.pickle\n")
    bam.write_text("")
    settings = tmp_path / "settings.txt"
    settings.write_text("[sampler]\nburn_in = 10\nlag = 2\nnum_iters = 100\nexact_paired = True\n")
    single = ["--compute-genes-from-file", str(genes), str(bam), str(tmp_path / "out"), "--read-len", "36"]
    base = single + ["--paired-end", "250", "30"]
    try:
        assert run_miso.main(base) == 0
        assert run_miso.main(base + ["--exact-paired"]) == 0
        assert run_miso.main(base + ["--settings-filename", str(settings)]) == 0
        assert Settings.get_exact_paired() is True
        assert run_miso.main(single + ["--settings-filename", str(settings)]) == 0     # the key on a single-end run: nothing
    finally:
        Settings.load(None)
    assert [kw["exact_paired"] for kw in calls] == [False, True, True, False]
    assert not any(kw["exact"] for kw in calls)
    assert Settings.get_exact_paired() is False
    with pytest.raises(SystemExit):        # --exact-paired without --paired-end: an argument error before any work
        run_miso.main(single + ["--exact-paired"])
    assert len(calls) == 4


@pytest.mark.parametrize("text,want", [("True", True), ("1", True), ("true", True), ("yes", True), ("on", True),
                                       ("False", False), ("0", False), ("false", False), ("no", False), ("off", False)])
def test_settings_key_spellings(tmp_path, text, want):
    settings = tmp_path / "settings.txt"
    settings.write_text("[sampler]\nburn_in = 10\nlag = 2\nnum_iters = 100\nexact_paired = %s\n" % text)
    try:
        Settings.load(str(settings))
        assert Settings.get_exact_paired() is want and Settings.get_exact() is False
        settings.write_text("[sampler]\nburn_in = 10\nlag = 2\nnum_iters = 100\nexact_paired = maybe\n")
        Settings.load(str(settings))
        with pytest.raises(ValueError, match="Invalid exact_paired parameter"):
            Settings.get_exact_paired()
    finally:
        Settings.load(None)


def test_compute_gene_psi_hands_the_switch_to_the_sampler(tmp_path, monkeypatch):
    """run_miso.compute_gene_psi(exact_paired=True) -> params["exact_paired"] of the paired-end MISOSampler it makes"""
    made = []

    class Stop(Exception):
        pass

    class FakeSampler(object):
        def __init__(self, params, **kw):
            made.append((dict(params), kw["paired_end"]))
            raise Stop()
    monkeypatch.setattr(run_miso.miso, "MISOSampler", FakeSampler)
    monkeypatch.setattr(run_miso, "collect_gene_events", lambda entries, *a, **kw: ([(None, None, None, None, 0)], {}))
    monkeypatch.setattr(run_miso, "preload_genes", lambda *a, **kw: None)
    for paired_end, flag in (((250.0, 30.0), True), ((250.0, 30.0), False), (None, True)):
        with pytest.raises(Stop):
            run_miso.compute_gene_psi(None, None, "reads.bam", str(tmp_path / "o"), 36, 1, gene_entries=[("g", "i")],
                                      bamfile=object(), paired_end=paired_end, exact_paired=flag, verbose=False)
    assert [("exact_paired" in p, pe) for p, pe in made] == [(True, True), (False, True), (False, False)]
    assert made[0][0]["exact_paired"] == 1 and not any("exact" in p for p, _ in made)


def test_dispatcher_hands_the_flag_on(tmp_path, monkeypatch):
    from miso_amd import index_gff
    gff = tmp_path / "g.gff"
    gff.write_text("##gff-version 3\n"
                   "chr1\tx\tgene\t1000\t1900\t.\t+\t.\tID=g0\n"
                   "chr1\tx\tmRNA\t1000\t1900\t.\t+\t.\tID=g0.A;Parent=g0\n"
                   "chr1\tx\texon\t1000\t1100\t.\t+\t.\tID=g0.A.1;Parent=g0.A\n"
                   "chr1\tx\texon\t1800\t1900\t.\t+\t.\tID=g0.A.2;Parent=g0.A\n"
                   "chr1\tx\tmRNA\t1000\t1900\t.\t+\t.\tID=g0.B;Parent=g0\n"
                   "chr1\tx\texon\t1000\t1100\t.\t+\t.\tID=g0.B.1;Parent=g0.B\n"
                   "chr1\tx\texon\t1400\t1500\t.\t+\t.\tID=g0.B.2;Parent=g0.B\n"
                   "chr1\tx\texon\t1800\t1900\t.\t+\t.\tID=g0.B.3;Parent=g0.B\n")
    idx = str(tmp_path / "indexed")
    index_gff.index_gff(str(gff), idx)
    bam = tmp_path / "reads.bam"
    bam.write_text("")
    monkeypatch.setenv("MISO_DISPATCH", "subprocess")
    cmds = []
    monkeypatch.setattr(miso_cli.GenesDispatcher, "_run_subprocesses",
                        lambda self, jobs, parts, table: cmds.extend(cmd for _, cmd, _ in jobs) or [])
    base = ["--run", idx, str(bam), "--output-dir", str(tmp_path / "out"), "--read-len", "36", "-p", "1"]
    for flag in ([], ["--exact-paired"]):
        assert miso_cli.main(base + ["--paired-end", "250", "30"] + flag) == 0
    assert len(cmds) == 2 and "--exact-paired" not in cmds[0] and "--exact-paired" in cmds[1]
    assert "--exact" not in cmds[1]
    # argument errors, before any work
    with pytest.raises(SystemExit):
        miso_cli.main(base + ["--exact-paired"])
    with pytest.raises(SystemExit):        # comparing two paired exact posteriors stays the error it is
        miso_cli.main(base + ["--paired-end", "250", "30", "--exact-paired", "--exact-compare", "--compare", str(bam)])
    assert len(cmds) == 2


def test_no_cpu_path():
    b = miso_amd.Batch(36, iters=50, burn=10, lag=1, chains=1, paired=True, mean=250.0, var=900.0, exact_paired=True)
    match = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    fraglen = np.array([[250, 0], [0, 240], [260, 200]], np.int32)
    assert b.exact_paired and not b.exact and b.add_problem(match, [1500, 1000], [3, 2], fraglen=fraglen) == 0
    el = capi.C.c_int(-1)
    A = capi._p(np.array([60000.0, 43000.0]))
    assert capi.lib().miso_exact_paired_eligible(2, A, capi._p(np.ones(2)), 0, capi.C.byref(el)) == 0 and el.value == 1
    assert capi.lib().miso_exact_paired_eligible(2, A, capi._p(np.array([0.5, 1.0])), 0, capi.C.byref(el)) == 0 and el.value == 0
    assert capi.lib().miso_exact_paired_eligible(2, A, capi._p(np.ones(2)), 1, capi.C.byref(el)) == 0 and el.value == 0
    assert capi.lib().miso_exact_paired_eligible(3, A, capi._p(np.ones(3)), 0, capi.C.byref(el)) == 0 and el.value == 0
    # the switch's own errors need no device
    with pytest.raises(miso_amd.InternalError, match="Invalid value"):
        miso_amd.Batch(36, exact_paired=True)
    if capi.device_count() > 0:
        return      # (with a device the calls work: tests/test_gpu_exact_paired.py)
    with pytest.raises(miso_amd.InternalError, match="no HIP device"):
        b.run()
    assert b"no HIP device" in capi.lib().miso_last_error()
    with pytest.raises(miso_amd.InternalError, match="no HIP device"):
        capi.selftest_exact_paired([[1, 1, 60000.0, 43000.0, 1, 1]], [[(0.01, 0.002)]], [0.5])
