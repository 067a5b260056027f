"""CPU: the exact-posterior mode's switches reach the batch -- `miso --run ... --exact`, the settings key `exact` under
[sampler], MISO_EXACT=1 and params["exact"] all end in capi.Batch(exact=True) -- and without a device the call fails
with ENODEVICE like every other (no CPU path)."""
import os
import sys

import numpy as np
import pytest

import miso_amd
from miso_amd import capi, run_miso
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


def _prepare(params_extra, paired=False):
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
    monkeypatch.delenv("MISO_EXACT", raising=False)
    _prepare({})
    _prepare({"exact": 1})
    monkeypatch.setenv("MISO_EXACT", "1")
    _prepare({})
    _prepare({"exact": 0})                 # the parameter wins over the environment
    _prepare({}, paired=True)              # single-end only: a paired-end run never asks for it
    assert [kw["exact"] for kw in batch_kwargs] == [False, True, True, False, False]


def test_flag_and_settings_key_reach_the_workers(tmp_path, monkeypatch):
    calls = []
    monkeypatch.setattr(run_miso, "compute_gene_psi", lambda *a, **kw: calls.append(kw))
    genes, bam = tmp_path / "genes.txt", tmp_path / "reads.bam"
    genes.write_text("g1\t/nowhere/g1.pickle\n")
    bam.write_text("")
    settings = tmp_path / "settings.txt"
    settings.write_text("[sampler]\nburn_in = 10\nlag = 2\nnum_iters = 100\nexact = True\n")
    base = ["--compute-genes-from-file", str(genes), str(bam), str(tmp_path / "out"), "--read-len", "36"]
    try:
        assert run_miso.main(base) == 0
        assert run_miso.main(base + ["--exact"]) == 0
        assert run_miso.main(base + ["--settings-filename", str(settings)]) == 0
        assert Settings.get_exact() is True
    finally:
        Settings.load(None)
    assert [kw["exact"] for kw in calls] == [False, True, True]
    assert Settings.get_exact() is False


@pytest.mark.parametrize("text,want", [("True", True), ("1", True), ("true", True), ("yes", True), ("on", True),
                                       ("False", False), ("0", False), ("false", False), ("no", False), ("off", False)])
def test_settings_key_spellings(tmp_path, text, want):
    settings = tmp_path / "settings.txt"
    settings.write_text("[sampler]\nburn_in = 10\nlag = 2\nnum_iters = 100\nexact = %s\n" % text)
    try:
        Settings.load(str(settings))
        assert Settings.get_exact() is want
        settings.write_text("[sampler]\nburn_in = 10\nlag = 2\nnum_iters = 100\nexact = maybe\n")
        Settings.load(str(settings))
        with pytest.raises(ValueError, match="Invalid exact parameter"):
            Settings.get_exact()
    finally:
        Settings.load(None)


def test_compute_gene_psi_hands_the_switch_to_the_sampler(tmp_path, monkeypatch):
    """run_miso.compute_gene_psi(exact=True) -> params["exact"] of the MISOSampler it makes"""
    made = []

    class Stop(Exception):
        pass

    class FakeSampler(object):
        def __init__(self, params, **kw):
            made.append(dict(params))
            raise Stop()
    monkeypatch.setattr(run_miso.miso, "MISOSampler", FakeSampler)
    monkeypatch.setattr(run_miso, "collect_gene_events", lambda entries, *a, **kw: ([(None, None, None, None, 0)], {}))
    monkeypatch.setattr(run_miso, "preload_genes", lambda *a, **kw: None)
    for exact in (True, False):
        with pytest.raises(Stop):
            run_miso.compute_gene_psi(None, None, "reads.bam", str(tmp_path / "o"), 36, 1, gene_entries=[("g", "i")],
                                      bamfile=object(), exact=exact, verbose=False)
    assert ["exact" in p for p in made] == [True, False] and made[0]["exact"] == 1


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
    for flag in ([], ["--exact"]):
        assert miso_cli.main(["--run", idx, str(bam), "--output-dir", str(tmp_path / "out"), "--read-len", "36", "-p", "1"] + flag) == 0
    assert len(cmds) == 2 and "--exact" not in cmds[0] and "--exact" in cmds[1]


def test_no_cpu_path(tmp_path):
    match = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    b = miso_amd.Batch(36, iters=50, burn=10, lag=1, chains=1, exact=True)
    assert b.exact and b.add_problem(match, [135, 95], [1, 1]) == 0
    el = capi.C.c_int(-1)
    assert capi.lib().miso_exact_eligible(0, 2, capi._p(np.array([100.0, 60.0])), capi._p(np.ones(2)), capi.C.byref(el)) == 0
    assert el.value == 1
    assert capi.lib().miso_exact_eligible(0, 2, capi._p(np.array([100.0, 60.0])), capi._p(np.array([0.5, 1.0])), capi.C.byref(el)) == 0
    assert el.value == 0
    if capi.device_count() > 0:
        return      # (with a device the call works: tests/test_gpu_exact.py)
    with pytest.raises(miso_amd.InternalError, match="no HIP device"):
        b.run()
    assert b"no HIP device" in capi.lib().miso_last_error()
    with pytest.raises(miso_amd.InternalError, match="no HIP device"):
        capi.selftest_exact([[1, 1, 3, 100, 60, 1, 1]], [0.5])
