"""GPU: miso_batch_diagnose (miso_amd/csrc/kernels_diagnose.hip) against the fixed-order restatement of
tests/_diag_ref.py, bit for bit; `lag` as an integer.  The columns are chosen (batches adopted with from_samples), at the
smallest shapes at which each piece of the kernel can go wrong:

    C = 1, S = 8              h = 4, the minimum                    C = 1, S = 7        MISO_EINVAL
    C = 2, S = 18             n = 9 odd: the middle draw dropped    C = 6, S = 51       three ignored trailing columns
    C = 1, S = 8192 .. 8195   either side of the LDS path, see below   C = 6, S = 8200  the uncached path with a remainder
    a linear ramp             the lag loop runs out at 2k + 1 <= h - 1, h even (S = 16) and odd (S = 18)
    a constant column, a column with one NaN, one with one +inf: all-NaN outputs, lag 0; an ordinary column beside them
    K = 2, 3 and 40 in one batch: the grid's `k >= K` guard
    C = 2048 and 2049         the most chains taken (96 KB of per-sequence LDS) and the first count refused

The LDS path is chosen by the draws that are used, N = 2 C h <= 8192, not by S: at C = 1, S = 8192 and 8193 (N = 8192, the
odd n dropping its middle draw) are the last cached shapes and S = 8194 and 8195 (N = 8194) the first uncached ones, with
M = 2 sequences, so that a lag pair has four units, one per wavefront, and the moments loop leaves two wavefronts idle.
"""
import math

import numpy as np
import pytest

import _diag_ref as R
import _golden
from miso_amd import capi, workload

pytestmark = pytest.mark.gpu


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.int64)


def _check_event(b, i, samples, C, label):
    """Event i's four outputs against diag_fixed on every column."""
    rhat, ess, mcse, lag = b.diagnostics(i)
    assert lag.dtype == np.int64
    for k in range(samples.shape[1]):
        want = R.diag_fixed(samples[:, k], C)
        got = (rhat[k], ess[k], mcse[k], int(lag[k]))
        print("%s event %d column %d: got %r want %r" % (label, i, k, got, want))
        if math.isnan(want[0]):
            assert all(math.isnan(v) for v in got[:3]) and got[3] == 0, (label, i, k, got)
        else:
            assert got[3] == want[3], (label, i, k, got, want)
            assert np.array_equal(_bits(got[:3]), _bits(want[:3])), (label, i, k, got, want)


def _psi_like(rng, S, K, C, phi=0.3):
    """[S, K] columns of AR(1) chains around distinct means (so the columns differ), rows in the file's layout."""
    cols = [R.ar1(rng, phi, C, -(-S // C), mean=0.2 + 0.6 * k / K, sd=0.04)[:S] for k in range(K)]
    return np.ascontiguousarray(np.stack(cols, axis=1))


SHAPES = [(8, 1), (18, 2), (51, 6), (8192, 1), (8193, 1), (8194, 1), (8195, 1), (8200, 6)]


@pytest.fixture(scope="module")
def shaped():
    """Per (S, C): the events' samples, made once."""
    rng = np.random.default_rng(2024)
    out = {}
    for S, C in SHAPES:
        Ks = (2, 3, 40) if S < 100 else (2,)
        out[(S, C)] = [_psi_like(rng, S, K, C) for K in Ks]
    return out


@pytest.mark.parametrize("S,C", SHAPES)
def test_chosen_columns_bit_for_bit(shaped, S, C):
    events = shaped[(S, C)]
    b = capi.SamplesBatch(events)
    b.diagnose(C)
    for i, ev in enumerate(events):
        _check_event(b, i, ev, C, "S=%d C=%d" % (S, C))
    many = b.diagnostics_many(range(len(events)), [e.shape[1] for e in events])
    for i in range(len(events)):
        for a, c in zip(many[i], b.diagnostics(i)):
            assert np.array_equal(a, c, equal_nan=True)


def test_too_few_samples_per_chain():
    b = capi.SamplesBatch([np.random.default_rng(1).random((7, 2))])
    with pytest.raises(capi.InternalError, match="Too few samples per chain for diagnostics"):
        b.diagnose(1)
    with pytest.raises(capi.InternalError, match="has not run"):
        b.diagnostics(0)
    b16 = capi.SamplesBatch([np.random.default_rng(1).random((16, 2))])
    with pytest.raises(capi.InternalError, match="Too few samples per chain"):
        b16.diagnose(3)                                  # n = 5, h = 2


def test_the_most_chains_and_one_more():
    C, S = 2048, 2048 * 8                                # h = 4, M = 4096 sequences: uncached, 3 M doubles of LDS
    ev = _psi_like(np.random.default_rng(5), S, 2, C)
    b = capi.SamplesBatch([ev])
    b.diagnose(C)
    _check_event(b, 0, ev, C, "C=2048")
    wide = capi.SamplesBatch([np.random.default_rng(5).random((2049 * 8, 2))])
    with pytest.raises(capi.InternalError, match="Too many chains for diagnostics"):
        wide.diagnose(2049)
    with pytest.raises(capi.InternalError, match="has not run"):
        wide.diagnostics(0)


@pytest.mark.parametrize("S", [16, 18])
def test_a_ramp_runs_out_of_lags(S):
    h = S // 2
    ramp = np.arange(float(S))
    ev = np.ascontiguousarray(np.stack([ramp, 100.0 - 0.5 * ramp], axis=1))
    b = capi.SamplesBatch([ev])
    b.diagnose(1)
    _check_event(b, 0, ev, 1, "ramp S=%d" % S)
    assert b.diagnostics(0)[3].tolist() == [2 * ((h - 2) // 2 + 1)] * 2


@pytest.mark.parametrize("bad", ["constant", "nan", "inf"])
@pytest.mark.parametrize("S,C", [(51, 6), (8200, 6)])
def test_degenerate_columns_beside_an_ordinary_one(bad, S, C):
    rng = np.random.default_rng(7)
    ev = _psi_like(rng, S, 3, C)
    if bad == "constant":
        ev[:, 1] = 0.25
    else:
        ev[S // 3, 1] = math.nan if bad == "nan" else math.inf
    other = _psi_like(rng, S, 2, C)
    b = capi.SamplesBatch([ev, other])
    b.diagnose(C)
    rhat, ess, mcse, lag = b.diagnostics(0)
    assert math.isnan(rhat[1]) and math.isnan(ess[1]) and math.isnan(mcse[1]) and lag[1] == 0
    assert np.isfinite(rhat[[0, 2]]).all() and (lag[[0, 2]] >= 2).all()
    _check_event(b, 0, ev, C, "%s S=%d" % (bad, S))
    _check_event(b, 1, other, C, "beside %s S=%d" % (bad, S))


def test_errors():
    exons, isoforms, pos, cig = workload.event_reads(0, K=2, n_reads=50)
    b = capi.Batch(36, iters=600, burn=100, lag=5, chains=6)
    b.add_event(capi.Gene(exons, isoforms), pos, cig)
    with pytest.raises(capi.InternalError, match="not launched"):
        b.diagnose()
    with pytest.raises(capi.InternalError):
        b.diagnostics(0)
    s = capi.SamplesBatch([np.random.default_rng(3).random((64, 2))])
    with pytest.raises(capi.InternalError, match="no chain count"):
        s.diagnose()                                     # chains = 0: an adopted batch has none of its own
    with pytest.raises(capi.InternalError, match="has not run"):
        s.diagnostics(0)
    with pytest.raises(capi.InternalError):
        s.diagnose(-1)
    s.diagnose(2)
    assert s.diagnostics(0)[0].shape == (2,)


def _sampled_batch(stop):
    b = capi.Batch(36, iters=600, burn=100, lag=5, chains=6, stop=stop, max_iters=20000)
    for e in range(8):
        exons, isoforms, pos, cig = workload.event_reads(e, K=2, n_reads=50)
        b.add_event(capi.Gene(exons, isoforms), pos, cig)
    return b


def test_sampled_batch_and_relaunch():
    b = _sampled_batch(capi.MISO_STOP_FIXEDNO)
    b.run(device=0, seed=11, first_event_id=0)
    b.diagnose()
    first = [b.result(i).samples.copy() for i in range(8)]
    for i in range(8):
        assert first[i].shape == (600, 2)
        _check_event(b, i, first[i], 6, "sampled")
    b.launch(seed=12, first_event_id=0)
    with pytest.raises(capi.InternalError, match="has not run"):
        b.diagnostics(0)
    b.sync()
    b.diagnose()
    b.download()
    for i in range(8):
        again = b.result(i).samples
        assert not np.array_equal(again, first[i])
        _check_event(b, i, again, 6, "relaunched")


def test_convergent_mean_diagnoses_the_last_round():
    b = _sampled_batch(capi.MISO_STOP_CONVERGENT_MEAN)
    b.upload(0)
    b.launch(seed=11, first_event_id=0)
    b.diagnose()                                         # runs sync() and with it the further rounds
    rounds = b.rounds()
    print("CONVERGENT_MEAN rounds:", rounds)
    b.download()
    assert b.rounds() == rounds
    for i in range(8):
        _check_event(b, i, b.result(i).samples, 6, "convergent")


@pytest.mark.parametrize("name", ["se_k2_convergent", "se_k3_convergent"])
def test_convergent_mean_after_further_rounds(name):
    """The events of tests/test_gpu_convergent.py, which need more than one round: diagnose() straight after launch() has
    to run them, and what it diagnoses is what download() then returns, not the first round."""
    g = _golden.load(name)
    kw = dict(iters=g["iters"], burn=g["burn"], lag=g["lag"], chains=g["chains"], overhang=g["overhang"])
    G = capi.Gene(g["exon_list"], g["isoform_list"])
    fixed = capi.Batch(g["read_len"], stop=capi.MISO_STOP_FIXEDNO, **kw)
    fixed.add_event(G, g["pos"], g["cigars"])
    fixed.run(seed=11, first_event_id=77)
    b = capi.Batch(g["read_len"], stop=capi.MISO_STOP_CONVERGENT_MEAN, max_iters=g["max_iters"], **kw)
    b.add_event(G, g["pos"], g["cigars"])
    b.upload(0)
    b.launch(seed=11, first_event_id=77)
    b.diagnose()
    assert b.rounds() > 1
    b.download()
    last = b.result(0).samples
    assert not np.array_equal(last, fixed.result(0).samples)        # the first round is the FIXEDNO run
    _check_event(b, 0, last, int(g["chains"]), name)
