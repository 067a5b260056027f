"""CPU: the exact comparison of two exact-mode posteriors (tests/_exact_compare_ref.py, the restatement of
csrc/kernels_exact_compare.hip) against mpmath, its symmetries, the `.miso_bf_exact` writer and the
front end's argument errors.

The reference side: the three normalisers are integrated in logit space piece by piece around their modes, as
tests/test_exact_ref.py does.  H(z) = P(psi_1 - psi_2 <= z) is a composite Gauss-Legendre rule over the narrower
posterior's window, split where the shifted argument leaves (0, 1); the other posterior's CDF at all of its nodes (every
z at once) is the regularised incomplete beta function where the effective lengths are equal and the reads few, else the
density integrated between the sorted arguments (five-point Gauss-Legendre between close neighbours, mp.quad otherwise:
the scheme of tests/test_gpu_exact.py's Kolmogorov-Smirnov reference).
"""
import os

import mpmath as mp
import numpy as np
import pytest

from _exact_compare_ref import HYPERS, PAIRS, ZS, compare, log_prior0, pair_rows, pooled_row
from _exact_ref import Posterior, Stats
from miso_amd import compare as compare_py
from miso_amd import filter_events
from miso_amd import miso as miso_cli

H_TOL = 5e-6        # half a unit of the fifth decimal; the table prints four
COMBOS = [(p, h) for h in HYPERS for p in PAIRS]
COMBO_IDS = ["%s|%s|%s-h%g_%g" % (",".join(map(str, p[0])), ",".join(map(str, p[1])), ",".join(map(str, p[2])), h[0], h[1])
             for p, h in COMBOS]
_worst = {"d0": (0.0, None), "H": (0.0, None)}


@pytest.fixture(scope="module")
def post(orc):
    return Posterior(orc)


_results = {}


def result_of(post, pair, hyper, zs=tuple(ZS)):
    """the restatement's output and its three tables, computed once per (pair, hyper, zs)"""
    key = (pair, hyper, zs)
    if key not in _results:
        r1, r2 = pair_rows(pair, hyper)
        tabs = [post.tabulate(Stats(*r)) for r in (r1, r2, pooled_row(r1, r2))]
        _results[key] = (compare(post, r1, r2, zs), tabs, (r1, r2))
    return _results[key]


class MpPosterior:
    """the density of a row (n10, n01, n, e0, e1, h0, h1) in logit space, scaled by exp(-gmax) of its restated table"""

    def __init__(self, row, tab):
        self.a, self.b = mp.mpf(row[0]) + mp.mpf(row[5]), mp.mpf(row[1]) + mp.mpf(row[6])
        self.n, self.e0, self.e1 = mp.mpf(row[2]), mp.mpf(row[3]), mp.mpf(row[4])
        self.gmax = mp.mpf(float(tab["gmax"]))
        self.tm, self.tL, self.tR = (mp.mpf(float(tab[k])) for k in ("tm", "tL", "tR"))

    def f(self, t):
        # x = 1 / (1 + e^-t), y = 1 - x; both exponents are >= 1 in logit space, so no 0 log 0 arises at an edge
        if t >= 0:
            em = mp.exp(-t)
            lx, ly = -mp.log1p(em), -t - mp.log1p(em)
            lden = mp.log(self.e0 + em * self.e1) - mp.log1p(em)
        else:
            ep = mp.exp(t)
            lx, ly = t - mp.log1p(ep), -mp.log1p(ep)
            lden = mp.log(ep * self.e0 + self.e1) - mp.log1p(ep)
        return mp.exp(self.a * lx + self.b * ly - self.n * lden - self.gmax)

    def landmarks(self):
        tm, tL, tR = self.tm, self.tL, self.tR
        return [tm - 300, tL, tm - (tm - tL) / 4, tm - (tm - tL) / 16, tm, tm + (tR - tm) / 16, tm + (tR - tm) / 4, tR, tm + 300]

    def log_Z(self):
        pts = sorted(set(self.landmarks()))
        return self.gmax + mp.log(sum(mp.quad(self.f, [lo, hi]) for lo, hi in zip(pts[:-1], pts[1:])))


def _gauss_legendre(n):
    """nodes and weights on [-1, 1] (Newton on the Legendre polynomial, in mp precision)"""
    xs, ws = [], []
    for i in range(1, n + 1):
        x = mp.cos(mp.pi * (i - mp.mpf(1) / 4) / (n + mp.mpf(1) / 2))
        for _ in range(100):
            p0, p1 = mp.mpf(1), x
            for k in range(2, n + 1):
                p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
            dp = n * (x * p1 - p0) / (x * x - 1)
            dx = p1 / dp
            x -= dx
            if abs(dx) < mp.mpf(10) ** (-mp.mp.dps + 2):
                break
        xs.append(x)
        ws.append(2 / ((1 - x * x) * dp * dp))
    return xs, ws


def mp_cdf_at(B, row_b, us):
    """the CDF of posterior B at psi = us (mp numbers; <= 0 gives 0, >= 1 gives 1), all at once"""
    out = {}
    inside = sorted({u for u in us if 0 < u < 1})
    for u in us:
        if u <= 0:
            out[u] = mp.mpf(0)
        elif u >= 1:
            out[u] = mp.mpf(1)
    if not inside:
        return out
    if row_b[3] == row_b[4] and row_b[2] < 1e4:     # a Beta law
        for u in inside:
            out[u] = mp.betainc(B.a, B.b, 0, u, regularized=True)
        return out
    ts = {u: mp.log(u) - mp.log1p(-u) for u in inside}
    gx, gw = _gauss_legendre(5)
    short = (B.tR - B.tL) / 256
    lm = B.landmarks()
    pts = sorted(set(lm) | {t for t in ts.values() if lm[0] < t < lm[-1]})
    cum, acc = {pts[0]: mp.mpf(0)}, mp.mpf(0)
    for lo, hi in zip(pts[:-1], pts[1:]):
        if hi - lo <= short:
            c, r = (lo + hi) / 2, (hi - lo) / 2
            acc += r * sum(w * B.f(c + r * x) for x, w in zip(gx, gw))
        else:
            acc += mp.quad(B.f, [lo, hi])
        cum[hi] = acc
    for u in inside:
        t = ts[u]
        out[u] = mp.mpf(0) if t <= lm[0] else mp.mpf(1) if t >= lm[-1] else cum[t] / acc
    return out


def mp_H(rows, tabs, zs, panels=32, order=8):
    """P(psi_1 - psi_2 <= z) for every z, from the narrower posterior's side"""
    mp.mp.dps = 30
    P = [MpPosterior(rows[0], tabs[0]), MpPosterior(rows[1], tabs[1])]
    width = [1 / (1 + mp.exp(-p.tR)) - 1 / (1 + mp.exp(-p.tL)) for p in P]
    a_is_2 = width[1] < width[0]
    A, B, row_b = (P[1], P[0], rows[0]) if a_is_2 else (P[0], P[1], rows[1])
    gx, gw = _gauss_legendre(order)
    zs = [mp.mpf(z) for z in zs]
    # the argument of B's CDF is x + z (A = sample 2) or x - z (A = sample 1): it leaves (0, 1) at x = -+z, 1 -+ z
    kinks = set()
    for z in zs:
        s = -z if a_is_2 else z
        for x in (s, 1 + s):
            if 0 < x < 1:
                t = mp.log(x) - mp.log1p(-x)
                if A.tL < t < A.tR:
                    kinks.add(t)
    edges = sorted({A.tL + (A.tR - A.tL) * k / panels for k in range(panels + 1)} | kinks)
    nodes = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        c, r = (lo + hi) / 2, (hi - lo) / 2
        for x, w in zip(gx, gw):
            t = c + r * x
            nodes.append((t, r * w * A.f(t)))
    total = sum(w for _, w in nodes)
    xs = [1 / (1 + mp.exp(-t)) for t, _ in nodes]
    args = {z: [(x + z) if a_is_2 else (x - z) for x in xs] for z in zs}
    cdf = mp_cdf_at(B, row_b, [u for z in zs for u in args[z]])
    out = []
    for z in zs:
        s = sum(w * cdf[u] for (_, w), u in zip(nodes, args[z])) / total
        out.append(float(s if a_is_2 else 1 - s))
    return out


@pytest.mark.parametrize("pair,hyper", COMBOS, ids=COMBO_IDS)
def test_log_density_at_zero_against_mpmath(post, pair, hyper):
    got, tabs, rows = result_of(post, pair, hyper)
    mp.mp.dps = 40
    lz = [MpPosterior(r, t).log_Z() for r, t in zip(rows + (pooled_row(*rows),), tabs)]
    want = (lz[2] - lz[0]) - lz[1]
    err = abs(float(mp.mpf(float(got[2])) - want))
    bound = 16 * 2.0 ** -53 * float(sum(abs(v) for v in lz)) + 1e-12
    if err / bound > _worst["d0"][0]:
        _worst["d0"] = (err / bound, (pair, hyper, err, bound))
    print("log_d0 %.17g, error %.3g, bound %.3g; worst error / bound so far %.3g at %s" % ((got[2], err, bound) + _worst["d0"]))
    assert err <= bound
    # the Bayes factor that goes with it
    log_bf = float(log_prior0(*rows)) - float(got[2])
    assert got[4] == np.float64(log_bf) / np.float64(2.302585092994046)
    assert got[3] == min(post.exp(np.float64(log_bf)), 1e12)
    if hyper == (1.0, 1.0):
        assert log_prior0(*rows) == 0.0


@pytest.mark.parametrize("pair,hyper", COMBOS, ids=COMBO_IDS)
def test_cdf_of_the_difference_against_mpmath(post, pair, hyper):
    got, tabs, rows = result_of(post, pair, hyper)
    want = mp_H(rows, tabs, ZS)
    errs = [abs(g - w) for g, w in zip(got[5:], want)]
    if max(errs) > _worst["H"][0]:
        _worst["H"] = (max(errs), (pair, hyper, ZS[int(np.argmax(errs))]))
    print("H %s, errors %s; worst so far %.3g at %s" % ((["%.7f" % g for g in got[5:]], ["%.2g" % e for e in errs]) + _worst["H"]))
    assert max(errs) <= H_TOL
    assert all(0.0 <= g <= 1.0 for g in got[5:])


@pytest.mark.parametrize("hyper", HYPERS, ids=lambda h: "h%g_%g" % h)
def test_monotone_and_symmetric(post, hyper):
    zs = (-0.2, -0.1, -0.05, 0.0, 0.05, 0.1, 0.2)
    for pair in PAIRS:
        r1, r2 = pair_rows(pair, hyper)
        a = compare(post, r1, r2, zs)
        b = compare(post, r2, r1, zs)
        assert (np.diff(a[5:]) >= 0).all() and (np.diff(b[5:]) >= 0).all(), pair
        assert np.abs(b[5:] - (1.0 - a[5:][::-1])).max() <= 1e-5, (pair, a[5:], b[5:])
        tabs = [post.tabulate(Stats(*r)) for r in (r1, r2, pooled_row(r1, r2))]
        lz = [abs(float(t["gmax"] + post.log(t["Z"]))) for t in tabs]
        assert abs(a[2] - b[2]) <= 16 * 2.0 ** -53 * sum(lz) + 1e-12, pair
        assert (a[0], a[1]) == (b[1], b[0])


# ---- the `.miso_bf_exact` writer ----
H1 = {"isoforms": "'A_up_B_dn','A_up_dn'", "counts": "(0,1):5,(1,0):11,(1,1):17", "assigned_counts": "0:20,1:13",
      "chrom": "chr1", "strand": "+", "mRNA_starts": "100,100", "mRNA_ends": "900,900"}
H2 = dict(H1, counts="(0,1):9,(1,0):3,(1,1):20", assigned_counts="0:12,1:20")


def _rows():
    s1 = (np.array([0.56, 0.44]), np.array([0.31, 0.2]), np.array([0.8, 0.69]))
    s2 = (np.array([0.2, 0.8]), np.array([0.07, 0.6]), np.array([0.4, 0.93]))
    grid1 = (np.array([0.5640391, 0.4359609]), np.array([0.30512, 0.2]), np.array([0.80004, 0.69]))
    grid2 = (np.array([0.1961334, 0.8038666]), np.array([0.06, 0.6]), np.array([0.39996, 0.93]))
    # cdf at (0.1, -0.1, 0.2, -0.2)
    exact = (0.5640391, 0.1961334, -1.88604, 3.2e13, 13.505, np.array([0.04, 0.001, 0.13, 0.0002]), grid1, grid2)
    return [("ev_exact", s1, s2, [6.4, 6.4], H1, H2, exact), ("ev_sampled", s1, s2, [6.4, 6.4], H1, H2, None)]


def test_writer_and_filter(tmp_path):
    path = str(tmp_path / "a_vs_b.miso_bf_exact")
    assert compare_py.write_exact_comparison(path, _rows(), [0.1, 0.2]) == 2
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) == 4
    header = lines[0].split("\t")
    assert header == compare_py.HEADER_FIELDS + ["exact", "log10_bayes_factor", "prob_abs_diff_ge_0.1", "prob_abs_diff_ge_0.2"]
    row = dict(zip(header, lines[1].split("\t")))
    assert row == dict(event_name="ev_exact", sample1_posterior_mean="0.5640", sample1_ci_low="0.3051", sample1_ci_high="0.8000",
                       sample2_posterior_mean="0.1961", sample2_ci_low="0.0600", sample2_ci_high="0.4000", diff="0.3679",
                       bayes_factor="1000000000000.00", isoforms=H1["isoforms"], sample1_counts=H1["counts"],
                       sample1_assigned_counts=H1["assigned_counts"], sample2_counts=H2["counts"],
                       sample2_assigned_counts=H2["assigned_counts"], chrom="chr1", strand="+", mRNA_starts="100,100",
                       mRNA_ends="900,900", exact="1", log10_bayes_factor="13.5050",
                       **{"prob_abs_diff_ge_0.1": "0.9610", "prob_abs_diff_ge_0.2": "0.8702"})
    # any other event: its `.miso_bf` line verbatim, then exact = 0 and NA
    plain = compare_py.comparison_line(*_rows()[1][:6])
    assert lines[2] == plain + "\t0\tNA\tNA\tNA"
    # filter_events reads the table by column name
    t = filter_events.Table(path)
    assert filter_events.filter_rows(t) == [0, 1]
    assert filter_events.filter_rows(t, bayes_factor=10.0) == [0]
    assert filter_events.filter_rows(t, delta_psi=0.365) == [0]
    done = filter_events.multi_filter([path], str(tmp_path / "filtered"), bf_filter=10.0, out=open(os.devnull, "w"))
    assert done == [(str(tmp_path / "filtered" / "a_vs_b.miso_bf_exact.filtered"), 1, 2)]
    assert open(done[0][0]).read() == lines[0] + "\n" + lines[1] + "\n"


def test_writer_thresholds():
    assert compare_py.delta_points([0.1, 0.25]) == (0.1, -0.1, 0.25, -0.25)
    assert compare_py.exact_header_fields([0.05, 0.5])[-2:] == ["prob_abs_diff_ge_0.05", "prob_abs_diff_ge_0.5"]
    for bad in ([], [0.0], [1.0], [-0.1], [0.1, 0.2, 0.3, 0.4, 0.5]):
        with pytest.raises(ValueError):
            compare_py.check_delta_thresholds(bad)


# ---- `miso --run ... --exact-compare`: argument errors before any work ----
@pytest.mark.parametrize("extra,message", [
    (["--exact", "--exact-compare"], "goes with --compare"),
    (["--compare", "b.bam", "--exact-compare"], "needs the exact-posterior mode"),
    (["--compare", "b.bam", "--exact", "--exact-compare", "--paired-end", "250", "30"], "single-end"),
    (["--compare", "b.bam", "--exact", "--exact-compare", "--delta-psi-thresholds", "0.1", "1.0"], "outside"),
    (["--compare", "b.bam", "--exact", "--delta-psi-thresholds", "0.1"], "goes with --exact-compare"),
], ids=["no-compare", "no-exact-mode", "paired-end", "bad-threshold", "thresholds-alone"])
def test_miso_argument_errors(tmp_path, monkeypatch, capsys, extra, message):
    def never(*a, **kw):
        raise AssertionError("work was started")
    monkeypatch.setattr(miso_cli, "compute_all_genes_psi", never)
    monkeypatch.setattr(miso_cli, "GenesDispatcher", never)
    with pytest.raises(SystemExit) as e:
        miso_cli.main(["--run", str(tmp_path / "index"), str(tmp_path / "a.bam"), "--read-len", "36",
                       "--output-dir", str(tmp_path / "out")] + extra)
    assert e.value.code == 2
    assert message in capsys.readouterr().err
    assert not (tmp_path / "out").exists()
