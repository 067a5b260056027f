"""A fixed-order restatement of the exact comparison of two exact-mode posteriors (miso_amd/csrc/kernels_exact_compare.hip,
DESIGN.md section 16), built on tests/_exact_ref.py's Posterior: every operation is one IEEE-754 double operation in the
kernel's order, so the device's results can be compared with these bit for bit (tests/test_gpu_exact_compare.py) and
these with mpmath (tests/test_exact_compare_ref.py).  Test infrastructure only: nothing under miso_amd/ imports it.
"""
import numpy as np

from _exact_ref import CELLS, EDGE_ROUNDS, G, LANES, MODE_ROUNDS, T_MODE, T_SPAN, DROP, Stats, lgamma

LN10 = np.float64(2.302585092994046)
BF_CAP = np.float64(1e12)

# the issue's pair list: (n10, n01, n11) of sample 1, of sample 2, (e0, e1)
PAIRS = [
    ((0, 0, 0), (0, 0, 0), (100, 60)),
    ((11, 5, 17), (3, 9, 20), (179, 140)),
    ((400, 300, 300), (300, 400, 300), (275, 165)),
    ((400, 300, 300), (410, 290, 300), (275, 165)),
    ((40000, 30000, 30000), (39000, 31000, 30000), (275, 165)),
    ((40000, 30000, 30000), (11, 5, 17), (275, 165)),
    ((11, 5, 17), (40000, 30000, 30000), (275, 165)),
    ((50000, 0, 0), (3, 0, 0), (1000, 20)),
    ((0, 17, 13), (17, 0, 13), (175, 140)),
    ((1, 100000, 0), (0, 60000, 20000), (150, 150)),
    ((0, 0, 5), (0, 0, 7), (150, 150)),
    ((3, 0, 0), (0, 0, 0), (150, 150)),
]
HYPERS = [(1.0, 1.0), (2.0, 5.0)]
ZS = [-0.2, -0.05, 0.0, 0.05, 0.1, 0.2]


def pair_rows(pair, hyper):
    """the two samples' statistics in miso_selftest_exact's layout: (n10, n01, n, e0, e1, h0, h1)"""
    c1, c2, (e0, e1) = pair
    return tuple([float(c[0]), float(c[1]), float(sum(c)), float(e0), float(e1), float(hyper[0]), float(hyper[1])] for c in (c1, c2))


def pooled_row(r1, r2):
    """the product of the two posteriors as a posterior of its own"""
    f = np.float64
    return [f(r1[0]) + f(r2[0]), f(r1[1]) + f(r2[1]), f(r1[2]) + f(r2[2]), f(r1[3]), f(r1[4]),
            (f(r1[5]) + f(r2[5])) - f(1.0), (f(r1[6]) + f(r2[6])) - f(1.0)]


def log_prior0(r1, r2):
    """log of the prior density of psi_1 - psi_2 at 0, the host's arithmetic (the C library's lgamma)"""
    f = np.float64
    h0p, h1p = (f(r1[5]) + f(r2[5])) - f(1.0), (f(r1[6]) + f(r2[6])) - f(1.0)
    lp = (f(lgamma(h0p)) + f(lgamma(h1p))) - f(lgamma(h0p + h1p))
    for r in (r1, r2):
        lp = lp - ((f(lgamma(r[5])) + f(lgamma(r[6]))) - f(lgamma(f(r[5]) + f(r[6]))))
    return lp


def window(post, st):
    """steps 1 - 2 of the scheme alone: mode, window, and the window's width in psi"""
    f64 = np.float64
    lo, hi = post._section(st, f64(-T_MODE), f64(T_MODE), MODE_ROUNDS, lambda pt: ~(pt[1] > 0.0))
    tm = f64(0.5) * (lo + hi)
    gmax = post.point(st, tm)[0]
    thr = gmax - f64(DROP)
    tL, _ = post._section(st, tm - f64(T_SPAN), tm, EDGE_ROUNDS, lambda pt: pt[0] >= thr)
    _, tR = post._section(st, tm, tm + f64(T_SPAN), EDGE_ROUNDS, lambda pt: pt[0] < thr)
    width = post.point(st, tR)[2] - post.point(st, tL)[2]
    return tm, gmax, tL, tR, width


def lane_sum(term):
    """sum over the G + 1 grid points in the mean's order: a lane's own points in order (the last lane takes the grid's last
    point too), then the lanes in order"""
    acc = np.zeros(LANES)
    body = term[:G].reshape(LANES, CELLS)
    for j in range(CELLS):
        acc = acc + body[:, j]
    acc[LANES - 1] = acc[LANES - 1] + term[G]
    s = np.float64(0.0)
    for l in range(LANES):
        s = s + acc[l]
    return s


def table_cdf(tab, u, v):
    """the tabulated, unnormalised CDF at psi = u, with v = 1 - psi computed on its own: the cubic Hermite interpolant of F on
    the cell of logit psi, 0 / Z where the argument leaves (0, 1) or the window"""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    F, f, h, Z = tab["F"], tab["f"], tab["h"], tab["Z"]
    post = tab["post"]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = post.log(np.where(u > 0.0, u, 1.0)) - post.log(np.where(v > 0.0, v, 1.0))
        s = (t - tab["tL"]) / h
        s = np.where(s > 0.0, s, 0.0)
        s = np.where(s < np.float64(G), s, np.float64(G))
        j = np.minimum(s.astype(np.int64), G - 1)
        fr = s - j.astype(np.float64)
        F0, F1, m0, m1 = F[j], F[j + 1], h * f[j], h * f[j + 1]
        dF = F1 - F0
        c2 = (3.0 * dF - 2.0 * m0) - m1
        c3 = (m0 + m1) - 2.0 * dF
        val = F0 + (m0 + fr * (c2 + fr * c3)) * fr
    val = np.where(val > Z, Z, val)
    val = np.where(val < 0.0, 0.0, val)
    val = np.where(t >= tab["tR"], Z, val)
    val = np.where(u > 0.0, val, 0.0)
    val = np.where(v > 0.0, val, Z)
    return val


def compare(post, r1, r2, zs=()):
    """what exact_compare reports of one comparable pair: [mean1, mean2, log_d0, bayes_factor, log10_bf, H(z) ...]"""
    f64 = np.float64
    st = [Stats(*r1), Stats(*r2), Stats(*pooled_row(r1, r2))]
    w1, w2 = window(post, st[0])[4], window(post, st[1])[4]
    a_is_2 = bool(w2 < w1)       # A: the narrower window in psi, a tie goes to sample 1
    tabs = [post.tabulate(s) for s in st]
    for tb in tabs:
        tb["post"] = post
    lz = [tb["gmax"] + post.log(tb["Z"]) for tb in tabs]
    log_d0 = (lz[2] - lz[0]) - lz[1]
    log_bf = log_prior0(r1, r2) - log_d0
    bf = post.exp(log_bf)
    bf = BF_CAP if bf > BF_CAP else bf
    out = [tabs[0]["mean0"], tabs[1]["mean0"], log_d0, bf, log_bf / LN10]
    A, B = (tabs[1], tabs[0]) if a_is_2 else (tabs[0], tabs[1])
    t = A["tL"] + A["h"] * np.arange(G + 1, dtype=np.float64)
    g, _, x, y, _, _, _ = post.point(A["st"], t)
    wgt = np.ones(G + 1)
    wgt[0] = wgt[G] = 0.5
    wf = wgt * post.exp(g - A["gmax"])
    sf = lane_sum(wf)
    for z in zs:
        z = f64(z)
        if a_is_2:      # H = sum w F_1(y + z) / Z_1
            val = table_cdf(B, x + z, y - z)
        else:           # H = 1 - sum w F_2(x - z) / Z_2
            val = table_cdf(B, x - z, y + z)
        s = lane_sum(wf * (val / B["Z"])) / sf
        out.append(s if a_is_2 else f64(1.0) - s)
    return np.array(out, dtype=np.float64)
