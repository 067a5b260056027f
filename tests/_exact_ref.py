"""A fixed-order restatement of the exact-posterior mode (miso_amd/csrc/kernels_exact.hip).

Every floating-point operation below is one IEEE-754 double operation in the order the kernel makes it (numpy's
elementwise + - * / on float64 are exactly those; nothing here is fused), `exp` / `log` are the checker library's
orc_det_exp / orc_det_log (include/miso_detmath.h) and the uniforms its Philox (include/miso_philox.h), so the device's
results can be compared with these bit for bit (tests/test_gpu_exact.py) and these with mpmath (tests/test_exact_ref.py).
Test infrastructure only: nothing under miso_amd/ imports this module.
"""
import ctypes as C
import ctypes.util

import numpy as np

G = 2048            # cells of the grid (G + 1 points)
LANES = 64          # one wavefront per event: lane l owns cells [CELLS l, CELLS l + CELLS)
CELLS = G // LANES
DROP = 40.0         # the window: where the log density (logit space) is within DROP of its largest value
T_MODE = 64.0       # the mode is looked for in [-T_MODE, T_MODE] ...
T_SPAN = 128.0      # ... and each window end within T_SPAN of it
MODE_ROUNDS, EDGE_ROUNDS, NEWTON = 4, 3, 4
SITE_EXACT = 5      # include/miso_philox.h MISO_SITE_EXACT
SITE_GIBBS, ITER_INIT = 2, 0xFFFFFFFF

# the issue's case list: (n10, n01, n11, e0, e1)
CASES = [
    (0, 0, 0, 100, 60),
    (0, 0, 1000, 300, 100),
    (0, 17, 13, 175, 140),
    (11, 5, 17, 179, 140),
    (3, 0, 0, 50, 1),
    (400, 300, 300, 275, 165),
    (0, 60000, 20000, 500, 300),
    (40000, 30000, 30000, 275, 165),
    (50000, 0, 0, 1000, 20),
    (1, 100000, 0, 150, 150),
]
HYPERS = [(1.0, 1.0), (2.0, 5.0), (0.5, 0.5)]

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.lgamma.restype = C.c_double
_libm.lgamma.argtypes = [C.c_double]


def lgamma(x):
    """the C library's lgamma: what the host packs into the event's constants (host.cpp: std::lgamma)"""
    return float(_libm.lgamma(float(x)))


HYPER_MAX = 2.0 ** 20                      # csrc/batch.hpp EXACT_HYPER_MAX
LEN_MIN, LEN_MAX = 2.0 ** -40, 2.0 ** 40    # EXACT_LEN_MIN, EXACT_LEN_MAX
LEN_RATIO_MAX = 2.0 ** 20                   # EXACT_LEN_RATIO_MAX


def fence(length, hyper):
    """csrc/batch.hpp exact_fence: both hyperparameters in [1, 2^20], both lengths in [2^-40, 2^40] and within a factor 2^20
    of each other (false for a NaN, an infinity)"""
    return (all(1 <= h <= HYPER_MAX for h in hyper[:2]) and all(LEN_MIN <= e <= LEN_MAX for e in length[:2])
            and length[0] <= LEN_RATIO_MAX * length[1] and length[1] <= LEN_RATIO_MAX * length[0])


def eligible(paired, K, eff, hyper):
    """include/miso_amd.h miso_exact_eligible: single-end, two isoforms, effective lengths and hyperparameters inside the fence"""
    return (not paired) and K == 2 and fence(eff, hyper)


class Stats:
    """the five statistics of an event and its hyperparameters, as the kernel holds them"""

    def __init__(self, n10, n01, n, e0, e1, h0, h1):
        f = np.float64
        self.n10, self.n01, self.n = f(n10), f(n01), f(n)
        self.e0, self.e1 = f(e0), f(e1)
        self.hm0, self.hm1 = f(h0) - f(1.0), f(h1) - f(1.0)          # the packed constants are hyper - 1
        self.am1, self.bm1 = self.n10 + self.hm0, self.n01 + self.hm1  # exponents of x and 1 - x in p(x)
        self.a, self.b = self.am1 + f(1.0), self.bm1 + f(1.0)          # ... in logit space (the Jacobian x (1 - x))
        self.c = (self.a + self.b) - self.n
        self.lg_sum = f(lgamma(h0 + h1))
        self.lg_each = f(lgamma(h0) + lgamma(h1))


def case_stats(case, hyper):
    n10, n01, n11, e0, e1 = case
    return Stats(n10, n01, n10 + n01 + n11, e0, e1, hyper[0], hyper[1])


class Posterior:
    def __init__(self, orc):
        self.orc = orc
        self._exp = np.frompyfunc(lambda v: orc.lib.orc_det_exp(float(v)), 1, 1)
        self._log = np.frompyfunc(lambda v: orc.lib.orc_det_log(float(v)), 1, 1)

    def exp(self, v):
        return np.asarray(self._exp(np.asarray(v, np.float64)), dtype=np.float64)

    def log(self, v):
        return np.asarray(self._log(np.asarray(v, np.float64)), dtype=np.float64)

    def point(self, st, t):
        """at logit-space points t: g (log density up to a constant), g', x, 1 - x, L = log(1 + E), log of the denominator's
        numerator, |t|"""
        t = np.asarray(t, np.float64)
        at = np.abs(t)
        E = self.exp(-at)
        s = 1.0 + E
        L = self.log(s)
        pos = t >= 0
        r = 1.0 / s
        Er = E / s
        x = np.where(pos, r, Er)
        y = np.where(pos, Er, r)
        Ee0 = E * st.e0
        Ee1 = E * st.e1
        den = np.where(pos, st.e0 + Ee1, Ee0 + st.e1)
        ld = self.log(den)
        lin = np.where(pos, st.b, st.a) * at
        g = ((0.0 - lin) - st.c * L) - st.n * ld
        q = np.where(pos, st.e0, Ee0) / den
        gp = st.a - (st.c * x + st.n * q)
        return g, gp, x, y, L, ld, at

    def _section(self, st, lo, hi, rounds, pred):
        """`rounds` times: 64 points inside [lo, hi], the first at which pred holds closes the new interval"""
        k = np.arange(1, LANES + 1, dtype=np.float64)
        for _ in range(rounds):
            w = (hi - lo) / np.float64(65.0)
            pts = lo + w * k
            p = pred(self.point(st, pts))
            idx = int(np.argmax(p)) if p.any() else LANES
            nlo = lo if idx == 0 else lo + w * np.float64(idx)
            nhi = hi if idx == LANES else lo + w * np.float64(idx + 1)
            lo, hi = nlo, nhi
        return lo, hi

    def tabulate(self, st):
        f64 = np.float64
        lo, hi = self._section(st, f64(-T_MODE), f64(T_MODE), MODE_ROUNDS, lambda pt: ~(pt[1] > 0.0))
        tm = f64(0.5) * (lo + hi)
        gmax = self.point(st, tm)[0]
        thr = gmax - f64(DROP)
        tL, _ = self._section(st, tm - f64(T_SPAN), tm, EDGE_ROUNDS, lambda pt: pt[0] >= thr)
        _, tR = self._section(st, tm, tm + f64(T_SPAN), EDGE_ROUNDS, lambda pt: pt[0] < thr)
        h = (tR - tL) / f64(G)
        t = tL + h * np.arange(G + 1, dtype=np.float64)
        g, gp, x, y, _, _, _ = self.point(st, t)
        f = self.exp(g - gmax)
        d = f * gp
        hh = f64(0.5) * h
        h12 = (h * h) / f64(12.0)
        cell = hh * (f[:-1] + f[1:]) + h12 * (d[:-1] - d[1:])
        cell = np.where(cell < 0.0, 0.0, cell)
        F = np.zeros(G + 1)
        part = np.zeros(LANES)
        loc = np.zeros((LANES, CELLS))
        for l in range(LANES):
            acc = f64(0.0)
            for j in range(CELLS):
                acc = acc + cell[CELLS * l + j]
                loc[l, j] = acc
            part[l] = acc
        off = f64(0.0)
        for l in range(LANES):
            F[CELLS * l + 1: CELLS * l + CELLS + 1] = off + loc[l]
            off = off + part[l]
        # the mean: trapezoid sums, a lane's own points in order (the last lane takes the grid's last point too), then lanes in order
        wgt = np.ones(G + 1)
        wgt[0] = wgt[G] = 0.5
        wf = wgt * f
        xf, yf = x * wf, y * wf
        sx = sy = sf = f64(0.0)
        for l in range(LANES):
            ax = ay = af = f64(0.0)
            for i in range(CELLS * l, CELLS * l + CELLS + (1 if l == LANES - 1 else 0)):
                ax, ay, af = ax + xf[i], ay + yf[i], af + wf[i]
            sx, sy, sf = sx + ax, sy + ay, sf + af
        return dict(st=st, tm=tm, gmax=gmax, tL=tL, tR=tR, h=h, f=f, F=F, Z=F[G], mean0=sx / sf, mean1=sy / sf)

    def invert(self, tab, target):
        """the logit-space points at which the tabulated CDF takes the values `target` (array)"""
        T = np.asarray(target, np.float64)
        F, f, h = tab["F"], tab["f"], tab["h"]
        lo = np.zeros(T.shape, np.int64)
        hi = np.full(T.shape, G, np.int64)
        for _ in range(11):
            mid = (lo + hi) >> 1
            le = F[mid] <= T
            lo = np.where(le, mid, lo)
            hi = np.where(le, hi, mid)
        j = lo
        F0, F1, m0, m1 = F[j], F[j + 1], h * f[j], h * f[j + 1]
        dF = F1 - F0
        R = T - F0
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(dF > 0.0, R / dF, 0.5)
            s = np.where(s > 1.0, 1.0, s)
            s = np.where(s < 0.0, 0.0, s)
            c2 = (3.0 * dF - 2.0 * m0) - m1
            c3 = (m0 + m1) - 2.0 * dF
            for _ in range(NEWTON):
                r = (m0 + s * (c2 + s * c3)) * s - R
                dp = m0 + s * (2.0 * c2 + (3.0 * c3) * s)
                s = np.where(dp > 0.0, s - r / dp, s)
                s = np.where(s > 1.0, 1.0, s)
                s = np.where(s < 0.0, 0.0, s)
        return tab["tL"] + h * (j.astype(np.float64) + s)

    def at(self, tab, t):
        """x, 1 - x and the marginal score at logit-space points t"""
        st = tab["st"]
        _, _, x, y, L, ld, at = self.point(st, t)
        pos = np.asarray(t) >= 0
        nL = 0.0 - L
        naL = (0.0 - at) - L
        lx = np.where(pos, nL, naL)
        ly = np.where(pos, naL, nL)
        ldx = ld - L
        ll = (((st.am1 * lx + st.bm1 * ly) - st.n * ldx) + st.lg_sum) - st.lg_each
        return x, y, ll

    def icdf(self, tab, probs):
        """{x, 1 - x} at the inverse CDF of every probability"""
        p = np.asarray(probs, np.float64)
        x, y, _ = self.at(tab, self.invert(tab, p * tab["Z"]))
        return np.stack([x, y], axis=1)

    def summary(self, tab, confidence_level=0.95):
        """miso_batch_get_exact_summary: (mean, ci_low, ci_high), two values each"""
        alpha = np.float64(1.0) - np.float64(confidence_level)
        q = self.icdf(tab, [alpha / 2, 1 - alpha / 2])
        return (np.array([tab["mean0"], tab["mean1"]]), np.array([q[0, 0], q[1, 1]]), np.array([q[1, 0], q[0, 1]]))

    def words(self, seed, event_id, S):
        key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        return np.array([self.orc.philox((s, 0, SITE_EXACT, event_id), key)[0] for s in range(S)], dtype=np.uint32)

    def draw(self, tab, seed, event_id, S):
        """the event's S sample rows [S, 2] and their log scores"""
        u = (self.words(seed, event_id, S).astype(np.float64) + 0.5) * (1.0 / 4294967296.0)
        x, y, ll = self.at(tab, self.invert(tab, u * tab["Z"]))
        return np.stack([x, y], axis=1), ll

    def assignment(self, psi, seed, event_id, n_draw):
        """the per-read reassignment of the drawing reads from psi = (x, 1 - x): algorithm = MARGINAL's (kernels_marginal.hip)"""
        total = (np.float64(0.0) + psi[0]) + psi[1]
        out = np.zeros(n_draw, np.int32)
        for r in range(n_draw):
            w = self.orc.split_word(seed, event_id, 0, ITER_INIT, r)
            rnd = (np.float64(w) * (1.0 / 4294967296.0)) * total
            out[r] = 0 if rnd < psi[0] else 1
        return out
