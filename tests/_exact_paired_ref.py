"""A fixed-order restatement of the paired-end exact-posterior mode (miso_amd/csrc/kernels_exact_paired.hip with
exact_paired.hpp), in the style of _exact_ref.py, on which it builds: the pair-free part of the
density is that module's `point` with the effective lengths replaced by A = exp(assscores).

Every floating-point operation is one IEEE-754 double operation in the order the kernel makes it; exp / log are the checker
library's orc_det_exp / orc_det_log, the uniforms its Philox.  One shortcut that changes no bit: the log of a block's
product is computed once per DISTINCT block (blocks of sixteen equal pairs repeat in the large cases) and the blocks' logs
are then added in block order, as the kernel adds them.  Test infrastructure only.
"""
import numpy as np

from _exact_ref import DROP, G, LANES, CELLS, T_MODE, SITE_GIBBS, ITER_INIT, Posterior, Stats, fence

BLOCK = 16          # exact_paired.hpp EXP_BLOCK
PASSES = 2          # EXP_PASSES
PASS_PTS = 8        # EXP_PASS_PTS: 512 points per window pass
MIN_PROB = 2.0 ** -63


def eligible(K, A, hyper, any_bad=False):
    """include/miso_amd.h miso_exact_paired_eligible"""
    return K == 2 and fence(A, hyper) and not any_bad


class PairedStats:
    """n10, n01, A0, A1, the hyperparameters and the drawing pairs' (m0, m1) as the kernel holds them"""

    def __init__(self, n10, n01, A0, A1, h0, h1, pairs):
        self.m = np.ascontiguousarray(pairs, dtype=np.float64).reshape(-1, 2)
        self.nd = len(self.m)
        n = (np.float64(n10) + np.float64(n01)) + np.float64(self.nd)
        self.base = Stats(n10, n01, n, A0, A1, h0, h1)
        self.c8 = (n + ((self.base.hm0 + 1.0) + (self.base.hm1 + 1.0))) * np.float64(0.03125)


class PairedPosterior(Posterior):
    def pair_logsum(self, ps, x, y):
        """sum_i log(x m0_i + y m1_i) at the points (x, y): sixteen factors multiplied in pair order from 1.0, one log per
        block, the logs added in block order from 0.0"""
        x = np.asarray(x, np.float64)
        y = np.asarray(y, np.float64)
        P = np.zeros(x.shape)
        memo = {}
        for b0 in range(0, ps.nd, BLOCK):
            blk = ps.m[b0:b0 + BLOCK]
            key = blk.tobytes()
            if key not in memo:
                pr = np.ones(x.shape)
                for m0, m1 in blk:
                    pr = pr * (x * m0 + y * m1)
                memo[key] = self.log(pr)
            P = P + memo[key]
        return P

    def eval(self, ps, t):
        g, _, x, y, _, _, _ = self.point(ps.base, t)
        return g + self.pair_logsum(ps, x, y), x, y

    def window(self, ps):
        f64 = np.float64
        lo, hi = f64(-T_MODE), f64(T_MODE)
        npts = LANES * PASS_PTS
        idx = np.arange(npts, dtype=np.float64)
        gref = f64(0.0)
        for _ in range(PASSES):
            d = (hi - lo) / f64(npts - 1)
            g, _, _ = self.eval(ps, lo + d * idx)
            gm = g.max()
            thr = gm - (f64(DROP) + ps.c8 * (d * d))
            keep = np.nonzero(g >= thr)[0]
            first, last = int(keep[0]), int(keep[-1])
            nlo = lo if first <= 0 else lo + d * f64(first - 1)
            nhi = hi if last >= npts - 1 else lo + d * f64(last + 1)
            lo, hi, gref = nlo, nhi, gm
        return lo, hi, gref

    def tabulate(self, ps):
        f64 = np.float64
        tL, tR, gref = self.window(ps)
        h = (tR - tL) / f64(G)
        h24 = h / f64(24.0)
        t = tL + h * np.arange(-1, G + 2, dtype=np.float64)       # the points -1 .. G + 1
        g, x, y = self.eval(ps, t)
        fe = self.exp(g - gref)
        f, x, y = fe[1:-1], x[1:-1], y[1:-1]
        cell = h24 * ((13.0 * (fe[1:-2] + fe[2:-1]) - fe[:-3]) - fe[3:])
        cell = np.where(cell < 0.0, 0.0, cell)
        F = np.zeros(G + 1)
        off = f64(0.0)
        for l in range(LANES):
            acc = f64(0.0)
            loc = np.zeros(CELLS)
            for j in range(CELLS):
                acc = acc + cell[CELLS * l + j]
                loc[j] = acc
            F[CELLS * l + 1: CELLS * l + CELLS + 1] = off + loc
            off = off + acc
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
        Z = F[G]
        return dict(st=ps.base, ps=ps, tm=f64(0.5) * (tL + tR), gmax=gref, tL=tL, tR=tR, h=h, f=f, F=F, Z=Z,
                    mean0=sx / sf, mean1=sy / sf, logZ=self.log(Z) + gref)

    def out8(self, tab):
        """what miso_selftest_exact_paired returns per element"""
        return np.array([tab[k] for k in ("mean0", "mean1", "tL", "tR", "Z", "gmax", "h", "logZ")], dtype=np.float64)

    def at(self, tab, t):
        """x, 1 - x and the marginal log density (with the Dirichlet normaliser) at logit-space points t"""
        st, ps = tab["st"], tab["ps"]
        _, _, x, y, L, ld, at = self.point(st, t)
        pos = np.asarray(t) >= 0
        nL = 0.0 - L
        naL = (0.0 - at) - L
        lx = np.where(pos, nL, naL)
        ly = np.where(pos, naL, nL)
        ldx = ld - L
        P = self.pair_logsum(ps, x, y)
        ll = ((((st.am1 * lx + st.bm1 * ly) + P) - st.n * ldx) + st.lg_sum) - st.lg_each
        return x, y, ll

    def assignment(self, tab, psi, seed, event_id):
        """the reassignment of the drawing pairs from psi = (x, 1 - x): the paired pick rule on the words of the paired
        sampler's initial reassignment of chain 0 (kernels_k2.inl pe_pick, gibbs(MISO_ITER_INIT))"""
        ps = tab["ps"]
        key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        out = np.zeros(ps.nd, np.int32)
        blk = None
        for r in range(ps.nd):
            if r % 4 == 0:
                blk = self.orc.philox((r // 4, ITER_INIT, SITE_GIBBS, event_id), key)
            c0 = np.float64(0.0) + psi[0] * ps.m[r, 0]
            T = c0 + psi[1] * ps.m[r, 1]
            rnd = (np.float64(blk[r % 4]) * (1.0 / 4294967296.0)) * T
            out[r] = 0 if rnd < c0 else 1
        return out


# ---- the fragment-length law and the test cases ----

def fragment_dist(mean, var, num_devs=4.0, read_len=36):
    """(start, probabilities) as the library makes them (host.cpp normal_fragment; math.exp is the C library's exp)"""
    import math
    sd = math.sqrt(var)
    start = max(int(mean - sd * num_devs), read_len)
    end = max(int(mean + sd * num_devs), start)
    prob = []
    for i in range(start, end + 1):
        x = (i - mean) / sd
        prob.append(0.398942280401432677939946059934 * math.exp(-0.5 * x * x) / sd)
    total = 0.0
    for v in prob:
        total += v
    scale = 1.0 / total
    return start, np.array([v * scale for v in prob], dtype=np.float64)


def ass_sums(isolen, start, il):
    """A_k = exp(assscores_k) = sum over the fragment lengths of max(isolen_k - length + 1, 0) (overhang 1; miso_paired.c:403-419)"""
    return [float(sum(max(int(L) - start - j + 1, 0) for j in range(il))) for L in isolen]


def _ratio_pairs(n, log_ratio, m_big=0.012):
    import math
    small = m_big * math.exp(-abs(log_ratio))
    return [(m_big, small) if log_ratio >= 0 else (small, m_big)] * n


def synthetic_cases():
    """[(name, n10, n01, A0, A1, pairs)]: the issue's list without the simulated events"""
    rng = np.random.default_rng(17)

    def rnd(n):
        return rng.uniform(1e-5, 0.0133, size=(n, 2))
    return [
        ("no-pairs", 11, 5, 60000.0, 43000.0, []),
        ("one-pair", 3, 4, 60000.0, 43000.0, [(0.011, 0.0004)]),
        ("B-1", 2, 1, 52000.0, 61000.0, rnd(BLOCK - 1)),
        ("B", 2, 1, 52000.0, 61000.0, rnd(BLOCK)),
        ("B+1", 2, 1, 52000.0, 61000.0, rnd(BLOCK + 1)),
        ("m0=m1", 7, 9, 60000.0, 43000.0, [(0.0101, 0.0101)] * 40),
        ("two-mode", 0, 0, float(np.exp(6.0)), 1.0, _ratio_pairs(6, 4.5)),
        ("two-mode-mirrored", 0, 0, 1.0, float(np.exp(6.0)), _ratio_pairs(6, -4.5)),
        ("50000+50000", 30000, 20000, 60000.0, 43000.0, [(0.012, 0.004)] * 50000),
        ("3-0-A50-1", 3, 0, 50.0, 1.0, []),
    ]


def simulated_case(orc, n_pairs, seed=11, mean=250.0, var=900.0, read_len=36):
    """a simulate_pe event as (n10, n01, A0, A1, pairs) with what is needed to run the samplers on it"""
    from _problems import simulate_pe
    exons, isoforms, g, pos, cig = simulate_pe(orc, 2, n_pairs, read_len=read_len, mean=mean, var=var, seed=seed)
    rc, match, fl = orc.match_iso_paired(g, pos, cig, read_len, mean, var)
    assert rc == 0
    start, prob = fragment_dist(mean, var, 4.0, read_len)
    A = ass_sums(orc.isolength(g), start, len(prob))
    both = (match[:, 0] > 0) & (match[:, 1] > 0)
    n10 = int(((match[:, 0] > 0) & ~both).sum())
    n01 = int(((match[:, 1] > 0) & ~both).sum())
    pairs = np.stack([prob[fl[both, 0] - start], prob[fl[both, 1] - start]], axis=1)
    assert np.allclose(pairs, match[both], rtol=1e-12, atol=0)
    return dict(n10=n10, n01=n01, A=A, pairs=pairs, exons=exons, isoforms=isoforms, g=g, pos=pos, cig=cig,
                match=match, fraglen=fl)
