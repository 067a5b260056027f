"""A fixed-order restatement of the quantiles of delta psi = psi_1 - psi_2 from the exact CDF (miso_amd/csrc/exact_delta.hpp
with kernels_exact_delta.hip and kernels_exact_paired_delta.hip), built on the restatements of the two
exact comparisons: every operation is one IEEE-754 double operation in the kernels' order, so the device's results can be
compared with these bit for bit (tests/test_gpu_exact_delta.py, tests/test_gpu_exact_paired_delta.py) and these with mpmath
(tests/test_exact_delta_ref.py).  Test infrastructure only: nothing under miso_amd/ imports it.
"""
import numpy as np

from _exact_ref import G, Stats
from _exact_compare_ref import lane_sum, table_cdf, window
from _exact_paired_compare_ref import PairedCompare  # noqa: F401  (the paired side's posterior: callers pass one in)

ROUNDS = 5          # EXACT_DELTA_ROUNDS
PTS = 8             # EXACT_DELTA_PTS
PROBS = (0.5, 0.025, 0.975)


class DeltaCdf:
    """H(z) = P(psi_1 - psi_2 <= z) of one pair as the kernels' sweep makes it: A's tabulated posterior (the narrower window
    in psi), its weights wf = w f_A, B's table"""

    def __init__(self, post, A, B, a_is_2, f_A):
        t = A["tL"] + A["h"] * np.arange(G + 1, dtype=np.float64)
        pt = post.point(A["st"], t)
        self.x, self.y = pt[2], pt[3]
        wgt = np.ones(G + 1)
        wgt[0] = wgt[G] = 0.5
        self.wf = wgt * (post.exp(pt[0] - A["gmax"]) if f_A is None else f_A)
        self.sf = lane_sum(self.wf)
        self.A, self.B, self.a_is_2 = A, B, a_is_2
        self.tabs = (B, A) if a_is_2 else (A, B)        # sample 1's table, sample 2's
        self.evaluations = 0
        self._seen = {}

    def __call__(self, z):
        z = np.float64(z)
        key = z.tobytes()
        if key not in self._seen:
            self.evaluations += 1
            if self.a_is_2:     # H = sum w F_1(y + z) / Z_1
                val = table_cdf(self.B, self.x + z, self.y - z)
            else:               # H = 1 - sum w F_2(x - z) / Z_2
                val = table_cdf(self.B, self.x - z, self.y + z)
            s = lane_sum(self.wf * (val / self.B["Z"])) / self.sf
            self._seen[key] = s if self.a_is_2 else np.float64(1.0) - s
        return self._seen[key]


def single_cdf(post, r1, r2):
    """the CDF of one single-end pair, rows as _exact_compare_ref.pair_rows gives them"""
    st = [Stats(*r1), Stats(*r2)]
    w1, w2 = window(post, st[0])[4], window(post, st[1])[4]
    a_is_2 = bool(w2 < w1)       # A: the narrower window in psi, a tie goes to sample 1
    tabs = [post.tabulate(s) for s in st]
    for tb in tabs:
        tb["post"] = post
    A, B = (tabs[1], tabs[0]) if a_is_2 else (tabs[0], tabs[1])
    return DeltaCdf(post, A, B, a_is_2, None)       # (A's f made again from its points)


def paired_cdf(pc, ps1, ps2):
    """the CDF of one paired-end pair (pc: a PairedCompare; ps: _exact_paired_compare_ref.paired_stats)"""
    tabs = [pc.tabulate(ps1), pc.tabulate(ps2)]
    w1, w2 = (pc.point(tb["st"], tb["tR"])[2] - pc.point(tb["st"], tb["tL"])[2] for tb in tabs)
    a_is_2 = bool(w2 < w1)
    for tb in tabs:
        tb["post"] = pc
    A, B = (tabs[1], tabs[0]) if a_is_2 else (tabs[0], tabs[1])
    return DeltaCdf(pc, A, B, a_is_2, A["f"])       # (A's own f, kept from its table)


def points(b):
    """exact_delta_points: lo + j (hi - lo) / 9, j = 1 .. 8"""
    lo, _, hi, _ = b
    step = (hi - lo) / np.float64(PTS + 1)
    return [lo + np.float64(j) * step for j in range(1, PTS + 1)]


def update(b, z, H, p):
    """exact_delta_update: the smallest j with H_j >= p closes the bracket from above, the point before it from below"""
    lo, Hlo, hi, Hhi = b
    for zj, Hj in zip(z, H):
        if Hj >= p:
            hi, Hhi = zj, Hj
            break
        lo, Hlo = zj, Hj
    return lo, Hlo, hi, Hhi


def search(H, probs=PROBS, rounds=ROUNDS):
    """exact_delta_search: [q(p) for p in probs] + [H(0.0)]"""
    f = np.float64
    H0 = H(f(0.0))
    whole = (f(-1.0), f(0.0), f(1.0), f(1.0))
    z1 = points(whole)
    H1 = [H(z) for z in z1]
    out = []
    for p in probs:
        p = f(p)
        b = update(whole, z1, H1, p)
        for _ in range(1, rounds):
            z = points(b)
            b = update(b, z, [H(zz) for zz in z], p)
        lo, Hlo, hi, Hhi = b
        assert Hlo < p <= Hhi
        out.append(lo + (hi - lo) * ((p - Hlo) / (Hhi - Hlo)))
    return np.array(out + [H0], dtype=np.float64)


def delta_quantiles(post, r1, r2, probs=PROBS, rounds=ROUNDS):
    """what exact_delta_quantiles reports of one comparable single-end pair: [q(p) ..., H(0.0)]"""
    return search(single_cdf(post, r1, r2), probs, rounds)


def paired_delta_quantiles(pc, ps1, ps2, probs=PROBS, rounds=ROUNDS):
    """what exact_paired_delta_quantiles reports of one pair: [q(p) ..., H(0.0)]"""
    return search(paired_cdf(pc, ps1, ps2), probs, rounds)
