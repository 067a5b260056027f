"""The posterior predictive model check (include/miso_model_check.h) restated in Python, operation by
operation: the word stream, BINV and BTRS as include/miso_binomial.h has them, the chain of binomials, the Freeman-Tukey
discrepancy, the counts and the order of the double sums (every thread of 256 its own rows ascending, then the partial
sums folded in halves).  Python floats are IEEE doubles and nothing here contracts, so the device must agree bit for bit.
It uses what the CPU checker already exposes and nothing else: OrcLib.philox, orc_det_log / exp / sqrt, OrcLib.logfact."""
import math

import numpy as np
from scipy import stats

SITE_FIT = 6
BLOCK = 256
INF = float("inf")
NAN = float("nan")


def fdiv(a, b):
    """a / b as C divides doubles (no exception at b == 0)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


class Math:
    """the checker's deterministic transcendentals as plain callables"""

    def __init__(self, orc):
        self.orc = orc
        L = orc.lib
        self.log = lambda x: float(L.orc_det_log(float(x)))
        self.exp = lambda x: float(L.orc_det_exp(float(x)))
        self.sqrt = lambda x: float(L.orc_det_sqrt(float(x)))


class Stream:
    """miso_ustream: words 0, 1, 2, ... of (seed, event_id, chain, iteration, site), four per Philox block"""

    def __init__(self, orc, seed, event_id, chain, iteration, site):
        self.orc = orc
        self.key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        self.ctr = (iteration & 0xFFFFFFFF, (site | (chain << 8)) & 0xFFFFFFFF, event_id & 0xFFFFFFFF)
        self.next = 0
        self.block = None

    def u01(self):
        i = self.next & 3
        if i == 0:
            self.block = self.orc.philox((self.next >> 2,) + self.ctr, self.key)
        self.next += 1
        return float(int(self.block[i])) * (1.0 / 4294967296.0)


def binomial_inversion(M, s, n, r):
    q = 1.0 - r
    qn = M.exp(float(n) * M.log(q))
    np_ = float(n) * r
    bound = np_ + 10.0 * M.sqrt(np_ * q + 1.0)
    x = 0
    P, U = qn, s.u01()
    guard = 0
    if bound > float(n):
        bound = float(n)
    while U > P:
        x += 1
        if float(x) > bound:
            guard += 1
            if guard > 64:
                return int(np_)
            x, P, U = 0, qn, s.u01()
        else:
            U = (U - P) * (float(x) * q)
            P = P * (float(n - x + 1) * r)
    return x


def binomial_btrs(M, s, n, r, lf, stats=None):
    q, dn = 1.0 - r, float(n)
    spq = M.sqrt(dn * r * q)
    b = 1.15 + 2.53 * spq
    a = -0.0873 + 0.0248 * b + 0.01 * r
    c = dn * r + 0.5
    vr = 0.92 - 4.2 / b
    alpha = (2.83 + 5.1 / b) * spq
    m = float(math.floor((dn + 1.0) * r))
    lpq = M.log(r / q)
    h = lf[int(m)] + lf[n - int(m)]
    for _ in range(4096):
        u = s.u01() - 0.5
        v = s.u01()
        us = 0.5 - abs(u)
        if us == 0.0:            # 2 a / 0 is an infinity: k is no count
            continue
        k = float(math.floor((2.0 * a / us + b) * u + c))
        if not (0.0 <= k <= dn):
            continue
        if us >= 0.07 and v <= vr:
            return int(k)
        if v == 0.0:
            return int(k)
        v = v * alpha / (a / (us * us) + b)
        if M.log(v) <= (h - lf[int(k)] - lf[n - int(k)]) + (k - m) * lpq:
            return int(k)
    return int(m)


def binomial(M, s, n, p, lf, stats=None):
    """miso_binomial; stats (a dict) counts the calls by routine"""
    if n <= 0 or not (p > 0.0):
        return 0
    if p >= 1.0:
        return n
    r = 1.0 - p if p > 0.5 else p
    if float(n) * r < 10.0:
        y = binomial_inversion(M, s, n, r)
        if stats is not None:
            stats["inversion"] = stats.get("inversion", 0) + 1
    else:
        y = binomial_btrs(M, s, n, r, lf)
        if stats is not None:
            stats["btrs"] = stats.get("btrs", 0) + 1
    y = min(max(y, 0), n)
    return n - y if p > 0.5 else y


def weight(pattern, m, psi):
    acc = 0.0
    pattern = int(pattern)
    while pattern:                       # the set bits, lowest first
        low = pattern & -pattern
        acc = acc + float(psi[low.bit_length() - 1])
        pattern ^= low
    return float(m) * acc


def suffix(pattern, m, c, psi):
    C = len(pattern)
    T = weight(pattern[C - 1], m[C - 1], psi)
    for j in range(C - 2, c - 1, -1):
        T = weight(pattern[j], m[j], psi) + T
    return T


def fold(x):
    """256 partial sums folded in halves: x[t] += x[t + h], h = 128, 64, ..., 1"""
    x = np.array(x, dtype=np.float64)
    h = BLOCK // 2
    with np.errstate(all="ignore"):
        while h > 0:
            x[:h] = x[:h] + x[h:2 * h]
            h //= 2
    return float(x[0])


def discrepancy(M, counts, N, p):
    d = 0.0
    for c in range(len(counts)):
        t = M.sqrt(float(counts[c])) - M.sqrt(float(N) * p[c])
        d = d + t * t
    return d


def model_check(orc, pattern, m, n, samples, event_id, seed, lf=None, stats=None):
    """One event.  samples: [S, K].  Returns a dict with the raw call's results (status as the FIT_STATUS name)."""
    M = Math(orc)
    C = len(pattern)
    N = int(sum(int(x) for x in n))
    out = {"status": "ok", "rows": 0, "bad_rows": 0, "exceed": 0, "sum_obs": 0.0, "sum_rep": 0.0,
           "expected": np.zeros(C), "ge": np.zeros(C, np.int32), "le": np.zeros(C, np.int32)}
    samples = np.asarray(samples, dtype=np.float64)
    if C > 64 or (samples.ndim == 2 and samples.shape[1] > 64):
        out["status"] = "too_many_classes"
        return out
    if N == 0:
        out["status"] = "no_reads"
        return out
    if lf is None:
        lf = orc.logfact(N + 1)
    S = samples.shape[0]
    root_n = [M.sqrt(float(x)) for x in n]
    part_obs, part_rep = np.zeros(BLOCK), np.zeros(BLOCK)
    part_p = np.zeros((C, BLOCK))
    rows = bad = exceed = 0
    ge, le = np.zeros(C, np.int64), np.zeros(C, np.int64)
    for s in range(S):                       # thread s % 256 meets its rows in ascending order
        t = s % BLOCK
        psi = samples[s]
        T0 = suffix(pattern, m, 0, psi)
        if not (T0 > 0.0 and T0 < INF):
            bad += 1
            continue
        rows += 1
        st = Stream(orc, seed, event_id, 0, s, SITE_FIT)
        rem = N
        d_obs = d_rep = 0.0
        for c in range(C):
            w = weight(pattern[c], m[c], psi)
            p = fdiv(w, T0)
            root_e = M.sqrt(float(N) * p)
            rep = rem
            if c < C - 1:
                Tc = T0 if c == 0 else suffix(pattern, m, c, psi)
                rep = binomial(M, st, rem, fdiv(w, Tc), lf, stats)
                rem -= rep
            d = root_n[c] - root_e
            d_obs = d_obs + d * d
            d = M.sqrt(float(rep)) - root_e
            d_rep = d_rep + d * d
            part_p[c, t] = part_p[c, t] + p
            ge[c] += rep >= int(n[c])
            le[c] += rep <= int(n[c])
        part_obs[t] = part_obs[t] + d_obs
        part_rep[t] = part_rep[t] + d_rep
        exceed += d_rep >= d_obs
    out["bad_rows"] = bad
    if rows == 0:
        out["status"] = "no_rows"
        return out
    out.update(rows=rows, exceed=int(exceed), sum_obs=fold(part_obs), sum_rep=fold(part_rep), ge=ge.astype(np.int32),
               le=le.astype(np.int32))
    out["expected"] = np.array([fdiv(float(N) * fold(part_p[c]), float(rows)) for c in range(C)])
    return out


# the enumeration case, shared with the device's test: two isoforms, the three classes of a skipped exon, constant rows
ENUM_PATTERN = [2, 1, 3]
ENUM_M = [35, 85, 130]
ENUM_PSI = (0.5, 0.5)
ENUM_N = [2, 1, 3]
ENUM_ROWS = 8192
ENUM_BOUND = 0.028          # >= 5 sqrt(P (1 - P) / 8192) for every P


def enum_exact():
    """(p, exact P(D_rep >= D_obs), exact P(rep_c >= n_c), exact P(rep_c <= n_c), the smallest gap between the observed D
    and another outcome's) by enumeration of the 28 outcomes of Multinomial(6, p), in ordinary double arithmetic."""
    w = np.array([ENUM_M[c] * sum(ENUM_PSI[k] for k in range(2) if (ENUM_PATTERN[c] >> k) & 1) for c in range(3)])
    p = w / w.sum()
    N = sum(ENUM_N)
    D = lambda n: float(((np.sqrt(np.asarray(n, float)) - np.sqrt(N * p)) ** 2).sum())
    d_obs = D(ENUM_N)
    tail, gap = 0.0, np.inf
    for a in range(N + 1):
        for b in range(N + 1 - a):
            o = (a, b, N - a - b)
            if list(o) != ENUM_N:
                gap = min(gap, abs(D(o) - d_obs))
            if D(o) >= d_obs:
                tail += stats.multinomial.pmf(o, N, p)
    ge = [stats.binom.sf(ENUM_N[c] - 1, N, p[c]) for c in range(3)]
    le = [stats.binom.cdf(ENUM_N[c], N, p[c]) for c in range(3)]
    return p, tail, ge, le, gap


def check_enum(r):
    """the assertions of the enumeration case on a result (the restatement's dict or the device's ModelFit as a dict)"""
    _, tail, ge, le, gap = enum_exact()
    assert gap > 1e-9, "another outcome's discrepancy ties with the observed one: a rounding would decide"
    assert r["rows"] == ENUM_ROWS and r["bad_rows"] == 0
    for P in [tail] + ge + le:
        assert 5 * np.sqrt(P * (1 - P) / ENUM_ROWS) <= ENUM_BOUND
    print("exceed/rows", r["exceed"] / ENUM_ROWS, "exact", tail)
    assert abs(r["exceed"] / ENUM_ROWS - tail) <= ENUM_BOUND
    for c in range(3):
        print("class", c, "ge", r["ge"][c] / ENUM_ROWS, ge[c], "le", r["le"][c] / ENUM_ROWS, le[c])
        assert abs(r["ge"][c] / ENUM_ROWS - ge[c]) <= ENUM_BOUND
        assert abs(r["le"][c] / ENUM_ROWS - le[c]) <= ENUM_BOUND
