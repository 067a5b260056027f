"""CPU references for the chain diagnostics (miso_batch_diagnose, miso_amd/csrc/kernels_diagnose.hip).

* ``diag_fixed``  the device's order of operations restated in numpy, operation for operation: equal to the kernel's
                  outputs bit for bit (tests/test_gpu_diagnostics.py).
* ``diag_exact``  the definitions evaluated in exact rational arithmetic (fractions.Fraction); only the final square
                  roots, the division N / tau and the floor 1 / log10(N) are floats.  It also reports how far every
                  decision of Geyer's truncation was from its threshold.
* ``error_bound`` how far the first may be from the second, from the operation counts (tests/test_diag_ref.py).

The square roots: miso_det_sqrt equals the IEEE square root bit for bit (tests/test_detmath.py
test_sqrt_is_correctly_rounded), so math.sqrt restates it.
"""
import math
from fractions import Fraction

import numpy as np

NAN4 = (math.nan, math.nan, math.nan, 0)
U = 2.0 ** -53


def shape(S, C):
    """(n, h, M, N) of S sample columns from C chains."""
    n = S // C
    h = n // 2
    return n, h, 2 * C, 2 * C * h


def sequences(x, C):
    """The M = 2 C split sequences [M, h] of a column: j = 2 c + half."""
    x = np.asarray(x, dtype=np.float64)
    n, h, M, _ = shape(len(x), C)
    per_chain = x[:n * C].reshape(n, C)
    out = np.empty((M, h))
    for c in range(C):
        out[2 * c] = per_chain[:h, c]
        out[2 * c + 1] = per_chain[n - h:, c]
    return out


def _wavesum(u):
    """The kernel's wave sum: lane l adds u[l], u[l + 64], ... in order onto +0.0 (an absent term as +0.0, which changes
    nothing: a partial sum is never -0.0), then the tree p[l] += p[l + off], off = 32 .. 1."""
    q = max(1, -(-len(u) // 64))
    pad = np.zeros(q * 64)
    pad[:len(u)] = u
    p = np.zeros(64)
    for row in pad.reshape(q, 64):
        p = p + row
    off = 32
    while off >= 1:
        p[:off] = p[:off] + p[off:2 * off]
        off >>= 1
    return float(p[0])


def _seqsum(v):
    s = 0.0
    for a in v:
        s = s + a
    return s


def diag_fixed(x, C):
    """(rhat, ess, mcse, lag) of one column in the device's order of operations."""
    with np.errstate(all="ignore"):
        seq = sequences(x, C)
        M, h = seq.shape
        N = M * h
        if h < 4:
            raise ValueError("Too few samples per chain for diagnostics")
        m, s2, d = [], [], np.empty_like(seq)
        for j in range(M):
            mj = _wavesum(seq[j]) / float(h)
            d[j] = seq[j] - mj
            m.append(mj)
            s2.append(_wavesum(d[j] * d[j]) / float(h - 1))
        W = _seqsum(s2) / float(M)
        mm = _seqsum(m) / float(M)
        Bh = _seqsum([(a - mm) * (a - mm) for a in m]) / float(M - 1)
        V = (W * float(h - 1)) / float(h) + Bh
        if not (W > 0.0 and math.isfinite(V)):
            return NAN4

        def rho(t):
            A = _seqsum([_wavesum(d[j, :h - t] * d[j, t:]) / float(h) for j in range(M)]) / float(M)
            return 1.0 - (W - A) / V

        sumP, prev, pairs, k = 0.0, 0.0, 0, 0
        while True:
            P = (1.0 if k == 0 else rho(2 * k)) + rho(2 * k + 1)
            taken = True
            if k >= 1:
                taken = P > 0.0
                if taken:
                    P = P if P < prev else prev
            if taken:
                sumP = sumP + P
                prev = P
                pairs += 1
            if not (taken and 2 * (k + 1) + 1 <= h - 1):
                break
            k += 1
        tau = -1.0 + 2.0 * sumP
        floor_tau = 1.0 / math.log10(float(N))
        tau = tau if tau > floor_tau else floor_tau
        ess = float(N) / tau
        return math.sqrt(V / W), ess, math.sqrt(V / ess), 2 * pairs


def diag_exact(x, C):
    """The definitions in exact arithmetic.  Returns a dict: rhat, ess, mcse, lag; W, V, tau (floats of the exact values);
    margins: |P_k| of every evaluated pair k >= 1 and |P_k - P_{k-1}| of every monotone comparison made; pairs: the pairs
    taken.  For finite, non-degenerate columns."""
    seq = sequences(x, C)
    M, h = seq.shape
    N = M * h
    F = [[Fraction(float(v)) for v in row] for row in seq]
    m = [sum(r) / h for r in F]
    d = [[v - mj for v in r] for r, mj in zip(F, m)]
    s2 = [sum(v * v for v in r) / (h - 1) for r in d]
    W = sum(s2) / M
    mm = sum(m) / M
    Bh = sum((a - mm) ** 2 for a in m) / (M - 1)
    V = W * (h - 1) / h + Bh

    def rho(t):
        A = sum(sum(r[i] * r[i + t] for i in range(h - t)) / h for r in d) / M
        return 1 - (W - A) / V

    margins = []
    sumP, prev, pairs, k = Fraction(0), None, 0, 0
    while True:
        P = (1 if k == 0 else rho(2 * k)) + rho(2 * k + 1)
        taken = True
        if k >= 1:
            margins.append(abs(float(P)))
            taken = P > 0
            if taken:
                margins.append(abs(float(P - prev)))
                P = min(P, prev)
        if taken:
            sumP += P
            prev = P
            pairs += 1
        if not (taken and 2 * (k + 1) + 1 <= h - 1):
            break
        k += 1
    tau = max(float(-1 + 2 * sumP), 1.0 / math.log10(float(N)))
    ess = float(N) / tau
    return {"rhat": math.sqrt(float(V / W)), "ess": ess, "mcse": math.sqrt(float(V) / ess), "lag": 2 * pairs,
            "W": float(W), "V": float(V), "tau": tau, "pairs": pairs, "margins": margins}


def error_bound(x, C, pairs):
    """First-order bounds on |diag_fixed - diag_exact| for (rhat, ess, mcse), relative, given that both take the same
    `pairs` pairs.  u = 2^-53; X = max |x|, D = max |d| <= 2 X; g = ceil(h / 64) + 6 additions on the longest path of a
    wave sum (strided partials, then six tree levels).

      m_j       g additions and a division of terms bounded by X:          |dm|  <= (g + 1) u X
      d_j,i     the error of m_j and one rounding:                         |dd|  <= (g + 1) u X + u D  =: e_d
      a_j(t)    h products with two perturbed factors and one rounding each, summed (g) and divided:
                                                                           |da|  <= 2 D e_d + (g + 2) u D^2  =: e_a
      s2_j      the same sum over h - 1:                                   |ds2| <= e_a h / (h - 1)
      W, A_t    M additions and a division of M such terms:                |dW|  <= e_a h / (h - 1) + (M + 1) u W,
                                                                           |dA|  <= e_a + (M + 1) u W     (|A_t| <= W)
      Bh        M terms (m_j - mm)^2, each factor off by 2 |dm| + u R (R = max |m_j - mm| <= 2 X), M additions, a division:
                                                                           |dB|  <= (2 R (2 (g + 1) u X + u R) + (M + 3) u R^2) M / (M - 1)
      V         a product, a division, an addition:                        |dV|  <= |dW| + |dB| + 3 u V
      rho_t     1 - (W - A) / V, |W - A| <= 2 W <= 2 V h / (h - 1):        |dr|  <= (|dW| + |dA| + u 2 W) / V + 3 (|dV| / V + 2 u) + u
                (this is the cancellation: the absolute error of rho is the RELATIVE error of W - A against V)
      P_k       two rho and an addition:                                   |dP|  <= 2 |dr| + 2 u
      tau       `pairs` terms P <= 2 summed, doubled, minus one:           |dt|  <= 2 pairs (|dP| + 2 pairs u) + 4 pairs u + u
      ess       N / tau:   relative |dt| / tau + u  (tau >= 1 / log10 N; where the floor holds tau, its own rounding is u)
      mcse      sqrt(V / ess):   relative (|dV| / V + ess_rel) / 2 + 2 u
      rhat      sqrt(V / W):     relative (|dV| / V + |dW| / W) / 2 + 2 u

    Everything is first order in u; the returned bounds are doubled for the second-order terms."""
    seq = sequences(x, C)
    M, h = seq.shape
    ex = diag_exact(x, C)
    W, V, tau = ex["W"], ex["V"], ex["tau"]
    X = float(np.abs(seq).max())
    means = seq.mean(axis=1)
    D = float(np.abs(seq - means[:, None]).max()) * (1 + 1e-9) + 1e-300
    R = float(np.abs(means - means.mean()).max()) * (1 + 1e-9)
    g = -(-h // 64) + 6
    u = U
    e_d = (g + 1) * u * X + u * D
    e_a = 2 * D * e_d + (g + 2) * u * D * D
    dW = e_a * h / (h - 1) + (M + 1) * u * W
    dA = e_a + (M + 1) * u * W
    dB = (2 * R * (2 * (g + 1) * u * X + u * R) + (M + 3) * u * R * R) * M / (M - 1)
    dV = dW + dB + 3 * u * V
    dr = (dW + dA + 2 * u * W) / V + 3 * (dV / V + 2 * u) + u
    dP = 2 * dr + 2 * u
    dt = 2 * pairs * (dP + 2 * pairs * u) + 4 * pairs * u + u
    ess_rel = dt / tau + u
    mcse_rel = (dV / V + ess_rel) / 2 + 2 * u
    rhat_rel = (dV / V + dW / W) / 2 + 2 * u
    return {"rhat": 2 * rhat_rel, "ess": 2 * ess_rel, "mcse": 2 * mcse_rel, "dP": 2 * dP}


def ar1(rng, phi, chains, draws, mean=0.5, sd=0.05):
    """`chains` stationary AR(1) chains of `draws` draws as a sample column: draw i of chain c at i * chains + c."""
    e = rng.standard_normal((draws, chains))
    z = np.empty((draws, chains))
    z[0] = e[0]
    s = math.sqrt(1.0 - phi * phi)
    for i in range(1, draws):
        z[i] = phi * z[i - 1] + s * e[i]
    return (mean + sd * z).reshape(-1)
