"""Independent statements of the aerosol forcing rows (include/fiveeq.h "AEROSOL FORCING ROWS"), written from the header comment
and not from fiveeqscm_amd.aerosols.aerosol_rows_host, and the cases the CPU and GPU tests share:

  rows_scalar(...)  one member at a time in plain Python floats (IEEE doubles: every +, -, *, / is one rounding, Python never
                    fuses), fp32 rows rounded once through struct; the logarithm comes from the caller (`log`, a function of one
                    float), so that a correctly rounded stand-in (math.sqrt against np.sqrt) makes the comparison with the NumPy
                    twin exact whatever the two libraries' logarithms do in their last bit;
  rows_mp(...)      the formula in 50 digits (mpmath) on the given binary values, nothing rounded on the way;
  error_bound(...)  the absolute rounding-error bound of the fp64 operation list, derived below;
  case(...)         emissions, base and per-member parameters with the member classes the issue names in the edge lanes.

THE BOUND.  u = 2^-53 (every listed operation is within 0.5 ulp: a relative error <= u), gamma_j = j u / (1 - j u).
Linear term, A = sum_k |ari_k| |E_k - base_k|:  e = fl(E_k - base_k) and p = fl(ari_k e) carry (1 + u)^2, the K ordered adds
one more u each on a partial sum of magnitude <= A:            err_lin <= gamma_{K+2} A.
Cloud term: g = fl(1 / s) and p = fl(g E_k) carry (1 + u)^2, the ordered adds of the nonnegative p one u each, y = fl(1 + x)
one more: |y^ - y| <= gamma_{K+3} y, so the logarithm's ARGUMENT moves ln y by <= gamma_{K+3} / (1 - gamma_{K+3}); the
logarithm itself is within c ulp of ln y^ — an absolute 2 c u |ln y^| (ulp(L) <= 2 u |L|) — with c = 1 for np.log and c = 2
for the device's pinned fe_log.  Both y and y0:
    err_L + err_L0 <= 2 gamma_{K+3}' + 2 c u (|ln y| + |ln y0| + 2 gamma_{K+3}')         (gamma' = gamma / (1 - gamma))
v = fl(L - L0) adds u |v^|, w = fl(beta v) adds u |w^|, acc = fl(acc - w) adds u |F^|.  With |v^| <= |ln y - ln y0| + err_L +
err_L0 =: V:
    |F^ - F| <= gamma_{K+2} A + |beta| (1 + u) (err_L + err_L0 + u V) + u |beta| V (1 + u) + u (|F| + everything above).
error_bound returns this sum times 1.001 (the second-order products of the terms above, all below 1e-14 of it).
"""
import math
import struct

import numpy as np

U = 2.0 ** -53
N_ROWS = 12
ZERO_ROW = 6                       # a step without emissions: y == 1.0 exactly


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def rows_scalar(E, base, ari, shape, beta, in_aci, log=math.log, start=None, f32=False, cuts=()):
    """E [n_steps][K], base [K], ari / shape [K][n], beta [n], in_aci [K] booleans, start [n_steps][n] or None (what the rows hold
    before an accumulating call).  f32: ari, shape and beta are taken as fp32 values and each row value is rounded to fp32 at its
    store.  cuts: steps at which the run is cut into calls — each call recomputes g and L0 (the same bits), so this only walks
    the steps in pieces.  Returns rows [n_steps][n] as lists of Python floats."""
    n_steps, K, n = len(E), len(base), len(ari[0])
    rows = [[0.0] * n for _ in range(n_steps)]
    edges = [0] + sorted(cuts) + [n_steps]
    cloud = [k for k in range(K) if in_aci[k]]
    q = (lambda v: float(_f32(v))) if f32 else float
    for m in range(n):
        a = [q(ari[k][m]) for k in range(K)]
        for lo_, hi_ in zip(edges[:-1], edges[1:]):
            if cloud:
                bt = q(beta[m])
                g = {k: 1.0 / q(shape[k][m]) for k in cloud}
                x = 0.0
                for k in cloud:
                    p = g[k] * float(base[k])
                    x = x + p
                y0 = 1.0 + x
                L0 = log(y0)
            for t in range(lo_, hi_):
                acc = 0.0 if start is None else float(start[t][m])
                for k in range(K):
                    e = float(E[t][k]) - float(base[k])
                    p = a[k] * e
                    acc = acc + p
                if cloud:
                    x = 0.0
                    for k in cloud:
                        p = g[k] * float(E[t][k])
                        x = x + p
                    y = 1.0 + x
                    L = log(y)
                    v = L - L0
                    w = bt * v
                    acc = acc - w
                rows[t][m] = _f32(acc) if f32 else acc
    return rows


def rows_mp(E, base, ari, shape, beta, in_aci):
    """The rows [n_steps][n] as mpmath numbers at 50 digits on the given (binary) values of every input."""
    import mpmath as mp
    n_steps, K, n = len(E), len(base), len(ari[0])
    cloud = [k for k in range(K) if in_aci[k]]
    out = [[None] * n for _ in range(n_steps)]
    with mp.workdps(50):
        for m in range(n):
            L0 = mp.log(1 + sum(mp.mpf(float(base[k])) / mp.mpf(float(shape[k][m])) for k in cloud)) if cloud else mp.mpf(0)
            for t in range(n_steps):
                F = mp.mpf(0)
                for k in range(K):
                    F += mp.mpf(float(ari[k][m])) * (mp.mpf(float(E[t][k])) - mp.mpf(float(base[k])))
                if cloud:
                    L = mp.log(1 + sum(mp.mpf(float(E[t][k])) / mp.mpf(float(shape[k][m])) for k in cloud))
                    F -= mp.mpf(float(beta[m])) * (L - L0)
                out[t][m] = F
    return out


def error_bound(E_t, base, ari_m, shape_m, beta_m, in_aci, log_ulps):
    """The bound of the module docstring for one step's emission record E_t [K] and one member's parameters, in plain floats
    (the quantities it is made of are evaluated in fp64: their own rounding is covered by the 1.001)."""
    K = len(base)
    gam = lambda j: j * U / (1.0 - j * U)                                              # noqa: E731
    A = sum(abs(float(ari_m[k])) * abs(float(E_t[k]) - float(base[k])) for k in range(K))
    F = sum(float(ari_m[k]) * (float(E_t[k]) - float(base[k])) for k in range(K))
    bound = gam(K + 2) * A
    cloud = [k for k in range(K) if in_aci[k]]
    if cloud:
        ly = math.log1p(sum(float(E_t[k]) / float(shape_m[k]) for k in cloud))
        ly0 = math.log1p(sum(float(base[k]) / float(shape_m[k]) for k in cloud))
        g3 = gam(K + 3) / (1.0 - gam(K + 3))
        err_L = 2.0 * g3 + 2.0 * log_ulps * U * (abs(ly) + abs(ly0) + 2.0 * g3)
        V = abs(ly - ly0) + err_L
        b = abs(float(beta_m))
        bound += b * (1.0 + U) * (err_L + U * V) + U * b * V * (1.0 + U)
        F -= float(beta_m) * (ly - ly0)
    bound += U * (abs(F) + bound)
    return 1.001 * bound


# ---- the shared cases -------------------------------------------------------------------------------------------------------
def masks(K):
    """The aci masks of the issue for K species as lists of booleans: none, all, one bit that is not bit 0, alternating bits
    (K = 1 has only the first two)."""
    out = [0, (1 << K) - 1]
    if K > 1:
        out += [1 << (K - 1), 0x55 & ((1 << K) - 1)]
    return [[bool(mask >> k & 1) for k in range(K)] for mask in dict.fromkeys(out)]


def edge_lanes(n):
    return sorted({m for m in (0, 63, 64, n - 1) if 0 <= m < n})


S_CLASSES = ("huge", "straddle", "tiny")          # y - 1 < 1e-9;  y on both sides of sqrt(2) and of 2;  y > 1e6
B_CLASSES = ("zero", "negative", "positive")      # beta = 0;  beta < 0;  an ordinary beta (and, with it, an ari column of zeros)


def case(K, n, in_aci, base_zero, rot=0, seed=0, with_classes=True):
    """(E [N_ROWS, K], base [K], ari [K, n], shape [K, n], beta [n], classes {lane: (s class, beta class)}).  Emissions ramp up
    over the rows (a factor ~14) with a row of zeros at ZERO_ROW; base is 0 or a third of the first row.  The edge lanes 0, 63,
    64 and n - 1 take the classes in turn — lane i of them class (i + rot) % 3 of S_CLASSES and of B_CLASSES, so rot = 0, 1, 2
    shows every lane every class — and for n > 8 lanes 1..3 hold the three classes too.  The shape classes are written over the
    species of in_aci: `huge` s = 1e13, `straddle` s = max_t X_t / 1.3 (X_t the masked emission sum: x runs from ~0.1 to 1.3),
    `tiny` s = max_t X_t / 1e7.  The last species has an ari row of zeros for K >= 3.  with_classes=False: ordinary members only
    (rows of a few tenths of a W m-2, for a run through the engine)."""
    rng = np.random.default_rng(1000 * K + n + 7 * seed)
    t = np.arange(N_ROWS)[:, None]
    amp = rng.uniform(0.5, 30.0, (1, K))
    E = amp * (0.08 + t / (N_ROWS - 1.0)) * rng.uniform(0.9, 1.1, (N_ROWS, K))
    E[ZERO_ROW] = 0.0
    base = np.zeros(K) if base_zero else E[0] / 3.0
    ari = -rng.uniform(0.002, 0.05, (K, 1)) / amp.T * rng.uniform(0.5, 1.5, (K, n))
    ari[::2] *= -1.0 if K > 1 else 1.0                                                  # both signs (BC warms, SO2 cools)
    if K >= 3:
        ari[K - 1] = 0.0
    shape = amp.T * rng.uniform(0.5, 20.0, (K, n))
    beta = rng.uniform(0.3, 1.5, n)
    X = E[:, [k for k in range(K) if in_aci[k]]].sum(1).max() if any(in_aci) else 1.0
    s_of = {"huge": 1e13, "straddle": X / 1.3, "tiny": X / 1e7}
    lanes = {m: (i + rot) % 3 for i, m in enumerate(edge_lanes(n))} if with_classes else {}
    if n > 8 and with_classes:
        lanes.update({1: 0, 2: 1, 3: 2})
    classes = {}
    for m, c in lanes.items():
        classes[m] = (S_CLASSES[c], B_CLASSES[c])
        for k in range(K):
            if in_aci[k]:
                shape[k, m] = s_of[S_CLASSES[c]]
        beta[m] = {"zero": 0.0, "negative": -0.8, "positive": 1.1}[B_CLASSES[c]]
        if B_CLASSES[c] == "positive":
            ari[:, m] = 0.0
    return E, base, ari, shape, beta, classes
