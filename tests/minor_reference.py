"""Independent statements of the minor-gas forcing rows (include/fiveeq.h "MINOR-GAS FORCING ROWS"), written from the header
comment and not from fiveeqscm_amd.minor_gases.minor_gas_rows_host:

  rows_scalar(...)  one member at a time in plain Python floats (IEEE doubles: every +, -, *, / is one rounding, Python never
                    fuses), species in groups of 8, fp32 rows rounded once per group through struct;
  rows_mp(...)      the same recursion in 50 digits (mpmath), unrounded and ungrouped: what the rows approximate.

expm1 comes from the caller (`em1`, per species and member) where the device primitive's bits are wanted; math.expm1 otherwise.
"""
import math
import struct

GROUP = 8


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def rows_scalar(E, c, tau, eff, R0, dt=1.0, em1=None, start=None, f32=False, cuts=()):
    """E [n_steps][K], c [K], tau / eff / R0 / em1 [K][n] (lists or arrays), start [n_steps][n] or None (what the rows hold
    before an accumulating first group).  f32: tau and eff are taken as fp32 values and each group's sum is rounded to fp32
    at its end.  cuts: steps at which the run is cut into calls — each call recomputes em1 and a from tau (the same bits), so
    this only walks the steps in pieces.  Returns (rows [n_steps][n], R [K][n]) as lists of Python floats."""
    n_steps, K, n = len(E), len(c), len(tau[0])
    rows = [[0.0] * n for _ in range(n_steps)]
    R_out = [[0.0] * n for _ in range(K)]
    edges = [0] + sorted(cuts) + [n_steps]
    for m in range(n):
        tk = [float(_f32(tau[k][m]) if f32 else tau[k][m]) for k in range(K)]
        ef = [float(_f32(eff[k][m]) if f32 else eff[k][m]) for k in range(K)]
        R = [float(R0[k][m]) for k in range(K)]
        col = [None if start is None else float(start[t][m]) for t in range(n_steps)]
        for k0 in range(0, K, GROUP):
            group = range(k0, min(k0 + GROUP, K))
            for a_, b_ in zip(edges[:-1], edges[1:]):
                e1 = {k: (math.expm1(-dt / tk[k]) if em1 is None else float(em1[k][m])) for k in group}
                a = {k: tk[k] * float(c[k]) for k in group}
                for t in range(a_, b_):
                    for k in group:
                        u = a[k] * float(E[t][k])
                        v = R[k] - u
                        w = e1[k] * v
                        R[k] = R[k] + w
                    acc = 0.0 if col[t] is None else col[t]
                    for k in group:
                        p = ef[k] * R[k]
                        acc = acc + p
                    col[t] = _f32(acc) if f32 else acc
        for t in range(n_steps):
            rows[t][m] = col[t]
        for k in range(K):
            R_out[k][m] = R[k]
    return rows, R_out


def rows_mp(E, c, tau, eff, R0, dt=1.0):
    """The forcing [n_steps][n] as mpmath numbers at 50 digits: R <- R + expm1(-dt / tau) (R - tau c E), F = sum_k eff_k R_k, on
    the given (binary) values of every input, nothing rounded on the way."""
    import mpmath as mp
    n_steps, K, n = len(E), len(c), len(tau[0])
    out = [[None] * n for _ in range(n_steps)]
    with mp.workdps(50):
        for m in range(n):
            tk = [mp.mpf(float(tau[k][m])) for k in range(K)]
            e1 = [mp.expm1(-mp.mpf(dt) / tk[k]) for k in range(K)]
            R = [mp.mpf(float(R0[k][m])) for k in range(K)]
            for t in range(n_steps):
                F = mp.mpf(0)
                for k in range(K):
                    R[k] = R[k] + e1[k] * (R[k] - tk[k] * mp.mpf(float(c[k])) * mp.mpf(float(E[t][k])))
                    F += mp.mpf(float(eff[k][m])) * R[k]
                out[t][m] = F
    return out
