"""NumPy restatement of the PULSE RESPONSE pass of the C ABI (include/fiveeq.h, "PULSE RESPONSE": fiveeq_pulse_response_f64 /
_f32; csrc/fiveeq_pulse.hpp).  Used by the tests only: the package's pulse_response() has no CPU path.

GIVEN F rows the twin is EXACT: the differences are single fp64 subtractions of exactly widened values and the sums single fp64
additions in row order — IEEE operations NumPy performs as the kernel does.  pulse_sums() fed the DEVICE's F rows and the
stored T and C gives the device's five outputs bit for bit.  pulse_response_host() takes F from
_diagnose_host.total_forcing, which is within the oracle tolerance of the kernel's F, not its bits (see that module).
"""
import numpy as np

from . import _diagnose_host as diag


def pulse_sums(F, T, C, base, pulses, horizons, state=None, row0=0):
    """F, T [S, n_rows, N], C [S, n_rows, G, N] (any float dtype; widened exactly); pulses ((scenario, gas), ...); horizons:
    strictly increasing row counts from the first row of the experiment, row0 of which earlier calls covered; state [3, P, N]
    fp64: the sums before the first row (default 0).  Returns (out [5, P, H, N] fp64 = I_F, I_T, I_C, dT, dC with NaN where the
    rows do not end on the horizon, state [3, P, N] after the last row)."""
    Fw, Tw, Cw = (np.asarray(v).astype(np.float64) for v in (F, T, C))
    K, N = Fw.shape[1], Fw.shape[2]
    P, H = len(pulses), len(horizons)
    out = np.full((5, P, H, N), np.nan)
    run = np.zeros((3, P, N)) if state is None else np.array(state, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            for p, (s, g) in enumerate(pulses):
                d = (Fw[s, k] - Fw[base, k], Tw[s, k] - Tw[base, k], Cw[s, k, g] - Cw[base, k, g])
                for i in range(3):
                    run[i, p] = run[i, p] + d[i]
                for h, n_h in enumerate(horizons):
                    if row0 + k == n_h - 1:
                        out[0:3, p, h] = run[:, p]
                        out[3, p, h], out[4, p, h] = d[1], d[2]
    return out, run


def pulse_response_host(C, T, steps, params, *, F_ext, base, pulses, horizons, fscale=None, X=None, state=None, row0=0):
    """pulse.pulse_response over host arrays: F of every scenario from _diagnose_host (gas_forcing, total_forcing), then
    pulse_sums.  C [S, n_rows, G, N], T [S, n_rows, N]; F_ext [n_steps] or [S, n_steps]; X [S, n_steps, K] with fscale."""
    C = np.asarray(C)
    S, K, G, N = C.shape
    st = np.asarray(steps, dtype=np.int64)
    C0 = np.asarray(params["PI_conc"], dtype=np.float64).reshape(G)
    f = np.asarray(params["f"], dtype=np.float64).reshape(G, 3)
    fe = np.asarray(F_ext, dtype=np.float64)
    fe = np.broadcast_to(fe, (S, fe.shape[-1]))
    F = []
    for s in range(S):
        Fg = np.stack([diag.gas_forcing(C[s, :, g], C0[g], f[g], C.dtype.type) for g in range(G)], axis=1)
        F.append(diag.total_forcing(Fg, fe[s][st], fscale, None if X is None else np.asarray(X, dtype=np.float64)[s][st]))
    return pulse_sums(np.stack(F), T, C, base, pulses, horizons, state, row0)
