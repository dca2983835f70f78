"""NumPy restatement of the FORCING ROWS pass of the C ABI (include/fiveeq.h, "FORCING ROWS": fiveeq_forcing_rows_f64 / _f32;
csrc/fiveeq_forcrows.hpp).  Used by the tests only: the package's forcing_rows() has no CPU path.

What the twin is good for, and how far:
  * F and F_gas are WITHIN THE ORACLE TOLERANCE of the kernel's (1e-10 |F| + 1e-13 in fp64), not its bits: the kernel fuses
    the f1 / f3 / scale products into fma and evaluates log and sqrt with its own routines; NumPy rounds each product and calls
    libm.
  * N and H are EXACT GIVEN F: N = F - T / (q0 + q1) is one IEEE addition, one division and one subtraction in the rows'
    precision, H = H + dt * (double)N one product and one addition in fp64 — single IEEE operations, which NumPy performs as the
    kernel does.  imbalance() and heat() fed the DEVICE's F and the stored T give the device's N and H bit for bit.
The replay (S_io of the C ABI) is two nested fma per box and has no exact NumPy form; it is not restated here.
"""
import numpy as np


def gas_forcing(C, C0, f, dtype=np.float64):
    """F_g of one gas from its concentrations C (any shape) in `dtype`: f2 (C - C0), then the f1 log term and the f3 sqrt term,
    each only if its coefficient is not zero, behind the kernel's C > 0 guard (C <= 0 and NaN: no log term, sqrt C reads 0).  The
    constants are the kernel's: 1 / C0 and sqrt C0 computed in fp64 and rounded to `dtype`."""
    dt = np.dtype(dtype).type
    C = np.asarray(C, dtype=dt)
    C0d = float(C0)
    c0, inv_c0, sqrt_c0 = dt(C0d), dt(1.0 / C0d), dt(np.sqrt(C0d))
    f1, f2, f3 = (dt(float(v)) for v in f)
    with np.errstate(invalid="ignore", divide="ignore"):
        pos = C > 0
        Fg = f2 * (C - c0)
        if f1 != 0:
            Fg = np.where(pos, f1 * np.log(np.where(pos, C * inv_c0, dt(1))) + Fg, Fg)
        if f3 != 0:
            Fg = f3 * (np.where(pos, np.sqrt(np.where(pos, C, dt(1))), dt(0)) - sqrt_c0) + Fg
    return Fg.astype(dt)


def total_forcing(F_gas, F_ext_rows, fscale=None, X_rows=None):
    """F [n_rows, N] from F_gas [n_rows, G, N] in the kernel's order: F_ext, then the categories, then the gases.
    F_ext_rows [n_rows]: F_ext of each row's step; X_rows [n_rows, K]: the category record of each row's step; fscale
    [G + K, N] (gas rows first) or None for the plain sum."""
    dt = F_gas.dtype.type
    K_rows, G, N = F_gas.shape
    F = np.repeat(np.asarray(F_ext_rows, dtype=dt).reshape(K_rows, 1), N, axis=1)
    if fscale is not None:
        fs = np.asarray(fscale, dtype=dt)
        for k in range(fs.shape[0] - G):
            F = fs[G + k][None, :] * np.asarray(X_rows, dtype=dt)[:, k:k + 1] + F
    for g in range(G):
        F = (F_gas[:, g] if fscale is None else fs[g][None, :] * F_gas[:, g]) + F
    return F.astype(dt)


def imbalance(F, T, q):
    """N = F - T / (q0 + q1), each operation rounded on its own in the rows' precision: exact given F (module docstring)."""
    dt = F.dtype.type
    q = np.asarray(q, dtype=dt)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (F - np.asarray(T, dtype=dt) / (q[0] + q[1])[None, :]).astype(dt)


def heat(N, dt, heat0=None):
    """H [n_rows, N] fp64: H_k = H_{k-1} + dt * (double)N_k, rows in ascending order, from heat0 [N] (default 0): exact."""
    Nw = np.asarray(N).astype(np.float64)
    H = np.empty_like(Nw)
    run = np.zeros(Nw.shape[1]) if heat0 is None else np.asarray(heat0, dtype=np.float64).copy()
    step = np.float64(dt)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(Nw.shape[0]):
            run = run + step * Nw[k]
            H[k] = run
    return H


def forcing_rows_host(C_rows, steps, params, *, q, F_ext, dt=1.0, T_rows=None, fscale=None, X=None, want=("F",), heat0=None):
    """diagnose.forcing_rows over host arrays, from the functions above: dict with the entries of `want` ("F", "F_gas", "N",
    "H").  C_rows [n_rows, G, N]; F_ext [n_steps]; X [n_steps, K]."""
    C = np.asarray(C_rows)
    dtp = C.dtype.type
    st = np.asarray(steps, dtype=np.int64)
    G = C.shape[1]
    C0 = np.asarray(params["PI_conc"], dtype=np.float64).reshape(G)
    f = np.asarray(params["f"], dtype=np.float64).reshape(G, 3)
    Fg = np.stack([gas_forcing(C[:, g], C0[g], f[g], dtp) for g in range(G)], axis=1)
    Xr = None if X is None else np.asarray(X, dtype=np.float64)[st]
    F = total_forcing(Fg, np.asarray(F_ext, dtype=np.float64)[st], fscale, Xr)
    out = {"F": F, "F_gas": Fg}
    if "N" in want or "H" in want:
        out["N"] = imbalance(F, T_rows, q)
    if "H" in want:
        out["H"] = heat(out["N"], dt, heat0)
    return {k: v for k, v in out.items() if k in want}
