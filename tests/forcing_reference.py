"""The forcing run (include/fiveeq.h "FORCING SCALES") restated in NumPy from the oracle's step functions: the CPU reference of
tests/test_forcing_*.py and of the forcing leg of smoke().  It shares no code with the kernels."""
import numpy as np

from oracle import fiveeq_oracle as npo


def forcing_numpy(E, params, n_members, forcing, f_scale, fx_scale, F_ext=None, dt=1.0):
    """The forcing run restated in NumPy from the oracle's step functions (alpha_val, step_conc, step_forc, step_temp), all
    members at once: dict(C [n_steps, G, N], T [n_steps, N]).  f_scale [G] or [G, N], fx_scale [K] or [K, N].  forcing: an
    ExternalForcings or its table [n_steps, K]."""
    N = int(n_members)
    X = np.asarray(getattr(forcing, "table", forcing), dtype=np.float64)
    K = X.shape[1]
    drive = npo.make_drive(E, F_ext, dt)
    n_steps = drive.shape[0]
    a = np.atleast_2d(np.asarray(params["a"], float))
    tau = np.atleast_2d(np.asarray(params["tau"], float))
    G = a.shape[0]
    pools = [npo.n_pools_of(a[g]) for g in range(G)]
    ra = np.asarray(params["ra"], float).reshape(G)
    C0 = np.asarray(params["PI_conc"], float).reshape(G)
    c = np.asarray(params["emis2conc"], float).reshape(G)
    f = np.asarray(params["f"], float).reshape(G, 3)
    d = np.asarray(params["d"], float)
    r0, rC, rT = (npo._member_rows(params[k], G, N) for k in ("r0", "rC", "rT"))
    q = npo._member_rows(params["q"], 2, N)
    sg = npo._member_rows(f_scale, G, N)
    sx = npo._member_rows(fx_scale, K, N) if K else np.zeros((0, N))
    g0 = [float(npo.g_0(a[g], tau[g])) for g in range(G)]
    g1 = [float(npo.g_1(a[g], tau[g])) for g in range(G)]
    em1_d = np.expm1(-dt / d)
    R = [np.zeros((pools[g], N)) for g in range(G)]
    S = np.zeros((2, N))
    Cs, Ts = np.empty((n_steps, G, N)), np.empty((n_steps, N))
    for t in range(n_steps):
        T_old = S[0] + S[1]
        F = np.full(N, drive[t, 6])
        for k in range(K):
            F = F + sx[k] * X[t, k]
        for g in range(G):
            G_a = R[g].sum(0) / c[g]
            G_u = drive[t, 3 + g] - G_a
            al = npo.alpha_val(G_u, G_a, T_old, r0[g], rC[g], rT[g], ra[g], g0[g], g1[g], float(params["iirf_max"]))
            R[g], C = npo.step_conc(R[g], al, drive[t, g] * c[g], a[g, :pools[g]], tau[g, :pools[g]], C0[g], dt)
            F = F + sg[g] * npo.step_forc(C, C0[g], f[g])
            Cs[t, g] = C
        S, T = npo.step_temp(S, F, q, em1_d)
        Ts[t] = T
    return {"C": Cs, "T": Ts}
