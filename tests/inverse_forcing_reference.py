"""The concentration-driven (inverse) step WITH per-member forcing scales: the cases, a NumPy restatement and the 50-digit
anchored step — the references of tests/test_inverse_forcing_cpu.py and tests/test_inverse_forcing_gpu.py.

TEST INFRASTRUCTURE, beside tests/inverse_reference.py (whose cases, target series and units() are used here) and
tests/step_reference.py (whose step_inverse() is the 50-digit step).  It shares no code with the kernels.

    (a) restated_step()    the inverse step with scales, restated in NumPy from the oracle's step functions (alpha_val, step_forc,
                           step_temp): F = F_ext; F += sx_k X[t, k] per category; F += sg_g F_g per gas.
    (b) step_reference()   step_reference.step_inverse evaluated PER MEMBER on the member's own model: its f coefficients are the
                           shared ones times sg_g, its external forcing is F_ext[t] + sum_k sx_k X[t][k], both formed in 50 digits.

CASES: those of inverse_reference for the two layouts that carry the forcing scales — "{4}", "4+1+1", "multigas dt=0.5" and
"co2 dt=1" — each with K = 3 categories.  Gas scales lie in 0.75 .. 1.25 and category scales in 0.25 .. 2, all multiples of
2^-6; table entries are multiples of 2^-10 below 4 in magnitude: every one is exact in fp32, so one reference serves both
precisions.  Member i of an N-member ensemble is member i mod 16 of the case, its scale rows included.

SCALES OF THE ERROR UNITS.  E, cum, R and C keep the scales of step_reference.step_inverse (the gas step does not see the forcing
scales).  The forcing has more terms than the member's own model shows: the reference is handed ONE external forcing, and its
scale counts |F_ext + sum_k sx_k X_k|, where the program under test adds the K + 1 terms one by one and rounds each partial
sum.  So the A part of the pairs sS and sT grows by
    |em1_d_j| |q_j| (|F_ext| + sum_k |sx_k X[t][k]| - |F_ext + sum_k sx_k X[t][k]|)      (>= 0; zero when no term cancels)
per box j — written in _widen_thermal_scales(), next to where the existing pairs are read.  The gas terms need nothing: the
member's model carries f sg, so |sg_g| times the magnitudes of gas g's forcing terms are in the scale already.
"""
import functools

import mpmath as mp
import numpy as np

import inverse_reference as ir
import step_reference as sr
from oracle import fiveeq_oracle as npo

M = ir.M
N_STEPS = ir.N_STEPS
K_CAT = 3
CASES = ("{4}", "4+1+1", "multigas dt=0.5", "co2 dt=1")
OUTPUTS = ir.OUTPUTS
units = ir.units


def _grid(x, bits):
    return np.round(np.asarray(x, dtype=np.float64) * 2.0 ** bits) / 2.0 ** bits


def table(n_steps=N_STEPS):
    """[n_steps, 3], multiples of 2^-10: a negative aerosol-like ramp, volcanic spikes (steps 2, 9, 16, ...), an 11-step
    sinusoid.  A function of the step alone: the table of a longer run starts with the table of a shorter one."""
    t = np.arange(n_steps)
    return _grid(np.stack([-0.9 * (1.0 - np.exp(-(t + 1.0) / 40.0)) - 0.05, np.where(t % 7 == 2, -2.5, 0.0),
                           0.1 * np.sin(2.0 * np.pi * t / 11.0 + 0.3)], axis=1), 10)


def scale_rows(name):
    """(sg [G, 16] in 0.75 .. 1.25, sx [3, 16] in 0.25 .. 2): multiples of 2^-6, none equal to 1, the gas rows of a member
    pairwise different (a scale on the wrong gas is then a different number)."""
    G = ir.case(name)["n_gas"]
    rng = np.random.default_rng(20261020 + CASES.index(name))
    sg, sx = np.empty((G, M)), np.empty((K_CAT, M))
    for m in range(M):                                          # drawn again until none is 1 and the gas scales differ
        while True:
            col = _grid(rng.uniform(0.75, 1.25, size=G), 6)
            if np.all(col != 1.0) and np.unique(col).size == G:
                break
        sg[:, m] = col
        while True:
            col = _grid(rng.uniform(0.25, 2.0, size=K_CAT), 6)
            if np.all(col != 1.0):
                break
        sx[:, m] = col
    return sg, sx


@functools.lru_cache(maxsize=None)
def case(name, n_steps=N_STEPS):
    """inverse_reference.case(name) with target and F_ext of n_steps steps, plus sg [G, 16], sx [3, 16] and X [n_steps, 3].
    Treat as read-only (cached)."""
    c = dict(ir.case(name))
    c["target"] = ir.target_series(c["params"]["PI_conc"], n_steps)
    c["F_ext"] = ir.f_ext_series(n_steps)
    c["sg"], c["sx"] = scale_rows(name)
    c["X"] = table(n_steps)
    c["n_steps"] = n_steps
    return c


def tiled_params(c, N):
    """The parameter dict of N members, f_scale [G, N] and fx_scale [3, N] included: member i is member i mod 16."""
    idx = np.arange(N) % M
    p = ir.tiled_params(c, N)
    p["f_scale"], p["fx_scale"] = c["sg"][:, idx], c["sx"][:, idx]
    return p


# ---- (a) the NumPy restatement, and the versions of it that are wrong on purpose ------------------------------------------------
VARIANTS = ("a scale on the neighbouring gas", "a category scale applied to F_ext", "scales applied to T_old instead of F")


def restated_step(c, R, S, cum, t, variant=None):
    """One inverse step with scales of the case's 16 members from the state given, restated from the oracle's step functions.
    variant: None, or one of VARIANTS — gas g's forcing scaled by the scale of gas g + 1 (cyclically); F_ext multiplied by the
    first category's scale; the gas scales multiplied into T_old (the temperature the feedback sees) and left off F."""
    p, dt, G = c["params"], c["dt"], c["n_gas"]
    a, tau = np.atleast_2d(np.asarray(p["a"], dtype=np.float64)), np.atleast_2d(np.asarray(p["tau"], dtype=np.float64))
    C0, cc = np.asarray(p["PI_conc"], dtype=np.float64).reshape(G), np.asarray(p["emis2conc"], dtype=np.float64).reshape(G)
    f, ra = np.asarray(p["f"], dtype=np.float64).reshape(G, 3), np.asarray(p["ra"], dtype=np.float64).reshape(G)
    sg, sx, X = c["sg"], c["sx"], c["X"]
    R, S, cum = [np.array(x) for x in ir._gas_rows(c, R)], np.array(S, dtype=np.float64), np.array(cum, dtype=np.float64)
    T_old = S[0] + S[1]
    if variant == VARIANTS[2]:
        T_old = T_old * sg[0]
    F = np.full(M, c["F_ext"][t])
    if variant == VARIANTS[1]:
        F = F * sx[0]
    for k in range(X.shape[1]):
        F = F + sx[k] * X[t, k]
    E_out = np.empty((G, M))
    for g, P in enumerate(c["pools"]):
        ag, tg = a[g, :P], tau[g, :P]
        G_a = np.sum(R[g], axis=0) / cc[g]
        alpha = npo.alpha_val(cum[g] - G_a, G_a, T_old, p["r0"][g], p["rC"][g], p["rT"][g], ra[g], float(npo.g_0(a[g], tau[g])),
                              float(npo.g_1(a[g], tau[g])), float(p["iirf_max"]))
        at = alpha[None, :] * tg[:, None]
        em1 = np.expm1(-dt / at)
        atc = ag[:, None] * tg[:, None] * cc[g]
        E = (np.sum(R[g] + R[g] * em1, axis=0) - (c["target"][t, g] - C0[g])) / (alpha * np.sum(atc * em1, axis=0))
        R[g] = R[g] + em1 * (R[g] - (ag[:, None] * (E[None, :] * cc[g])) * at)
        cum[g] = cum[g] + E * dt
        Fg = npo.step_forc(C0[g] + np.sum(R[g], axis=0), C0[g], f[g])
        scale = sg[(g + 1) % G] if variant == VARIANTS[0] else (1.0 if variant == VARIANTS[2] else sg[g])
        F = F + scale * Fg
        E_out[g] = E
    S, T = npo.step_temp(S, F, np.asarray(p["q"], dtype=np.float64), np.expm1(-dt / np.asarray(p["d"], dtype=np.float64)))
    return {"E": E_out, "T": T, "R": np.concatenate(R), "S": S, "cum": cum}


def restated_run(c):
    """restated_step() over the case's steps from a zero state: dict E [n_steps, G, 16], T [n_steps, 16], R, S, cum."""
    SP, G, n = sum(c["pools"]), c["n_gas"], c["n_steps"]
    R, S, cum = np.zeros((SP, M)), np.zeros((2, M)), np.zeros((G, M))
    E, T = np.empty((n, G, M)), np.empty((n, M))
    for t in range(n):
        out = restated_step(c, R, S, cum, t)
        E[t], T[t], R, S, cum = out["E"], out["T"], out["R"], out["S"], out["cum"]
    return {"E": E, "T": T, "R": R, "S": S, "cum": cum}


@functools.lru_cache(maxsize=None)
def oracle_run(name, n_steps=N_STEPS):
    """oracle.fiveeq_oracle.run_inverse MEMBER BY MEMBER: each member alone, its f[g] multiplied by its sg_g and F_ext + X @ sx
    as its external forcing — no step code of this module.  dict E [n_steps, G, 16], T [n_steps, 16], R [SP, 16], S, cum."""
    c = case(name, n_steps)
    p, G = c["params"], c["n_gas"]
    base_f = np.asarray(p["f"], dtype=np.float64).reshape(G, 3)
    E, T = np.empty((n_steps, G, M)), np.empty((n_steps, M))
    R, S, cum = np.empty((sum(c["pools"]), M)), np.empty((2, M)), np.empty((G, M))
    for m in range(M):
        pm = {k: (v[:, m:m + 1] if k in ("r0", "rC", "rT", "q") else v) for k, v in p.items()}
        pm["f"] = base_f * c["sg"][:, m][:, None]
        o = npo.run_inverse(c["target"], pm, 1, F_ext=c["F_ext"] + c["X"] @ c["sx"][:, m], dt=c["dt"])
        E[:, :, m], T[:, m] = o["E"][:, :, 0], o["T"][:, 0]
        R[:, m], S[:, m], cum[:, m] = np.concatenate(o["R"])[:, 0], o["S"][:, 0], o["cumE"][:, 0]
    return {"E": E, "T": T, "R": R, "S": S, "cum": cum}


# ---- (b) the 50-digit step of each member on its own model ------------------------------------------------------------------------
def _widen_thermal_scales(out, mc, q, F_ext, terms):
    """The A parts of sS and sT of one member's step_inverse() result, grown by the cancellation among the external terms the
    added fma's round one by one: |em1_d_j| |q_j| (|F_ext| + sum |terms| - |F_ext + sum terms|)."""
    extra = abs(F_ext) + mp.fsum(abs(v) for v in terms) - abs(F_ext + mp.fsum(terms))
    A, B = out["sS"]
    A = [A[j] + abs(mc["em1_d"][j]) * abs(sr.M(float(q[j]))) * extra for j in range(2)]
    out["sS"], out["sT"] = (A, B), (A[0] + A[1], out["sT"][1])


def step_reference(c, R, S, cum, t):
    """The 50-digit inverse step t with scales of the case's 16 members from the state R [SP, 16], S [2, 16], cum [G, 16] (fp64
    arrays: what the program under test holds before the step), in the layout of inverse_reference.step_reference()."""
    p, G = c["params"], c["n_gas"]
    R, S, cum = ir._gas_rows(c, R), np.asarray(S, dtype=np.float64), np.asarray(cum, dtype=np.float64)
    cols = []
    with mp.workdps(sr.DPS):
        for m in range(M):
            mc = dict(c["mc"], gases=[dict(gs, f=[v * sr.M(float(c["sg"][g, m])) for v in gs["f"]])
                                      for g, gs in enumerate(c["mc"]["gases"])])
            F_ext = sr.M(float(c["F_ext"][t]))
            terms = [sr.M(float(c["sx"][k, m])) * sr.M(float(c["X"][t, k])) for k in range(c["X"].shape[1])]
            r = [[p[k][g, m] for k in ("r0", "rC", "rT")] for g in range(G)]
            q = list(p["q"][:, m])
            col = sr.step_inverse(mc, r, q, [list(Rg[:, m]) for Rg in R], list(S[:, m]), list(cum[:, m]), list(c["target"][t]),
                                  F_ext + mp.fsum(terms))
            _widen_thermal_scales(col, mc, q, F_ext, terms)
            cols.append(col)
        flat = lambda per_gas: [v for gas in per_gas for v in gas]                                   # noqa: E731
        per_gas = lambda key: [[col[key][g] for col in cols] for g in range(G)]                      # noqa: E731
        return {"E": sr._pack(per_gas("E")), "cum": sr._pack(per_gas("cum")), "C": sr._pack(per_gas("C")),
                "T": sr._pack([[col["T"] for col in cols]]),
                "R": sr._pack(list(zip(*[flat(col["R"]) for col in cols]))),
                "S": sr._pack([[col["S"][j] for col in cols] for j in range(2)]),
                "sE": np.array(per_gas("sE"), dtype=np.float64), "scum": np.array(per_gas("scum"), dtype=np.float64),
                "sC": np.array(per_gas("sC"), dtype=np.float64),
                "sR": np.array([[float(v) for v in flat(col["sR"])] for col in cols]).T,
                "sT": (np.array([[float(col["sT"][0]) for col in cols]]), np.array([[float(col["sT"][1]) for col in cols]])),
                "sS": (np.array([[float(col["sS"][0][j]) for col in cols] for j in range(2)]),
                       np.array([[float(col["sS"][1][j]) for col in cols] for j in range(2)])),
                "iirf": np.array(per_gas("iirf"), dtype=np.float64)}


def anchored(c, step, eps=sr.EPS["f64"]):
    """`step` run over the case's steps one at a time from its own state (zero at step 0), each step measured against
    step_reference() from that state: (worst units per output over all steps and members, [(outputs, reference)] per step)."""
    SP, G = sum(c["pools"]), c["n_gas"]
    R, S, cum = np.zeros((SP, M)), np.zeros((2, M)), np.zeros((G, M))
    worst, steps = dict.fromkeys(OUTPUTS, 0.0), []
    for t in range(c["n_steps"]):
        ref = step_reference(c, R, S, cum, t)
        got = step(c, R, S, cum, t)
        for name, u in units(got, ref, eps).items():
            worst[name] = max(worst[name], float(u.max()))
        steps.append((got, ref))
        R, S, cum = got["R"], got["S"], got["cum"]
    return worst, steps


@functools.lru_cache(maxsize=None)
def restated_anchored(name):
    """anchored(case(name), restated_step), cached: the measurement of K."""
    return anchored(case(name), restated_step)
