"""The cases, the 50-digit step and the NumPy twin of the MIXED DRIVE (include/fiveeq.h "MIXED DRIVE", fused_mixed_kernel): some
gases concentration-driven, the others emission-driven, by a per-gas mask (bit g set = gas g concentration-driven).

TEST INFRASTRUCTURE, beside tests/step_reference.py and tests/inverse_reference.py, whose method it keeps: ANCHORED STEPS (one
step at a time from the state the program under test holds itself, each held to the 50-digit step from exactly that state, in
units of eps x scale: errors do not accumulate) and ONE ARITHMETIC (tests/test_mixed_gpu.py).

CASES: the two 4 + 1 + 1 cases of inverse_reference — "4+1+1" (a drawn model, dt = 1) and "multigas dt=0.5" (the default set
with the 1e6-year pool) — with its 16 fp32-exact members, its target series and its F_ext.  An emission-driven gas takes
EMIS_AMPLITUDE[g] x SHAPE[t]: the shape of the targets (zero at step 0, rising, held, falling through zero, NEGATIVE emissions,
returning), amplitudes that are fp32-exact (so are the running sums: multiples of 1/8 times dt) and sized so that C leaves C0
by about what the targets do: 1.5 GtC/yr, 16 Mt CH4/yr and 2 Mt N2O-N2/yr per unit of SHAPE against 2 ppm, 24 ppb and 1.5 ppb.
"""
import functools

import mpmath as mp
import numpy as np

import inverse_reference as ir
import step_reference as sr
from oracle import fiveeq_oracle as npo

M = ir.M
N_STEPS = ir.N_STEPS
CASES = ("4+1+1", "multigas dt=0.5")
MASKS = (0b001, 0b010, 0b011, 0b100, 0b101, 0b110)         # the proper masks of three gases
EMIS_AMPLITUDE = np.array([1.5, 16.0, 2.0])                # per unit of SHAPE
OUTPUTS = ("X", "T", "R", "S", "cum")                      # X: per gas, C (emission-driven) or E (concentration-driven)
VARIANTS = ("alpha of a concentration-driven gas from the shared drive column", "cum advanced for an emission-driven gas",
            "E of an emission-driven gas read from column 3 + g")


def concentration_gases(mask, n_gas=3):
    return tuple(g for g in range(n_gas) if mask >> g & 1)


def emission_series(n_steps=N_STEPS, n_gas=3):
    """[n_steps, G]: EMIS_AMPLITUDE x SHAPE (the 12-step shape repeated)."""
    return np.resize(ir.SHAPE, n_steps)[:, None] * EMIS_AMPLITUDE[None, :n_gas]


@functools.lru_cache(maxsize=None)
def case(name, n_steps=N_STEPS):
    """inverse_reference.case(name) over n_steps steps, with the emission series E [n_steps, G] and its cumulative sums BEFORE
    each step, cum_shared [n_steps, G] (what drive columns 3 + g hold for an emission-driven gas).  Read-only (cached)."""
    assert name in CASES, name
    c = dict(ir.case(name))
    E = emission_series(n_steps, c["n_gas"])
    cum = np.zeros_like(E)
    cum[1:] = np.cumsum(E * c["dt"], axis=0)[:-1]
    c.update(target=ir.target_series(c["params"]["PI_conc"], n_steps), F_ext=ir.f_ext_series(n_steps), E=E, cum_shared=cum,
             n_steps=n_steps)
    return c


def drive_columns(c, mask):
    """What the drive table of the case holds under `mask`: (cols 0..G-1, cols 3..3+G-1), each [n_steps, G]."""
    conc = np.array([bool(mask >> g & 1) for g in range(c["n_gas"])])
    return np.where(conc[None, :], c["target"], c["E"]), np.where(conc[None, :], 0.0, c["cum_shared"])


# ---- the 50-digit step ---------------------------------------------------------------------------------------------------------
def _member_step(mc, mask, r, q, R, S, cum, cum_shared, drv, F_ext):
    """One mixed step of one member in 50 digits, composed per gas from step_reference's pieces with the scales of
    step_forward (an emission-driven gas: X = C) and step_inverse (a concentration-driven gas: X = E, cum advanced).  cum of an
    emission-driven gas is returned unchanged with scale 0: the program under test must not touch it."""
    M_ = sr.M
    with mp.workdps(sr.DPS):
        S = [M_(v) for v in S]
        T_old = S[0] + S[1]
        F, F_abs, dF = M_(F_ext), abs(M_(F_ext)), M_(0)
        out = dict(R=[], C=[], X=[], iirf=[], sR=[], sC=[], sX=[], cum=[], scum=[])
        for g, gs in enumerate(mc["gases"]):
            inv = bool(mask >> g & 1)
            Rg = [M_(v) for v in R[g]]
            iirf, alpha, k = sr._alpha(gs, mc["iirf_max"], [M_(v) for v in r[g]], Rg, M_(cum[g]) if inv else M_(cum_shared[g]), T_old)
            em1 = [mp.expm1(-mc["dt"] / (alpha * ti)) for ti in gs["tau"]]
            if inv:
                num = mp.fsum(Ri + Ri * e for Ri, e in zip(Rg, em1))
                den = alpha * mp.fsum(ai * ti * gs["c"] * e for ai, ti, e in zip(gs["a"], gs["tau"], em1))
                Eg = (num - (M_(drv[g]) - gs["C0"])) / den
                sE = k * (mp.fsum(abs(Ri) * (1 + abs(e)) for Ri, e in zip(Rg, em1)) + abs(M_(drv[g])) + abs(gs["C0"])) / abs(den)
                out["cum"].append(M_(cum[g]) + Eg * mc["dt"]), out["scum"].append(abs(M_(cum[g])) + mc["dt"] * sE)
            else:
                Eg = M_(drv[g])
                out["cum"].append(M_(cum[g])), out["scum"].append(M_(0))
            dR = [e * (Ri - ai * gs["c"] * Eg * alpha * ti) for Ri, e, ai, ti in zip(Rg, em1, gs["a"], gs["tau"])]
            Rn = [Ri + di for Ri, di in zip(Rg, dR)]
            C = gs["C0"] + mp.fsum(Rn)
            sC = abs(gs["C0"]) + mp.fsum(abs(v) for v in Rg) + k * mp.fsum(abs(v) for v in dR)
            Fg, Fg_abs, dFdC = sr._forcing(gs, C)
            F, F_abs, dF = F + Fg, F_abs + Fg_abs, dF + dFdC * sC
            out["R"].append(Rn), out["C"].append(C), out["iirf"].append(iirf), out["sC"].append(sC)
            out["X"].append(Eg if inv else C), out["sX"].append(sE if inv else sC)
            out["sR"].append([abs(Ri) + k * abs(di) for Ri, di in zip(Rg, dR)])
        Sn, A, B = sr._thermal(mc, [M_(v) for v in q], S, F, F_abs, dF)
        out.update(S=Sn, T=Sn[0] + Sn[1], sS=(A, B), sT=(A[0] + A[1], B[0] + B[1]))
        return out


def step_reference(c, mask, R, S, cum, t, scales=None):
    """The 50-digit mixed step t of the case's M members from the state R [SP, M], S [2, M], cum [G, M] (fp64 arrays: what the
    program under test holds before the step).  The layout step_reference.err_units() takes: values as fp64 pairs (hi, lo)
    under "X" (C of an emission-driven gas, E of a concentration-driven one), "cum", "C" [G, M], "T" [1, M], "R" [SP, M],
    "S" [2, M]; scales under "sX", "scum" (0 for an emission-driven gas, whose cum is returned unchanged), "sC", "sR" and the
    pairs "sT", "sS"; "iirf" [G, M] un-clamped.  scales = (sg [G, M], sx [K, M], X [n_steps, K]): the step with per-member
    forcing scales, as inverse_forcing_reference.step_reference has it — each member on its own model (f of gas g times sg_g),
    F_ext + sum_k sx_k X[t, k] as its external forcing, and the thermal scales widened by the cancellation among those terms
    (inverse_forcing_reference._widen_thermal_scales)."""
    import inverse_forcing_reference as fr
    p, G = c["params"], c["n_gas"]
    R, S, cum = ir._gas_rows(c, R), np.asarray(S, dtype=np.float64), np.asarray(cum, dtype=np.float64)
    col0, _ = drive_columns(c, mask)
    cols = []
    for m in range(M):
        r = [[p[k][g, m] for k in ("r0", "rC", "rT")] for g in range(G)]
        q, state = list(p["q"][:, m]), ([list(Rg[:, m]) for Rg in R], list(S[:, m]), list(cum[:, m]))
        if scales is None:
            cols.append(_member_step(c["mc"], mask, r, q, *state, list(c["cum_shared"][t]), list(col0[t]), c["F_ext"][t]))
            continue
        sg, sx, X = scales
        with mp.workdps(sr.DPS):
            mc = dict(c["mc"], gases=[dict(gs, f=[v * sr.M(float(sg[g, m])) for v in gs["f"]])
                                      for g, gs in enumerate(c["mc"]["gases"])])
            F_ext = sr.M(float(c["F_ext"][t]))
            terms = [sr.M(float(sx[k, m])) * sr.M(float(X[t, k])) for k in range(X.shape[1])]
            col = _member_step(mc, mask, r, q, *state, list(c["cum_shared"][t]), list(col0[t]), F_ext + mp.fsum(terms))
            fr._widen_thermal_scales(col, mc, q, F_ext, terms)
        cols.append(col)
    flat = lambda per_gas: [v for gas in per_gas for v in gas]                                   # noqa: E731
    per_gas = lambda key: [[col[key][g] for col in cols] for g in range(G)]                      # noqa: E731
    with mp.workdps(sr.DPS):
        return {"X": sr._pack(per_gas("X")), "cum": sr._pack(per_gas("cum")), "C": sr._pack(per_gas("C")),
                "T": sr._pack([[col["T"] for col in cols]]),
                "R": sr._pack(list(zip(*[flat(col["R"]) for col in cols]))),
                "S": sr._pack([[col["S"][j] for col in cols] for j in range(2)]),
                "sX": np.array(per_gas("sX"), dtype=np.float64), "scum": np.array(per_gas("scum"), dtype=np.float64),
                "sC": np.array(per_gas("sC"), dtype=np.float64),
                "sR": np.array([[float(v) for v in flat(col["sR"])] for col in cols]).T,
                "sT": (np.array([[float(col["sT"][0]) for col in cols]]), np.array([[float(col["sT"][1]) for col in cols]])),
                "sS": (np.array([[float(col["sS"][0][j]) for col in cols] for j in range(2)]),
                       np.array([[float(col["sS"][1][j]) for col in cols] for j in range(2)])),
                "iirf": np.array(per_gas("iirf"), dtype=np.float64)}


def units(got, ref, eps):
    """|got - ref| / (eps x scale) per output of OUTPUTS.  Where the scale is zero — the pools of step 0, and cum of an
    emission-driven gas at every step — the reference must be met exactly: 0 units for that, inf for anything else (NaN: inf)."""
    out = {}
    for name in OUTPUTS:
        g = np.asarray(got[name], dtype=np.float64).reshape(ref[name][0].shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            u = sr.err_units(g, ref, name, eps)
        u = np.where(sr.scale_of(ref, name, eps) == 0, np.where(g == ref[name][0], 0.0, np.inf), u)
        out[name] = np.where(np.isnan(u), np.inf, u)
    return out


# ---- the NumPy twin --------------------------------------------------------------------------------------------------------------
def restated_step(c, mask, R, S, cum, t, variant=None):
    """The mixed step written from the oracle's pieces: per gas the statements of fiveeq_oracle.run (an emission-driven gas) or
    of inverse_reference.restated_step (a concentration-driven gas), F and the thermal step as both have them.  variant: one of
    VARIANTS, a mistake made on purpose —
      [0] alpha of a concentration-driven gas from drive column 3 + g (zero for such a gas) instead of the member's own cum;
      [1] cum advanced by E dt for an emission-driven gas too;
      [2] the emission rate of an emission-driven gas read from column 3 + g (the cumulative emissions) instead of column g."""
    p, dt, G = c["params"], c["dt"], c["n_gas"]
    a, tau = np.atleast_2d(np.asarray(p["a"], dtype=np.float64)), np.atleast_2d(np.asarray(p["tau"], dtype=np.float64))
    C0, cc = np.asarray(p["PI_conc"], dtype=np.float64).reshape(G), np.asarray(p["emis2conc"], dtype=np.float64).reshape(G)
    f, ra = np.asarray(p["f"], dtype=np.float64).reshape(G, 3), np.asarray(p["ra"], dtype=np.float64).reshape(G)
    R, S, cum = [np.array(x) for x in ir._gas_rows(c, R)], np.array(S, dtype=np.float64), np.array(cum, dtype=np.float64)
    col0, col3 = drive_columns(c, mask)
    T_old = S[0] + S[1]
    F, X = np.zeros(M), np.empty((G, M))
    for g, P in enumerate(c["pools"]):
        ag, tg = a[g, :P], tau[g, :P]
        G_a = np.sum(R[g], axis=0) / cc[g]
        g0, g1 = float(npo.g_0(a[g], tau[g])), float(npo.g_1(a[g], tau[g]))
        if mask >> g & 1:
            own = np.full(M, col3[t, g]) if variant == VARIANTS[0] else cum[g]
            alpha = npo.alpha_val(own - G_a, G_a, T_old, p["r0"][g], p["rC"][g], p["rT"][g], ra[g], g0, g1, float(p["iirf_max"]))
            at = alpha[None, :] * tg[:, None]
            em1 = np.expm1(-dt / at)
            atc = ag[:, None] * tg[:, None] * cc[g]
            E = (np.sum(R[g] + R[g] * em1, axis=0) - (col0[t, g] - C0[g])) / (alpha * np.sum(atc * em1, axis=0))
            R[g] = R[g] + em1 * (R[g] - (ag[:, None] * (E[None, :] * cc[g])) * at)
            cum[g] = cum[g] + E * dt
            Cg = C0[g] + np.sum(R[g], axis=0)
            X[g] = E
        else:
            E = col3[t, g] if variant == VARIANTS[2] else col0[t, g]
            alpha = npo.alpha_val(col3[t, g] - G_a, G_a, T_old, p["r0"][g], p["rC"][g], p["rT"][g], ra[g], g0, g1,
                                  float(p["iirf_max"]))
            R[g], Cg = npo.step_conc(R[g], alpha, E * cc[g], ag, tg, C0[g], dt)
            if variant == VARIANTS[1]:
                cum[g] = cum[g] + E * dt
            X[g] = Cg
        F = F + npo.step_forc(Cg, C0[g], f[g])
    S, T = npo.step_temp(S, F + c["F_ext"][t], np.asarray(p["q"], dtype=np.float64), np.expm1(-dt / np.asarray(p["d"], dtype=np.float64)))
    return {"X": X, "T": T, "R": np.concatenate(R), "S": S, "cum": cum}


def anchored(c, mask, step, eps=sr.EPS["f64"]):
    """`step(c, mask, R, S, cum, t)` over the case's steps, one at a time from its own state (zero at step 0), each measured
    against the 50-digit step from that state.  Returns (worst units per output, the per-step list of (outputs, reference))."""
    SP, G = sum(c["pools"]), c["n_gas"]
    R, S, cum = np.zeros((SP, M)), np.zeros((2, M)), np.zeros((G, M))
    worst, steps = dict.fromkeys(OUTPUTS, 0.0), []
    for t in range(c["n_steps"]):
        ref = step_reference(c, mask, R, S, cum, t)
        got = step(c, mask, R, S, cum, t)
        for name, u in units(got, ref, eps).items():
            worst[name] = max(worst[name], float(u.max()))
        steps.append((got, ref))
        R, S, cum = got["R"], got["S"], got["cum"]
    return worst, steps


@functools.lru_cache(maxsize=None)
def restated_anchored(name, mask):
    """anchored(case(name), mask, restated_step), cached: the measurement of K_MIXED and the trajectory the input conditions
    are checked on."""
    return anchored(case(name), mask, restated_step)


def tiled_params(c, N):
    return ir.tiled_params(c, N)
