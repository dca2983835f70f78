"""One guarded model step in 50 digits (mpmath), and the edge ensemble the step tests run it on.

TEST INFRASTRUCTURE.  tests/golden/make_fiveeq_mp_reference.py restates the recurrence in 50 digits WITHOUT the step's two
data-dependent decisions; this module restates ONE step WITH them, as oracle.fiveeq_oracle has them:

    the C <= 0 guard   the log term is dropped and sqrt C := 0 (step_forc);
    the iIRF clamp     min(iIRF, iirf_max) (alpha_val).

Both decisions are taken in 50 digits.  Inputs are the fp64 numbers the engine and the oracle receive; everything derived
from them (g0, g1, expm1(-dt/d), alpha, ...) is recomputed here.  The per-member inputs of the edge ensemble are all exactly
representable in fp32, the emissions are multiples of 2^-10 whose running sums are exact in fp32, so ONE reference serves
the fp64 and the fp32 kernels: what a kernel's host does to the SHARED model constants (rounding them to fp32, folding them
into inv_g1, ndt_over_tau, atc) is part of the error under test.

CONDITION SCALES.  Every output comes with the sum of the magnitudes of the terms added to form it; errors are measured in
units of eps(dtype) x scale:

    R_i   |R_i| + k |dR_i|,                    k = 1 + |iIRF / g1| (the clamped iIRF: the exponent of alpha), dR_i the increment
    C_g   |C0| + sum_i |R_i| + k sum_i |dR_i|
    S_j   |S_j| + |em1_d_j| (|S_j| + |q_j| (sum |forcing terms| + sum_g |dF_g/dC_g| scale_C_g eps))
    T     sum_j of the S_j scales
    E     k (sum_i |R_i| (1 + |em1_i|) + |C*| + |C0|) / |alpha sum_i a_i tau_i c em1_i|      (the inverse step's diagnosed rate:
          the terms of its numerator over its denominator, and alpha's own conditioning k)
    cum   |cum| + dt x the scale of E                                (the inverse step's cumulative emissions, cum + E dt)

the forcing terms being |F_ext| and per gas |f1 ln(C/C0)| (dropped by the guard), |f2 (C - C0)|, |f3 sqrt C| (0 under the
guard) and |f3 sqrt C0|.  The S and T scales depend on eps through the last term and are returned as a pair (A, B):
scale = A + B eps.
"""
import functools

import mpmath as mp
import numpy as np

from fiveeqscm_amd import emissions as emi
from fiveeqscm_amd import params as prm

DPS = 50
M = mp.mpf
EPS = {"f64": float(np.finfo(np.float64).eps), "f32": float(np.finfo(np.float32).eps)}


def _m(x):
    return M(float(x))


def model_consts(params, dt=1.0):
    """The shared model in 50 digits: per gas (a, tau, g0, g1, ra, C0, c, f), the thermal boxes' expm1(-dt/d), iirf_max."""
    with mp.workdps(DPS):
        a_all = np.atleast_2d(np.asarray(params["a"], dtype=np.float64))
        tau_all = np.atleast_2d(np.asarray(params["tau"], dtype=np.float64))
        G = a_all.shape[0]
        H = M(100)
        gases = []
        for g in range(G):
            P = int(np.nonzero(a_all[g])[0][-1]) + 1
            a = [_m(v) for v in a_all[g, :P]]
            tau = [_m(v) for v in tau_all[g, :P]]
            g1 = mp.fsum(ai * ti * (1 - (1 + H / ti) * mp.exp(-H / ti)) for ai, ti in zip(a, tau))
            g0 = mp.exp(-mp.fsum(ai * ti * (1 - mp.exp(-H / ti)) for ai, ti in zip(a, tau)) / g1)
            gases.append(dict(a=a, tau=tau, g0=g0, g1=g1, ra=_m(np.asarray(params["ra"], dtype=np.float64).reshape(G)[g]),
                              C0=_m(np.asarray(params["PI_conc"], dtype=np.float64).reshape(G)[g]),
                              c=_m(np.asarray(params["emis2conc"], dtype=np.float64).reshape(G)[g]),
                              f=[_m(v) for v in np.asarray(params["f"], dtype=np.float64).reshape(G, 3)[g]]))
        dtm = _m(dt)
        return dict(gases=gases, dt=dtm, em1_d=[mp.expm1(-dtm / _m(v)) for v in params["d"]], iirf_max=_m(params["iirf_max"]))


def _forcing(gs, C):
    """(F_g, sum of |terms|, |dF_g/dC|) with the oracle's guards, decided in 50 digits."""
    f1, f2, f3 = gs["f"]
    C0 = gs["C0"]
    pos = C > 0
    logt = f1 * mp.log(C / C0) if pos else M(0)
    sq = f3 * mp.sqrt(C) if pos else M(0)
    lin = f2 * (C - C0)
    F = logt + lin + (sq - f3 * mp.sqrt(C0))
    dFdC = f2 + ((f1 / C + f3 / (2 * mp.sqrt(C))) if pos else M(0))
    return F, abs(logt) + abs(lin) + abs(sq) + abs(f3 * mp.sqrt(C0)), abs(dFdC)


def _alpha(gs, iirf_max, r, R, cum, T_old):
    G_a = mp.fsum(R) / gs["c"]
    iirf = r[0] + r[1] * (cum - G_a) + r[2] * T_old + gs["ra"] * G_a
    clamped = min(iirf, iirf_max)
    return iirf, gs["g0"] * mp.exp(clamped / gs["g1"]), 1 + abs(clamped / gs["g1"])


def _thermal(mc, q, S, F, F_abs, dF):
    """S_j + em1_d_j (S_j - q_j F) and its scale as the pair (A_j, B_j): scale = A + B eps."""
    Sn, A, B = [], [], []
    for j in range(2):
        e = mc["em1_d"][j]
        Sn.append(S[j] + e * (S[j] - q[j] * F))
        A.append(abs(S[j]) + abs(e) * (abs(S[j]) + abs(q[j]) * F_abs))
        B.append(abs(e) * abs(q[j]) * dF)
    return Sn, A, B


def step_forward(mc, r, q, R, S, cum, E, F_ext):
    """One emission-driven step of one member.  mc: model_consts(); r [G][3] = (r0, rC, rT) per gas; q [2]; R: one list of
    pools per gas; S [2]; cum [G]: cumulative emissions BEFORE the step; E [G]; F_ext.  All fp64 numbers (or mpf).
    Returns a dict of mpf: R (per gas), S, C [G], T, iirf [G] (UN-clamped), and the scales sR (per gas), sC [G], and the
    pairs sS = (A [2], B [2]), sT = (A, B)."""
    with mp.workdps(DPS):
        S = [M(v) for v in S]
        T_old = S[0] + S[1]
        F, F_abs, dF = M(F_ext), abs(M(F_ext)), M(0)
        out = dict(R=[], C=[], iirf=[], sR=[], sC=[])
        for g, gs in enumerate(mc["gases"]):
            Rg = [M(v) for v in R[g]]
            iirf, alpha, k = _alpha(gs, mc["iirf_max"], [M(v) for v in r[g]], Rg, M(cum[g]), T_old)
            dR = [mp.expm1(-mc["dt"] / (alpha * ti)) * (Ri - ai * gs["c"] * M(E[g]) * alpha * ti)
                  for Ri, ai, ti in zip(Rg, gs["a"], gs["tau"])]
            Rn = [Ri + di for Ri, di in zip(Rg, dR)]
            C = gs["C0"] + mp.fsum(Rn)
            sC = abs(gs["C0"]) + mp.fsum(abs(v) for v in Rg) + k * mp.fsum(abs(v) for v in dR)
            Fg, Fg_abs, dFdC = _forcing(gs, C)
            F, F_abs, dF = F + Fg, F_abs + Fg_abs, dF + dFdC * sC
            out["R"].append(Rn), out["C"].append(C), out["iirf"].append(iirf), out["sC"].append(sC)
            out["sR"].append([abs(Ri) + k * abs(di) for Ri, di in zip(Rg, dR)])
        Sn, A, B = _thermal(mc, [M(v) for v in q], S, F, F_abs, dF)
        out.update(S=Sn, T=Sn[0] + Sn[1], sS=(A, B), sT=(A[0] + A[1], B[0] + B[1]))
        return out


def step_inverse(mc, r, q, R, S, cum, C_target, F_ext):
    """The concentration-driven counterpart: C_target [G] (the concentration at the END of the step) in, the diagnosed
    emission rate E [G] out, with its scale sE; cum [G] is the member's own cumulative emissions before the step.
    Also R, S, C (the concentration reached), T, iirf and their scales, as step_forward(), and the member's cumulative
    emissions AFTER the step, cum [G] = cum_g + E_g dt, with their scale scum = |cum_g| + dt sE_g."""
    with mp.workdps(DPS):
        S = [M(v) for v in S]
        T_old = S[0] + S[1]
        F, F_abs, dF = M(F_ext), abs(M(F_ext)), M(0)
        out = dict(R=[], C=[], E=[], iirf=[], sR=[], sC=[], sE=[], cum=[], scum=[])
        for g, gs in enumerate(mc["gases"]):
            Rg = [M(v) for v in R[g]]
            iirf, alpha, k = _alpha(gs, mc["iirf_max"], [M(v) for v in r[g]], Rg, M(cum[g]), T_old)
            em1 = [mp.expm1(-mc["dt"] / (alpha * ti)) for ti in gs["tau"]]
            num = mp.fsum(Ri + Ri * e for Ri, e in zip(Rg, em1))
            den = alpha * mp.fsum(ai * ti * gs["c"] * e for ai, ti, e in zip(gs["a"], gs["tau"], em1))
            Eg = (num - (M(C_target[g]) - gs["C0"])) / den
            sE = k * (mp.fsum(abs(Ri) * (1 + abs(e)) for Ri, e in zip(Rg, em1)) + abs(M(C_target[g])) + abs(gs["C0"])) / abs(den)
            dR = [e * (Ri - ai * gs["c"] * Eg * alpha * ti) for Ri, e, ai, ti in zip(Rg, em1, gs["a"], gs["tau"])]
            Rn = [Ri + di for Ri, di in zip(Rg, dR)]
            C = gs["C0"] + mp.fsum(Rn)
            sC = abs(gs["C0"]) + mp.fsum(abs(v) for v in Rg) + k * mp.fsum(abs(v) for v in dR)
            Fg, Fg_abs, dFdC = _forcing(gs, C)
            F, F_abs, dF = F + Fg, F_abs + Fg_abs, dF + dFdC * sC
            out["R"].append(Rn), out["C"].append(C), out["E"].append(Eg), out["iirf"].append(iirf)
            out["sC"].append(sC), out["sE"].append(sE)
            out["cum"].append(M(cum[g]) + Eg * mc["dt"]), out["scum"].append(abs(M(cum[g])) + mc["dt"] * sE)
            out["sR"].append([abs(Ri) + k * abs(di) for Ri, di in zip(Rg, dR)])
        Sn, A, B = _thermal(mc, [M(v) for v in q], S, F, F_abs, dF)
        out.update(S=Sn, T=Sn[0] + Sn[1], sS=(A, B), sT=(A[0] + A[1], B[0] + B[1]))
        return out


# ------------------------------------------------------------------------------------------------
# the edge ensemble
# ------------------------------------------------------------------------------------------------
CLASSES = ("in-domain", "guarded", "clamped", "guarded+clamped", "slow-pool")        # (a) .. (e)
IN_DOMAIN, GUARDED, CLAMPED, BOTH, SLOW = range(5)
N_MAX = 202            # the ensembles of 200, 201 and 202 members are the first members of this one
T0 = 3                 # the step under test is run(T0, T0 + 1): cumulative emissions are not zero
N_STEPS = T0 + 9       # ... and the isolation runs go on for 9 steps (a fused 8-step statistics flush and a ragged rest)
PAIR_SHIFT = 8         # see member_classes()


def member_classes(N=N_MAX):
    """Class of each member.  Packed lane l (members 2l, 2l + 1) holds the ordered pair number (l + PAIR_SHIFT) mod 25 of the
    25 ordered pairs of classes (first = pair // 5, second = pair mod 5): every ordered pair sits in one packed lane every 50
    members.  Consecutive lanes hold consecutive pairs, whose second members differ: every aligned quad and octet of
    members is mixed.  PAIR_SHIFT = 8 puts (e | d) across members 63 | 64, (b | e) across 127 | 128, a guarded member first
    (member 0) and a guarded member alone in the last packed lane of 201."""
    i = np.arange(N)
    pair = (i // 2 + PAIR_SHIFT) % 25
    return np.where(i % 2 == 0, pair // 5, pair % 5)


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def edge_ensemble(kind):
    """The N_MAX-member edge ensemble of parameter set `kind` ("multigas": pools 4 + 1 + 1; "co2": pools {4}).
    Returns dict: params (per-member rows [., N_MAX]), R0 [SP, N_MAX], S0 [2, N_MAX], E [N_STEPS, G], F_ext [N_STEPS],
    cls [N_MAX], guard_gas / clamp_gas [N_MAX] (the gas a guarded / clamped member is driven out of domain in),
    target [G] (the inverse step's shared target concentrations).  Treat as read-only (cached)."""
    base = prm.default_params(kind)
    G, N = prm.n_gas_of(base), N_MAX
    pools = prm.pools_of(base)
    rng = np.random.default_rng(20261018)
    p = {k: v for k, v in prm.sample_ensemble(base, N, seed=20261018).items() if k not in ("TCR", "ECS")}
    cls = member_classes(N)
    i = np.arange(N)
    rep = i // 50
    guard_gas = rep % G                                             # every pair meets every gas as the guarded one
    clamp_gas = (rep + i % 2 + (i // 2) % 2) % G                    # ... and the clamped gas equal to it or not
    guarded, clamped = np.isin(cls, (GUARDED, BOTH)), np.isin(cls, (CLAMPED, BOTH))
    C0 = np.asarray(base["PI_conc"], dtype=np.float64).reshape(G)

    # state: in-domain excesses, then the classes' own
    w = np.array([0.45, 0.30, 0.17, 0.08])[:, None] * rng.uniform(0.7, 1.3, size=(4, N))
    w /= w.sum(0)
    R0 = [w * rng.uniform(60.0, 160.0, size=N)]
    if G == 3:
        R0 += [rng.uniform(300.0, 1100.0, size=(1, N)), rng.uniform(20.0, 60.0, size=(1, N))]
    slow = cls == SLOW                                                 # (e): the slow pool (tau = 1e6 yr) holds the excess
    R0[0][:, slow] = rng.uniform(100.0, 200.0, size=slow.sum()) * np.array([1.0, 1e-3, 1e-4, 1e-5])[:, None]
    for g in range(G):                                              # (b), (d): pools summing to -1.5 C0
        sel = guarded & (guard_gas == g)
        R0[g][:, sel] = -1.5 * C0[g] * (w[:, sel] if pools[g] == 4 else 1.0)
    S0 = np.stack([rng.uniform(0.3, 0.9, size=N), rng.uniform(0.2, 0.8, size=N)])
    S0[:, clamped] = np.array([9.0, 6.0])[:, None] * rng.uniform(0.95, 1.05, size=(2, int(clamped.sum())))   # T_old ~ 15 K
    # (c), (d): with T_old ~ 15 K the clamped gas's rT takes its iIRF far past iirf_max = 97, the other gases' keeps theirs below
    rT_over, rT_under = (6.0, 8.0, 4.0), (1.0, None, 0.0)
    rT = np.array(p["rT"], dtype=np.float64)
    for g in range(G):
        rT[g, clamped & (clamp_gas == g)] = rT_over[g]
        if rT_under[g] is not None:
            rT[g, clamped & (clamp_gas != g)] = rT_under[g]
    p["rT"] = rT
    for k in ("r0", "rC", "rT", "q"):
        p[k] = _f32(p[k])
    E_ = np.round(emi.rcp_like_emissions(750, G)[300:300 + N_STEPS] * 1024.0) / 1024.0
    F_ext = np.round((0.3 + 0.02 * np.arange(N_STEPS)) * 1024.0) / 1024.0
    target = np.array([330.0, 1500.0, -135.0][:G])                  # N2O's is -0.5 C0: the inverse step's guard, every member
    return dict(params=p, R0=_f32(np.concatenate(R0, axis=0)), S0=_f32(S0), E=E_, F_ext=F_ext, cls=cls, guard_gas=guard_gas,
                clamp_gas=clamp_gas, target=target, pools=pools, n_gas=G)


def member_params(ens, N):
    """The parameter dict of the first N members."""
    return {k: (v[:, :N] if k in ("r0", "rC", "rT", "q") else v) for k, v in ens["params"].items()}


def cum_before(ens, t=T0, dt=1.0):
    """Cumulative emissions before step t [G] (exact: the emissions are multiples of 2^-10)."""
    return np.sum(ens["E"][:t] * dt, axis=0)


def _split(x):
    """An mpf as an fp64 pair (hi, lo), hi + lo = x to 2^-106."""
    hi = float(x)
    return hi, float(x - M(hi))


def _pack(rows):
    """A nested list [K][N] of mpf -> (hi, lo) fp64 arrays [K, N]."""
    pairs = [[_split(v) for v in row] for row in rows]
    return (np.array([[h for h, _ in row] for row in pairs]), np.array([[lo for _, lo in row] for row in pairs]))


@functools.lru_cache(maxsize=None)
def reference(kind, inverse=False):
    """The 50-digit step of every member of edge_ensemble(kind) at step T0.  Values as fp64 pairs (hi, lo) under their
    names ("C": [G, N], "T": [1, N], "R": [SP, N], "S": [2, N], and "E": [G, N] of the inverse step), scales as fp64 arrays
    under "sC", "sR", "sE", and "sT" / "sS" as pairs (A, B) (scale = A + B eps); "iirf" [G, N] fp64, un-clamped."""
    ens = edge_ensemble(kind)
    p, G, pools = ens["params"], ens["n_gas"], ens["pools"]
    mc = model_consts(p)
    cum = cum_before(ens)
    offs = np.concatenate([[0], np.cumsum(pools)])
    cols = []
    for m in range(N_MAX):
        r = [[p[k][g, m] for k in ("r0", "rC", "rT")] for g in range(G)]
        R = [list(ens["R0"][offs[g]:offs[g + 1], m]) for g in range(G)]
        args = (mc, r, list(p["q"][:, m]), R, list(ens["S0"][:, m]), list(cum))
        cols.append(step_inverse(*args, list(ens["target"]), ens["F_ext"][T0]) if inverse
                    else step_forward(*args, list(ens["E"][T0]), ens["F_ext"][T0]))
    flat = lambda per_gas: [v for gas in per_gas for v in gas]                                   # noqa: E731
    with mp.workdps(DPS):
        out = {"C": _pack([[c["C"][g] for c in cols] for g in range(G)]),
               "T": _pack([[c["T"] for c in cols]]),
               "R": _pack(list(zip(*[flat(c["R"]) for c in cols]))),
               "S": _pack([[c["S"][j] for c in cols] for j in range(2)]),
               "sC": np.array([[float(c["sC"][g]) for c in cols] for g in range(G)]),
               "sR": np.array([[float(v) for v in flat(c["sR"])] for c in cols]).T,
               "sT": (np.array([[float(c["sT"][0]) for c in cols]]), np.array([[float(c["sT"][1]) for c in cols]])),
               "sS": (np.array([[float(c["sS"][0][j]) for c in cols] for j in range(2)]),
                      np.array([[float(c["sS"][1][j]) for c in cols] for j in range(2)])),
               "iirf": np.array([[float(c["iirf"][g]) for c in cols] for g in range(G)])}
        if inverse:
            out["E"] = _pack([[c["E"][g] for c in cols] for g in range(G)])
            out["sE"] = np.array([[float(c["sE"][g]) for c in cols] for g in range(G)])
    return out


def scale_of(ref, name, eps):
    s = ref["s" + name]
    return s[0] + s[1] * eps if isinstance(s, tuple) else s


def err_units(got, ref, name, eps, N=None):
    """|got - reference| / (eps x scale), elementwise, for output `name` of the first N members; got: fp64 array [K, N]
    (fp32 results widened exactly).  got - hi is exact where the two are within a factor 2 (Sterbenz), which is where the
    figure matters."""
    got = np.asarray(got, dtype=np.float64)
    got = got.reshape(-1, got.shape[-1])
    N = got.shape[-1] if N is None else N
    hi, lo = ref[name]
    return np.abs((got - hi[:, :N]) - lo[:, :N]) / (eps * scale_of(ref, name, eps)[:, :N])
