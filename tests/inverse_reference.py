"""The cases, the target series and the anchored-step yardstick of the concentration-driven (inverse) form.

TEST INFRASTRUCTURE, beside tests/step_reference.py (whose step_inverse() is the reference here).  A multi-step comparison of
an fp32 run with an fp64 oracle needs an allowance for the growth of the error that nobody can derive, so none is written:

    ANCHORED STEPS   the program under test (the device, the NumPy oracle, a deliberately wrong restatement) runs ONE step at a
                     time; before each step the state it holds itself (R, S, cum) is read back (fp32 words widen exactly), the
                     guarded 50-digit step is evaluated from exactly that state, and the step's outputs E, T, R, S and cum are
                     held to the single-step bound in units of eps(dtype) x scale.  Errors do not accumulate.
    ONE ARITHMETIC   the one-launch run equals the chain of single-step launches bit for bit (tests/test_inverse_gpu.py).

CASES.  One per compiled pool layout (a model drawn as tests/test_engine_gpu.py::test_all_compiled_layouts_match_oracle draws
it: random pool fractions and time-scales; ra, f, PI_conc, emis2conc of the default set), dt cycling through 1, 0.5, 0.25, 2;
and the default "multigas" and "co2" sets (with the 1e6-year pool) at dt = 1 and dt = 0.5.  Each case has M = 16 distinct
members (params.sample_ensemble, every per-member input rounded to fp32); an ensemble of N members is the case TILED: member
i is member i mod 16.  Targets and F_ext are multiples of 2^-10, so one reference serves fp64 and fp32 and the kernel's
drv[g] - C0 sees the target that was meant.

THE TARGET SERIES, per gas C0 + SHAPE x amplitude: equal to C0 at step 0 (from a zero state: E = 0 exactly), rising, held flat,
falling through C0, sitting below it (E < 0, cum < 0), and returning.  The amplitudes are small against C0, so every member
stays far from the C <= 0 guard and from the iIRF clamp (tests/test_inverse_cpu.py asserts it): no member sits at a decision.
"""
import functools

import mpmath as mp
import numpy as np

import step_reference as sr
from fiveeqscm_amd import params as prm
from oracle import fiveeq_oracle as npo

M = 16                                                     # distinct members of a case
N_STEPS = 12
LAYOUTS = ((1,), (2,), (3,), (4,), (1, 1), (4, 1), (4, 4), (1, 1, 1), (4, 1, 1), (4, 4, 1), (4, 4, 4))
DTS = (1.0, 0.5, 0.25, 2.0)
SHAPE = np.array([0.0, 0.5, 3.0, 8.0, 8.0, 5.0, 1.0, -3.0, -6.0, -6.0, -2.0, 6.0])
AMPLITUDE = np.array([2.0, 24.0, 1.5])                     # ppm CO2, ppb CH4, ppb N2O per unit of SHAPE
OUTPUTS = ("E", "T", "R", "S", "cum")


def layout_name(pools):
    return "{" + str(pools[0]) + "}" if len(pools) == 1 else "+".join(str(p) for p in pools)


DEFAULT_CASES = {"multigas dt=1": ("multigas", 1.0), "multigas dt=0.5": ("multigas", 0.5),
                 "co2 dt=1": ("co2", 1.0), "co2 dt=0.5": ("co2", 0.5)}
CASES = tuple(layout_name(p) for p in LAYOUTS) + tuple(DEFAULT_CASES)


def _q10(x):
    """Rounded to a multiple of 2^-10."""
    return np.round(np.asarray(x, dtype=np.float64) * 1024.0) / 1024.0


def target_series(C0, n_steps=N_STEPS):
    """[n_steps, G]: C0 + SHAPE x AMPLITUDE (the 12-step shape repeated), multiples of 2^-10."""
    C0 = np.asarray(C0, dtype=np.float64).reshape(-1)
    shape = np.resize(SHAPE, n_steps)
    return _q10(C0[None, :] + shape[:, None] * AMPLITUDE[None, :C0.size])


def f_ext_series(n_steps=N_STEPS):
    """[n_steps]: non-zero, changing sign, multiples of 2^-10."""
    return _q10(0.6 * np.cos(1.3 * np.arange(n_steps) + 0.4))


def _layout_model(pools, rng):
    base = prm.default_params("multigas")
    G = len(pools)
    a, tau = np.zeros((G, 4)), np.ones((G, 4))
    for g, P in enumerate(pools):
        w = rng.uniform(0.2, 1.0, size=P)
        a[g, :P] = w / w.sum()
        tau[g, :P] = np.sort(rng.uniform(2.0, 400.0, size=P))[::-1]
    return {"a": a, "tau": tau, "r0": [30.0, 9.0, 60.0][:G], "rC": [0.015, 0.0, 0.001][:G], "rT": [3.0, -0.3, 0.5][:G],
            "ra": base["ra"][:G], "PI_conc": base["PI_conc"][:G], "emis2conc": base["emis2conc"][:G], "f": base["f"][:G],
            "iirf_max": base["iirf_max"], "d": base["d"], "q": base["q"]}


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: params (r0, rC, rT [G, M], q [2, M], fp32-exact; the rest shared), dt, pools, n_gas, target [N_STEPS, G],
    F_ext [N_STEPS], mc (step_reference.model_consts).  Treat as read-only (cached)."""
    if name in DEFAULT_CASES:
        kind, dt = DEFAULT_CASES[name]
        base, seed = prm.default_params(kind), 20261018 + list(DEFAULT_CASES).index(name)
    else:
        k = [layout_name(p) for p in LAYOUTS].index(name)
        rng = np.random.default_rng(11)
        for pools in LAYOUTS[:k + 1]:                      # one stream for all layouts, as the engine test draws them
            base = _layout_model(pools, rng)
        dt, seed = DTS[k % len(DTS)], 3 + k
    p = {key: v for key, v in prm.sample_ensemble(base, M, seed=seed).items() if key not in ("TCR", "ECS")}
    for key in ("r0", "rC", "rT", "q"):
        p[key] = sr._f32(p[key])
    return dict(name=name, params=p, dt=dt, pools=prm.pools_of(p), n_gas=prm.n_gas_of(p), target=target_series(p["PI_conc"]),
                F_ext=f_ext_series(), mc=sr.model_consts(p, dt))


def tiled_params(c, N):
    """The parameter dict of N members: member i is member i mod M of the case."""
    idx = np.arange(N) % M
    return {k: (v[:, idx] if k in ("r0", "rC", "rT", "q") else v) for k, v in c["params"].items()}


def _gas_rows(c, R):
    offs = np.concatenate([[0], np.cumsum(c["pools"])])
    return [np.asarray(R, dtype=np.float64)[offs[g]:offs[g + 1]] for g in range(c["n_gas"])]


def step_reference(c, R, S, cum, t):
    """The 50-digit inverse step t of the case's M members from the state R [SP, M], S [2, M], cum [G, M] (fp64 arrays: what
    the program under test holds before the step).  Values as fp64 pairs (hi, lo) under "E", "cum", "C" [G, M], "T" [1, M],
    "R" [SP, M], "S" [2, M]; scales under "sE", "scum", "sC", "sR" and the pairs "sT", "sS" (scale = A + B eps); "iirf" [G, M]
    un-clamped: the layout of step_reference.reference(), for step_reference.err_units()."""
    p, G = c["params"], c["n_gas"]
    R, S, cum = _gas_rows(c, R), np.asarray(S, dtype=np.float64), np.asarray(cum, dtype=np.float64)
    cols = []
    for m in range(M):
        r = [[p[k][g, m] for k in ("r0", "rC", "rT")] for g in range(G)]
        cols.append(sr.step_inverse(c["mc"], r, list(p["q"][:, m]), [list(Rg[:, m]) for Rg in R], list(S[:, m]),
                                    list(cum[:, m]), list(c["target"][t]), c["F_ext"][t]))
    flat = lambda per_gas: [v for gas in per_gas for v in gas]                                   # noqa: E731
    per_gas = lambda key: [[col[key][g] for col in cols] for g in range(G)]                      # noqa: E731
    with mp.workdps(sr.DPS):
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


def units(got, ref, eps):
    """|got - ref| / (eps x scale) per output: {"E": [G, M], "T": [1, M], "R": [SP, M], "S": [2, M], "cum": [G, M]}.  Where the
    scale is zero (the pools of step 0: a zero state and E = 0) the reference is exactly zero: 0 units for exactly that, inf
    for anything else.  A NaN result gives inf."""
    out = {}
    for name in OUTPUTS:
        g = np.asarray(got[name], dtype=np.float64).reshape(ref[name][0].shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            u = sr.err_units(g, ref, name, eps)
        u = np.where(sr.scale_of(ref, name, eps) == 0, np.where(g == ref[name][0], 0.0, np.inf), u)
        out[name] = np.where(np.isnan(u), np.inf, u)
    return out


# ---- programs under test on the CPU: the NumPy oracle, and restatements of its step that are wrong on purpose ----------------
def oracle_step(c, R, S, cum, t):
    """One step of oracle.fiveeq_oracle.run_inverse from the state given."""
    out = npo.run_inverse(c["target"][t:t + 1], c["params"], M, F_ext=c["F_ext"][t:t + 1], dt=c["dt"], R0=_gas_rows(c, R), S0=S,
                          cumE0=cum)
    return {"E": out["E"][0], "T": out["T"][0], "C": out["C"][0], "R": np.concatenate(out["R"]), "S": out["S"], "cum": out["cumE"]}


VARIANTS = ("cum += E without dt", "alpha from the shared cumulative emissions", "a tau c of the neighbouring pool")


def restated_step(c, R, S, cum, t, variant=None):
    """The oracle's inverse step written out (variant=None: its bits), or with one of the VARIANTS' mistakes:
    cum += E instead of E dt; alpha taken from the SHARED cumulative emissions (the drive column the forward form reads, here
    the ensemble mean of cum) instead of the member's own; the first pool's a tau c in the denominator taken from the next pool."""
    p, dt, G = c["params"], c["dt"], c["n_gas"]
    a, tau = np.atleast_2d(np.asarray(p["a"], dtype=np.float64)), np.atleast_2d(np.asarray(p["tau"], dtype=np.float64))
    C0, cc = np.asarray(p["PI_conc"], dtype=np.float64).reshape(G), np.asarray(p["emis2conc"], dtype=np.float64).reshape(G)
    f, ra = np.asarray(p["f"], dtype=np.float64).reshape(G, 3), np.asarray(p["ra"], dtype=np.float64).reshape(G)
    R, S, cum = [np.array(x) for x in _gas_rows(c, R)], np.array(S, dtype=np.float64), np.array(cum, dtype=np.float64)
    T_old = S[0] + S[1]
    F, E_out = np.zeros(M), np.empty((G, M))
    for g, P in enumerate(c["pools"]):
        ag, tg = a[g, :P], tau[g, :P]
        G_a = np.sum(R[g], axis=0) / cc[g]
        own = np.full(M, cum[g].mean()) if variant == VARIANTS[1] else cum[g]
        alpha = npo.alpha_val(own - G_a, G_a, T_old, p["r0"][g], p["rC"][g], p["rT"][g], ra[g], float(npo.g_0(a[g], tau[g])),
                              float(npo.g_1(a[g], tau[g])), float(p["iirf_max"]))
        at = alpha[None, :] * tg[:, None]
        em1 = np.expm1(-dt / at)
        atc = ag[:, None] * tg[:, None] * cc[g]
        if variant == VARIANTS[2] and P > 1:
            atc = atc.copy()
            atc[0] = atc[1]
        E = (np.sum(R[g] + R[g] * em1, axis=0) - (c["target"][t, g] - C0[g])) / (alpha * np.sum(atc * em1, axis=0))
        R[g] = R[g] + em1 * (R[g] - (ag[:, None] * (E[None, :] * cc[g])) * at)
        cum[g] = cum[g] + (E if variant == VARIANTS[0] else E * dt)
        F = F + npo.step_forc(C0[g] + np.sum(R[g], axis=0), C0[g], f[g])
        E_out[g] = E
    S, T = npo.step_temp(S, F + c["F_ext"][t], np.asarray(p["q"], dtype=np.float64), np.expm1(-dt / np.asarray(p["d"], dtype=np.float64)))
    return {"E": E_out, "T": T, "R": np.concatenate(R), "S": S, "cum": cum}


def anchored(c, step, eps=sr.EPS["f64"]):
    """`step` (oracle_step, restated_step, ...) run over the case's N_STEPS steps, one at a time from its own state (zero at
    step 0), each step measured against the 50-digit step from that state.  Returns (worst units per output over all steps
    and members, the per-step list of (outputs of the program, reference))."""
    SP, G = sum(c["pools"]), c["n_gas"]
    R, S, cum = np.zeros((SP, M)), np.zeros((2, M)), np.zeros((G, M))
    worst, steps = dict.fromkeys(OUTPUTS, 0.0), []
    for t in range(N_STEPS):
        ref = step_reference(c, R, S, cum, t)
        got = step(c, R, S, cum, t)
        for name, u in units(got, ref, eps).items():
            worst[name] = max(worst[name], float(u.max()))
        steps.append((got, ref))
        R, S, cum = got["R"], got["S"], got["cum"]
    return worst, steps


@functools.lru_cache(maxsize=None)
def oracle_anchored(name):
    """anchored(case(name), oracle_step), cached: the measurement of K and the trajectory the input conditions are checked on."""
    return anchored(case(name), oracle_step)
