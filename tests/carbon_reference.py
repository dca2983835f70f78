"""What the carbon-rows tests share (tests/test_carbon_rows_cpu.py, tests/test_carbon_rows_gpu.py): rows made by hand for the
twin and the device alike, the engine's r-row layout, and the bound on alpha taken from the bound the project pins for fe_exp."""
import numpy as np

import math_reference as mref
from fiveeqscm_amd import _carbon_host as twin
from fiveeqscm_amd import params as prm

PREC = {np.float64: "f64", np.float32: "f32"}
# alpha = g0 * fe_exp(iirf * inv_g1) against g0 * exp(x) formed exactly at the SAME x = fl(iirf * inv_g1) (one IEEE product, which
# NumPy performs as the device does): fe_exp is held to CAPS[prec, "exp"] ulp (tests/test_math_edges_gpu.py), and the issue
# grants one ulp for each of the two products.  An ulp is at most 2^-mant of its value, so relative to the exact alpha:
ALPHA_REL = {p: (mref.CAPS[(p, "exp")] + 2.0) * 2.0 ** -mref.MANT[p] for p in ("f64", "f32")}


def r_rows(p, G, N):
    """[3 G, N] fp64: r0, rC, rT of gas 0, then of gas 1, ... — EnsembleEngine.r's layout."""
    rows = [np.broadcast_to(np.asarray(p[k], dtype=np.float64).reshape(G, -1), (G, N))[g] for g in range(G) for k in ("r0", "rC", "rT")]
    return np.array(rows)


def synthetic(G, K, N, dtype, conc=(), seed=0, first_step=2, n_extra=3):
    """Rows made by hand, the same for the twin and the device: dict with params, steps (consecutive from first_step), rows
    [K, G, N] (C near C0 (1 .. 1.6) for an emission-driven gas, emissions for a gas of `conc`), T [K, N], r [3 G, N], the host
    drive table [n_steps, 8] fp64 (emissions, or targets for a gas of `conc`) — all already rounded to dtype where the device
    holds them in the rows' precision."""
    rng = np.random.default_rng(1000 * seed + 10 * G + len(conc))
    base = prm.default_params("co2" if G == 1 else "multigas")
    p = prm.sample_ensemble_shard(base, N)
    C0 = np.asarray(base["PI_conc"], dtype=np.float64).reshape(G)
    n_steps = first_step + K + n_extra
    drive = np.zeros((n_steps, 8))
    rows = np.empty((K, G, N))
    for g in range(G):
        if g in conc:
            drive[:, g] = C0[g] * (1.0 + 0.6 * np.sort(rng.random(n_steps)))
            rows[:, g] = rng.normal(3.0, 4.0, size=(K, N))
        else:
            drive[:, g] = rng.normal(5.0, 3.0, size=n_steps)
            rows[:, g] = C0[g] * (1.0 + 0.6 * rng.random((K, N)))
    return dict(params=p, steps=np.arange(first_step, first_step + K), rows=rows.astype(dtype), T=rng.normal(1.2, 0.8, size=(K, N)).astype(dtype),
                r=r_rows(p, G, N).astype(dtype), drive=drive.astype(dtype).astype(np.float64), conc=tuple(conc), dt=1.0)


def host(case, want, rows=slice(None), members=slice(None), **kw):
    """The twin on (a row / member range of) a synthetic case."""
    return twin.carbon_rows_host(case["rows"][rows][..., members], case["steps"][rows], case["params"], r=case["r"][:, members],
                                 drive=case["drive"], dt=case["dt"], T_rows=case["T"][rows][..., members],
                                 concentration_gases=case["conc"], want=want, **kw)


def alpha_excess(alpha, iirf, params, gases, dt, dtype, max_points=600):
    """max over (a sample of) the elements of |alpha - g0 exp(x)| / (ALPHA_REL |g0 exp(x)|), x = fl(iirf * inv_g1) in dtype, the
    exact value by tests/math_reference.py: <= 1 means inside the bound.  alpha, iirf [K, n_sel, N] host arrays of dtype."""
    t = np.dtype(dtype).type
    prec = PREC[t]
    kg, _, _ = twin.kernel_constants(params, dt, t)
    worst = 0.0
    for slot, g in enumerate(gases):
        ii = np.asarray(iirf[:, slot], dtype=t).reshape(-1)
        al = np.asarray(alpha[:, slot], dtype=t).reshape(-1)
        if ii.size > max_points:
            pick = np.random.default_rng(5).choice(ii.size, max_points, replace=False)
            ii, al = ii[pick], al[pick]
        x = (ii * kg[g]["inv_g1"]).astype(t)
        ex = mref.reference("exp", x, prec)
        ref = np.longdouble(kg[g]["g0"]) * (ex.hi.astype(np.longdouble) + np.asarray(ex.lo, dtype=np.longdouble))
        err = np.abs(al.astype(np.longdouble) - ref) / (np.longdouble(ALPHA_REL[prec]) * np.abs(ref))
        worst = max(worst, float(err.max()))
    return worst
