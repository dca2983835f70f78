"""Pulse response without a GPU (include/fiveeq.h, "PULSE RESPONSE"): the symbols and their refusals on the host,
pulse_experiment, the NumPy twin (fiveeqscm_amd/_pulse_host.py) against the closed forms of a linear one-pool model run by the
oracle, and the twin's sums against plain Python floats."""
import ctypes
import os

import numpy as np
import pytest

from fiveeqscm_amd import _capi, _pulse_host as twin, pulse
from fiveeqscm_amd import params as prm
from oracle import fiveeq_oracle as npo

EPS = np.finfo(np.float64).eps


# ---- 1. symbols ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound_and_the_abi_stands():
    lib = _capi.load()
    for name in ("fiveeq_pulse_response_f64", "fiveeq_pulse_response_f32", "fiveeq_max_pulses", "fiveeq_max_horizons"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES
    assert len(_capi.SIGNATURES["fiveeq_pulse_response_f64"][1]) == 29
    assert lib.fiveeq_abi_version() == _capi.ABI_VERSION == 13
    assert lib.fiveeq_sizeof_model() == ctypes.sizeof(_capi.Model) == 448
    assert lib.fiveeq_max_pulses() == _capi.MAX_PULSES == 3
    assert lib.fiveeq_max_horizons() == _capi.MAX_HORIZONS == 8
    names = [os.path.basename(p) for p in _capi.SOURCES]
    assert names[names.index("fiveeq_forcrows.hpp") + 1] == "fiveeq_pulse.hpp", "the new header is not under the stamped source hash"
    with open(os.path.join(os.path.dirname(_capi.SOURCES[0]), "Makefile")) as fh:
        assert "fiveeq_forcrows.hpp fiveeq_pulse.hpp" in fh.read()
    with open(os.path.join(os.path.dirname(_capi.SOURCES[0]), "fiveeq_device.hpp")) as fh:
        text = fh.read()
    assert text.index('#include "fiveeq_forcrows.hpp"') < text.index('#include "fiveeq_pulse.hpp"')


# ---- 2. refusals --------------------------------------------------------------------------------------------------------------
def _call(lib, sfx="f64", model=None, **kw):
    """fiveeq_pulse_response_* on fake (never dereferenced) device pointers: a valid call of 3 scenarios x 4 rows x 8 members of
    the 4 + 1 + 1 layout, two pulses, two horizons, with the arguments of `kw` replaced."""
    P = 0x1000
    a = dict(n_scen=3, n_rows=4, n=8, ld=8, C=P, c_scen=96, c_row=24, c_gas=8, T=P, t_scen=32, t_row=8, steps=P, drive=P, n_steps=10,
             fscale=None, n_fext=0, fext=None, base=0, n_pulses=2, pscen=(1, 2), pgas=(0, 1), n_hor=2, hor=(2, 4), row0=0, out=P,
             ld_out=8, io=P)
    a.update(kw)
    m = model if model is not None else prm.make_model(prm.default_params("multigas"))
    p = lambda v: None if v is None else ctypes.c_void_p(v)                      # noqa: E731
    arr = lambda v: None if v is None else (ctypes.c_int32 * len(v))(*v)          # noqa: E731
    fn = getattr(lib, f"fiveeq_pulse_response_{sfx}")
    return fn(ctypes.byref(m), a["n_scen"], a["n_rows"], a["n"], a["ld"], p(a["C"]), a["c_scen"], a["c_row"], a["c_gas"], p(a["T"]),
              a["t_scen"], a["t_row"], p(a["steps"]), p(a["drive"]), a["n_steps"], p(a["fscale"]), a["n_fext"], p(a["fext"]), a["base"],
              a["n_pulses"], arr(a["pscen"]), arr(a["pgas"]), a["n_hor"], arr(a["hor"]), a["row0"], p(a["out"]), a["ld_out"], p(a["io"]),
              None)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_every_refusal_returns_on_the_host_with_a_message(sfx):
    """Each call must come back with its error code before anything is launched: the pointers are fake, and the test runs
    without a GPU."""
    lib = _capi.load()
    P = 0x1000
    cases_ = [
        (dict(n_pulses=0), "n_pulses=0 outside 1..3"),
        (dict(n_pulses=4, pscen=(1, 2, 1, 2), pgas=(0, 1, 2, 0)), "n_pulses=4 outside 1..3"),
        (dict(n_hor=0), "n_horizons=0 outside 1..8"),
        (dict(n_hor=9, hor=tuple(range(1, 10))), "n_horizons=9 outside 1..8"),
        (dict(hor=(4, 2)), "strictly increasing"),
        (dict(hor=(2, 2)), "strictly increasing"),
        (dict(hor=(0, 2)), "row count >= 1"),
        (dict(pscen=(1, 0)), "pulse 1 names the base scenario 0"),
        (dict(base=1), "pulse 0 names the base scenario 1"),
        (dict(pscen=(1, 3)), "scenario 3 outside the scenarios 0..2"),
        (dict(pscen=(-1, 2)), "scenario -1 outside"),
        (dict(base=3), "base=3 outside"),
        (dict(base=-1), "base=-1 outside"),
        (dict(pgas=(0, 3)), "gas 3 outside the gases 0..2"),
        (dict(pgas=(-1, 1)), "gas -1 outside"),
        (dict(n_scen=1), "n_scen=1"),
        (dict(pscen=None), "pulse_scen / pulse_gas is NULL"),
        (dict(pgas=None), "pulse_scen / pulse_gas is NULL"),
        (dict(hor=None), "horizons is NULL"),
        (dict(c_row=7), "c_row_stride=7 < n_members=8"),                  # strides that overlap
        (dict(c_gas=7), "|c_gas_stride|=7 < n_members=8"),
        (dict(c_gas=-7), "|c_gas_stride|=7 < n_members=8"),
        (dict(c_scen=7), "|c_scen_stride|=7 < n_members=8"),
        (dict(c_scen=0), "|c_scen_stride|=0 < n_members=8"),
        (dict(t_row=7), "t_row_stride=7 < n_members=8"),
        (dict(t_scen=-7), "|t_scen_stride|=7 < n_members=8"),
        (dict(ld=7), "ld=7 < n_members=8"),
        (dict(ld_out=7), "ld_out=7 < n_members=8"),
        (dict(n=0), "n_members=0"),
        (dict(n=-3), "n_members=-3"),
        (dict(n=1 << 31, ld=1 << 31, ld_out=1 << 31), "outside 1..2^31-1"),
        (dict(n_rows=-1), "n_rows=-1"),
        (dict(row0=-1), "row0=-1"),
        (dict(row0=(1 << 31) - 2), "row0=2147483646 with n_rows=4"),
        (dict(n_steps=0), "n_steps=0"),
        (dict(n_fext=5, fscale=P, fext=P), "n_fext=5 outside 0..4"),
        (dict(n_fext=-1), "n_fext=-1"),
        (dict(n_fext=2, fscale=P), "needs fext"),
        (dict(n_fext=2, fext=P), "needs fscale"),
        (dict(n_fext=2), "without fscale and fext"),
        (dict(C=None), "C_rows is NULL"),
        (dict(T=None), "T_rows is NULL"),
        (dict(steps=None), "steps is NULL"),
        (dict(drive=None), "drive is NULL"),
        (dict(out=None), "out is NULL"),
        (dict(io=None), "io is NULL"),
        (dict(C=P + 2), "aligned"),
        (dict(T=P + 2), "aligned"),
        (dict(steps=P + 2), "steps must be 4-byte aligned"),
        (dict(out=P + 4), "out and io must be 8-byte aligned"),
        (dict(io=P + 4), "out and io must be 8-byte aligned"),
    ]
    for kw, needle in cases_:
        assert _call(lib, sfx, **kw) == _capi.E_INVALID, kw
        assert needle in lib.fiveeq_last_error().decode(), (kw, lib.fiveeq_last_error())
    m = prm.make_model(prm.default_params("multigas"))
    m.gas[1].n_pools = 2
    m.gas[1].tau[1] = 1.0
    assert _call(lib, sfx, model=m) == _capi.E_UNSUPPORTED
    assert "no compiled kernel" in lib.fiveeq_last_error().decode()
    m = prm.make_model(prm.default_params("multigas"))
    m.dt = 0.0
    assert _call(lib, sfx, model=m) == _capi.E_INVALID
    # nothing to do is not an error, and launches nothing
    assert _call(lib, sfx, n_rows=0, C=None, T=None, steps=None) == _capi.OK


# ---- 3. pulse_experiment ------------------------------------------------------------------------------------------------------
def test_pulse_experiment_shapes_and_where_the_pulse_lands():
    rng = np.random.default_rng(2)
    E = rng.uniform(1.0, 2.0, size=(30, 3))
    exp = pulse.pulse_experiment(E, 7, [(0, 100.0), (2, -3.0)], 20, dt=0.5)
    assert exp.emissions.shape == (3, 30, 3) and exp.emissions.dtype == np.float64
    assert exp.scenario_names == ("base", "pulse:0", "pulse:2")
    assert exp.output_steps == range(7, 27) and exp.t0 == 7 and exp.pulses == ((0, 100.0), (2, -3.0))
    assert np.array_equal(exp.emissions[0], E)
    for p, (g, size) in enumerate(exp.pulses):
        d = exp.emissions[1 + p] - E
        assert d[7, g] == (E[7, g] + size / 0.5) - E[7, g]
        d[7, g] = 0.0
        assert not d.any(), "the pulse lands in step t0 of the named gas only"
    assert pulse.pulse_experiment(E, 0, [(1, 1.0)], 30).output_steps == range(0, 30)          # the whole run


def test_pulse_experiment_refusals():
    E = np.ones((30, 3))
    for t0, pulses, n_rows, needle in (
            (-1, [(0, 1.0)], 5, "t0=-1"),
            (26, [(0, 1.0)], 5, "t0 + n_rows <= n_steps"),
            (0, [(0, 1.0)], 0, "n_rows >= 1"),
            (0, [(0, 0.0)], 5, "not zero"),
            (0, [(0, np.inf)], 5, "finite"),
            (0, [(0, np.nan)], 5, "finite"),
            (0, [(0, 1.0), (0, 2.0)], 5, "not distinct"),
            (0, [(3, 1.0)], 5, "gas 3 outside"),
            (0, [], 5, "0 pulses"),
            (0, [(0, 1.0), (1, 1.0), (2, 1.0), (1, 2.0)], 5, "4 pulses")):
        with pytest.raises(ValueError, match=needle.replace("+", r"\+")):
            pulse.pulse_experiment(E, t0, pulses, n_rows)
    with pytest.raises(ValueError, match="n_steps, G"):
        pulse.pulse_experiment(np.ones(30), 0, [(0, 1.0)], 5)


def test_host_rows_are_a_type_error():
    torch = pytest.importorskip("torch")
    p = prm.default_params("co2")
    with pytest.raises(TypeError, match="no CPU fallback"):
        pulse.pulse_response(torch.zeros((2, 2, 1, 4), dtype=torch.float64), torch.zeros((2, 2, 4), dtype=torch.float64), [0, 1], p,
                             F_ext=np.zeros(2), dt=1.0, base=0, pulses=[(1, 0, 1.0)], horizons=[1])


# ---- 4. the analytic known answer ---------------------------------------------------------------------------------------------
def _linear_params(N, rng):
    """One gas with one pool, no feedback on the time scale (rC = rT = ra = 0: alpha is a constant per member) and a forcing
    linear in C (f = (0, f2, 0)): the model is linear, the response to a pulse independent of the baseline."""
    return {"a": [[1.0, 0.0, 0.0, 0.0]], "tau": [[40.0, 1.0, 1.0, 1.0]], "r0": rng.uniform(28.0, 36.0, size=(1, N)),
            "rC": [0.0], "rT": [0.0], "ra": [0.0], "PI_conc": [1.0], "emis2conc": [0.5], "f": [[0.0, 0.015, 0.0]],
            "iirf_max": 97.0, "d": [239.0, 4.1], "q": rng.uniform(0.2, 0.6, size=(2, N))}


@pytest.mark.parametrize("dt", [1.0, 0.5])
def test_twin_on_oracle_runs_against_the_closed_forms_of_the_linear_model(dt):
    """dR_k = -expm1(-dt / (alpha tau)) tau alpha c (size / dt) exp(-k dt / (alpha tau)), dF_k = f2 dR_k, I_F(n) the geometric sum,
    dT the two-box recursion on dF.

    THE TOLERANCE 1e-12 |ref| + n_h * 4 eps max|X| (X = F, T or C, whichever the quantity is a difference of).  The floor is the
    cancellation floor of the rows themselves: the oracle's value X of a row is a handful of rounded fp64 operations on
    quantities of its own size (F = f2 (C - C0) with C = C0 + R and C0 well below R here: one rounding of C, one of the
    product; T = S_0 + S_1: one rounding) — at most 2 eps |X| from the real-number value of the same expression, so a
    difference of two rows is within 4 eps max|X| of the real difference, whatever cancels in it, and a sum of n_h of them
    within n_h times that.  The rounding the oracle's STATE gathers over the steps (R and S are recursions) is relative to
    the state and is what the 1e-12 |ref| term is for: t0 + n steps of about eps each stay far below it."""
    rng = np.random.default_rng(7)
    N, n_steps, t0, n_rows, size = 6, 140, 5, 130, 300.0
    horizons = (1, 2, 20, 100, 130)
    p = _linear_params(N, rng)
    E = rng.uniform(0.5, 3.0, size=(n_steps, 1))
    exp = pulse.pulse_experiment(E, t0, [(0, size)], n_rows, dt=dt)
    runs = [npo.run(exp.emissions[s], p, N, dt=dt, keep=("C", "T", "F")) for s in range(2)]
    rows = slice(t0, t0 + n_rows)
    C = np.stack([r["C"][rows] for r in runs])
    T = np.stack([r["T"][rows] for r in runs])
    F_oracle = np.stack([r["F"][rows] for r in runs])
    out, state = twin.pulse_response_host(C, T, exp.output_steps, p, F_ext=np.zeros(n_steps), base=0, pulses=[(1, 0)],
                                          horizons=horizons)
    # the closed forms, per member
    a, tau = np.asarray(p["a"]), np.asarray(p["tau"])
    alpha = float(npo.g_0(a[0], tau[0])) * np.exp(np.minimum(p["r0"][0], p["iirf_max"]) / float(npo.g_1(a[0], tau[0])))
    at = alpha * tau[0, 0]
    c, f2 = p["emis2conc"][0], p["f"][0][1]
    k = np.arange(n_rows)[:, None]
    dR = -np.expm1(-dt / at) * at * c * (size / dt) * np.exp(-k * dt / at)                       # [n_rows, N]
    n_h = np.asarray(horizons)[:, None]
    I_C = at * c * (size / dt) * -np.expm1(-n_h * dt / at)                                       # the geometric sum
    em1_d = np.expm1(-dt / np.asarray(p["d"]))
    S = np.zeros((2, N))
    dT = np.empty((n_rows, N))
    for i in range(n_rows):
        S = S + em1_d[:, None] * (S - p["q"] * (f2 * dR[i])[None, :])
        dT[i] = S[0] + S[1]
    ref = {0: f2 * I_C, 1: np.stack([dT[:h].sum(0) for h in horizons]), 2: I_C, 3: dT[n_h[:, 0] - 1], 4: dR[n_h[:, 0] - 1]}
    scale = {0: np.abs(F_oracle).max(), 1: np.abs(T).max(), 2: np.abs(C).max(), 3: np.abs(T).max(), 4: np.abs(C).max()}
    worst = 0.0
    for i, name in enumerate(("I_F", "I_T", "I_C", "dT", "dC")):
        rows_in = n_h if i < 3 else 1
        tol = 1e-12 * np.abs(ref[i]) + rows_in * 4 * EPS * scale[i]
        err = np.abs(out[i, 0] - ref[i])
        worst = max(worst, float((err / tol).max()))
        assert np.all(err <= tol), (name, float((err / tol).max()))
    # the oracle-against-closed-form residual itself, row by row, stays within the per-row part of that tolerance
    for got, want, sc in ((F_oracle[1] - F_oracle[0], f2 * dR, scale[0]), (C[1, :, 0] - C[0, :, 0], dR, scale[2]), (T[1] - T[0], dT, scale[1])):
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want) + 4 * EPS * sc)
    assert np.array_equal(state[:, 0], out[0:3, 0, -1]), "the carried sums are the sums at the last row"
    print(f"\n  twin vs closed forms, dt={dt}: worst error / tolerance {worst:.3f}")


# ---- 5. the twin's sums are exact ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_twin_sums_against_plain_python_floats_bit_for_bit(dtype):
    rng = np.random.default_rng(11)
    S, K, G, N = 4, 9, 3, 5
    F = rng.normal(2.0, 1.0, size=(S, K, N)).astype(dtype)
    T = rng.normal(1.0, 0.5, size=(S, K, N)).astype(dtype)
    C = rng.uniform(300.0, 900.0, size=(S, K, G, N)).astype(dtype)
    pulses, base, horizons = [(3, 2), (0, 0), (2, 1)], 1, (1, 4, 9, 12)
    state0 = rng.normal(size=(3, 3, N))
    out, state = twin.pulse_sums(F, T, C, base, pulses, horizons, state0, row0=0)
    assert out.dtype == np.float64 and out.shape == (5, 3, 4, N) and np.isnan(out[:, :, 3]).all()
    for p, (s, g) in enumerate(pulses):
        for m in range(N):
            run = [float(state0[i, p, m]) for i in range(3)]
            for k in range(K):
                # python floats are IEEE doubles; a float32 widens to one exactly
                d = (float(F[s, k, m]) - float(F[base, k, m]), float(T[s, k, m]) - float(T[base, k, m]),
                     float(C[s, k, g, m]) - float(C[base, k, g, m]))
                run = [run[i] + d[i] for i in range(3)]
                if k + 1 in horizons:
                    h = horizons.index(k + 1)
                    assert [float(out[i, p, h, m]) for i in range(5)] == run + [d[1], d[2]], (p, m, k)
            assert [float(state[i, p, m]) for i in range(3)] == run
    # the rows split over two calls, the sums carried: the bits of one call
    a, sa = twin.pulse_sums(F[:, :5], T[:, :5], C[:, :5], base, pulses, horizons, state0)
    b, sb = twin.pulse_sums(F[:, 5:], T[:, 5:], C[:, 5:], base, pulses, horizons, sa, row0=5)
    merged = np.where(np.isnan(b), a, b)
    assert np.array_equal(merged, out, equal_nan=True) and np.array_equal(sb, state)
