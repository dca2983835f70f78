"""Forcing rows without a GPU (include/fiveeq.h, "FORCING ROWS"): the symbols and their refusals on the host, the NumPy twin
(fiveeqscm_amd/_diagnose_host.py) against the oracle's step_forc and against plain Python floats, the consecutive-steps check
and the unit constant."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

from fiveeqscm_amd import _capi, _diagnose_host as twin, diagnose
from fiveeqscm_amd import params as prm
from oracle import fiveeq_oracle as npo

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import fiveeq_cases as cases  # noqa: E402


def test_symbols_are_exported_and_bound_and_the_abi_stands():
    lib = _capi.load()
    for name in ("fiveeq_forcing_rows_f64", "fiveeq_forcing_rows_f32", "fiveeq_forcing_rows_tile"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES
    assert len(_capi.SIGNATURES["fiveeq_forcing_rows_f64"][1]) == 25
    assert lib.fiveeq_abi_version() == _capi.ABI_VERSION == 13
    assert lib.fiveeq_sizeof_model() == ctypes.sizeof(_capi.Model) == 448
    assert [lib.fiveeq_forcing_rows_tile(b) for b in (8, 4, 2)] == [512, 1024, 0]
    assert any(p.endswith("fiveeq_forcrows.hpp") for p in _capi.SOURCES), "the new header is not under the stamped source hash"
    with open(os.path.join(os.path.dirname(_capi.SOURCES[0]), "Makefile")) as fh:
        assert "fiveeq_forcrows.hpp" in fh.read()


def _call(lib, sfx="f64", model=None, **kw):
    """fiveeq_forcing_rows_* on fake (never dereferenced) pointers: a valid call of 4 rows x 8 members of the 4 + 1 + 1 layout
    asking for F, with the arguments of `kw` replaced."""
    P = 0x1000
    a = dict(n_rows=4, n=8, ld=8, C=P, c_row=24, c_gas=8, T=None, t_row=8, steps=P, drive=P, n_steps=10, q=P, fscale=None,
             n_fext=0, fext=None, F=P, Fg=None, N=None, H=None, ld_out=8, H_io=None, S_io=None, mism=None)
    a.update(kw)
    m = model if model is not None else prm.make_model(prm.default_params("multigas"))
    p = lambda v: None if v is None else ctypes.c_void_p(v)                      # noqa: E731
    fn = getattr(lib, f"fiveeq_forcing_rows_{sfx}")
    return fn(ctypes.byref(m), a["n_rows"], a["n"], a["ld"], p(a["C"]), a["c_row"], a["c_gas"], p(a["T"]), a["t_row"], p(a["steps"]),
              p(a["drive"]), a["n_steps"], p(a["q"]), p(a["fscale"]), a["n_fext"], p(a["fext"]), p(a["F"]), p(a["Fg"]), p(a["N"]),
              p(a["H"]), a["ld_out"], p(a["H_io"]), p(a["S_io"]), p(a["mism"]), None)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_every_refusal_returns_on_the_host_with_a_message(sfx):
    """Each call must come back with its error code before anything is launched: the pointers are fake, and the test runs
    without a GPU."""
    lib = _capi.load()
    P = 0x1000
    cases_ = [
        (dict(N=P), "need T_rows"),                                       # N without T rows
        (dict(H=P), "need T_rows"),                                       # H without T rows
        (dict(H_io=P), "need T_rows"),
        (dict(S_io=P, mism=P), "S_io (the replay) needs T_rows"),         # S_io without T rows
        (dict(S_io=P, T=P), "needs n_mismatch"),
        (dict(n_fext=5, fscale=P, fext=P), "n_fext=5 outside 0..4"),      # K > MAX_FEXT
        (dict(n_fext=-1), "n_fext=-1"),
        (dict(n_fext=2, fscale=P), "needs fext"),                         # scales without X
        (dict(n_fext=2, fext=P), "needs fscale"),                         # X without scales
        (dict(n_fext=2), "without fscale and fext"),
        (dict(c_row=7), "c_row_stride=7 < n_members=8"),                  # strides smaller than n_members
        (dict(c_gas=7), "|c_gas_stride|=7 < n_members=8"),
        (dict(c_gas=-7), "|c_gas_stride|=7 < n_members=8"),
        (dict(T=P, N=P, t_row=7), "t_row_stride=7 < n_members=8"),
        (dict(ld=7), "ld=7 < n_members=8"),
        (dict(ld_out=7), "ld_out=7 < n_members=8"),
        (dict(n=0), "n_members=0"),
        (dict(n_rows=-1), "n_rows=-1"),
        (dict(n_steps=0), "n_steps=0"),
        (dict(C=None), "C_rows is NULL"),
        (dict(steps=None), "steps is NULL"),
        (dict(drive=None), "drive is NULL"),
        (dict(q=None), "q is NULL"),
        (dict(C=P + 2), "aligned"),
        (dict(steps=P + 2), "steps must be 4-byte aligned"),
    ]
    for kw, needle in cases_:
        assert _call(lib, sfx, **kw) == _capi.E_INVALID, kw
        assert needle in lib.fiveeq_last_error().decode(), (kw, lib.fiveeq_last_error())
    # a pool layout outside fiveeq_layout_supported
    m = prm.make_model(prm.default_params("multigas"))
    m.gas[1].n_pools = 2
    m.gas[1].tau[1] = 1.0
    assert _call(lib, sfx, model=m) == _capi.E_UNSUPPORTED
    assert "no compiled kernel" in lib.fiveeq_last_error().decode()
    m = prm.make_model(prm.default_params("multigas"))
    m.dt = 0.0
    assert _call(lib, sfx, model=m) == _capi.E_INVALID
    # nothing to do is not an error, and launches nothing
    assert _call(lib, sfx, n_rows=0, C=None, steps=None) == _capi.OK


def _golden_C(kind):
    with open(os.path.join(HERE, "golden", "fiveeq_golden.json")) as fh:
        rec = json.load(fh)["cases"][kind]
    p, N = cases.members(kind)
    G = 1 if kind == "co2" else 3
    return p, np.array([float.fromhex(h) for h in rec["C"]]).reshape(len(cases.STEPS), G, N)


@pytest.mark.parametrize("kind", ["co2", "multigas"])
def test_twin_forcing_against_the_oracle_on_the_golden_members(kind):
    p, C = _golden_C(kind)
    C0 = np.asarray(p["PI_conc"], dtype=np.float64).reshape(-1)
    f = np.asarray(p["f"], dtype=np.float64).reshape(-1, 3)
    for g in range(C.shape[1]):
        ref = npo.step_forc(C[:, g], C0[g], f[g])
        got = twin.gas_forcing(C[:, g], C0[g], f[g])
        assert np.all(np.abs(got - ref) <= 1e-10 * np.abs(ref) + 1e-13), (kind, g)
    out = twin.forcing_rows_host(C, cases.STEPS, p, q=np.ones((2, C.shape[2])), F_ext=np.zeros(max(cases.STEPS) + 1), want=("F", "F_gas"))
    ref = sum(npo.step_forc(C[:, g], C0[g], f[g]) for g in range(C.shape[1]))
    assert np.all(np.abs(out["F"] - ref) <= 1e-10 * np.abs(ref) + 1e-13)


def test_twin_forcing_on_the_guard_values_and_nan():
    """C <= 0: no log term, sqrt C reads 0 (the term is -f3 sqrt C0); NaN propagates; C = C0 gives exactly 0."""
    C0 = 278.0
    for f in ([5.35, 0.0, 0.0], [0.0, 0.0, 0.036], [4.0, 1e-3, 0.05], [0.0, 2e-3, 0.0]):
        C = np.array([-3.0, 0.0, -0.0, C0, 1e-300, 400.0, np.nan])
        ref = npo.step_forc(C, C0, np.array(f))
        got = twin.gas_forcing(C, C0, f)
        ok = np.abs(got - ref) <= 1e-10 * np.abs(ref) + 1e-13
        assert np.all(ok[:6]) and np.isnan(got[6]) and np.isnan(ref[6]), (f, got, ref)
        for i in (0, 1, 2):                                     # the guard's values, spelt out: f2 (C - C0) - f3 sqrt C0
            want = f[1] * (C[i] - C0) + (f[2] * (0.0 - np.sqrt(C0)) if f[2] else 0.0)
            assert got[i] == want, (f, i)
        assert abs(got[3]) <= 1e-13
    got32 = twin.gas_forcing(np.array([400.0, -1.0], dtype=np.float32), C0, [5.35, 0.0, 0.036], np.float32)
    assert got32.dtype == np.float32 and abs(float(got32[0]) - float(npo.step_forc(np.array(400.0), C0, np.array([5.35, 0.0, 0.036])))) < 1e-5


def test_twin_scales_and_table_in_the_kernels_order():
    rng = np.random.default_rng(3)
    Fg = rng.normal(size=(5, 3, 7))
    fs = rng.uniform(0.5, 1.5, size=(5, 7))
    X = rng.normal(size=(5, 2))
    fe = rng.normal(size=5)
    got = twin.total_forcing(Fg, fe, fs, X)
    want = fe[:, None] + fs[3] * X[:, :1] + fs[4] * X[:, 1:2] + fs[0] * Fg[:, 0] + fs[1] * Fg[:, 1] + fs[2] * Fg[:, 2]
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=1e-15)
    assert np.array_equal(twin.total_forcing(Fg, fe), ((fe[:, None] + Fg[:, 0]) + Fg[:, 1]) + Fg[:, 2])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_twin_imbalance_and_heat_against_plain_python_floats_bit_for_bit(dtype):
    rng = np.random.default_rng(11)
    K, N, dt = 9, 5, 0.5
    F = rng.normal(2.0, 1.0, size=(K, N)).astype(dtype)
    T = rng.normal(1.0, 0.5, size=(K, N)).astype(dtype)
    q = rng.uniform(0.2, 0.6, size=(2, N)).astype(dtype)
    heat0 = rng.normal(size=N)
    Nn = twin.imbalance(F, T, q)
    H = twin.heat(Nn, dt, heat0)
    assert Nn.dtype == dtype and H.dtype == np.float64
    rnd = (lambda v: float(np.float32(v))) if dtype == np.float32 else float          # one rounding to the rows' precision
    for m in range(N):
        run = float(heat0[m])
        for k in range(K):
            # python floats are IEEE doubles; for fp32 rows every exact double result of two floats is rounded once to float,
            # which is the float operation's own rounding (the double result of +, -, / of two floats rounds innocuously)
            n = rnd(float(F[k, m]) - rnd(float(T[k, m]) / rnd(float(q[0, m]) + float(q[1, m]))))
            assert n == float(Nn[k, m]), (k, m)
            run = run + dt * n
            assert run == float(H[k, m]), (k, m)
    assert np.array_equal(twin.heat(Nn, dt)[0], dt * Nn[0].astype(np.float64))


def test_rows_of_non_consecutive_steps_are_refused_naming_the_gap():
    diagnose.check_consecutive([3, 4, 5, 6], "the heat uptake H")
    diagnose.check_consecutive([7], "the replay")
    with pytest.raises(ValueError, match=r"row 1 holds step 4, row 2 step 6"):
        diagnose.check_consecutive([3, 4, 6, 7, 9], "the heat uptake H")


def test_host_rows_are_a_type_error():
    torch = pytest.importorskip("torch")
    p = prm.default_params("co2")
    with pytest.raises(TypeError, match="no CPU fallback"):
        diagnose.forcing_rows(torch.zeros((2, 1, 4), dtype=torch.float64), [0, 1], p, q=torch.ones((2, 4), dtype=torch.float64),
                              F_ext=np.zeros(2), dt=1.0)


def test_the_unit_constant_against_its_derivation():
    seconds = 365.25 * 24 * 3600
    assert seconds == 31557600.0
    assert diagnose.W_YR_M2_TO_ZJ == 5.100656e14 * seconds / 1e21
    assert abs(diagnose.W_YR_M2_TO_ZJ - 16.0964) < 1e-4
