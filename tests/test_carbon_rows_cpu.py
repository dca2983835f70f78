"""Carbon rows without a GPU (include/fiveeq.h, "CARBON ROWS"): the symbols and their refusals on the host, the NumPy twin
(fiveeqscm_amd/_carbon_host.py) against the oracle's alpha and cumulative emissions, its exact identities and its exact fma,
and the wrapper's refusals, each raised before any GPU call."""
import ctypes
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

import carbon_reference as cref
from fiveeqscm_amd import _capi, _carbon_host as twin, carbon
from fiveeqscm_amd import params as prm
from oracle import fiveeq_oracle as npo

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import fiveeq_cases as cases  # noqa: E402

N_STEPS = 60


def test_symbols_are_exported_and_bound_and_the_abi_stands():
    lib = _capi.load()
    for name in ("fiveeq_carbon_rows_f64", "fiveeq_carbon_rows_f32", "fiveeq_carbon_rows_tile", "fiveeq_carbon_rows_unroll",
                 "fiveeq_carbon_rows_yrows"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES
    assert len(_capi.SIGNATURES["fiveeq_carbon_rows_f64"][1]) == 27
    assert lib.fiveeq_abi_version() == _capi.ABI_VERSION == 13
    assert lib.fiveeq_sizeof_model() == ctypes.sizeof(_capi.Model) == 448
    assert [lib.fiveeq_carbon_rows_tile(b) for b in (8, 4, 2)] == [512, 1024, 0]
    assert all(lib.fiveeq_carbon_rows_unroll(w, s) >= 1 for w in (0, 1) for s in (0, 1)) and lib.fiveeq_carbon_rows_yrows() >= 1
    assert any(p.endswith("fiveeq_carbon.hpp") for p in _capi.SOURCES), "the new header is not under the stamped source hash"
    with open(os.path.join(os.path.dirname(_capi.SOURCES[0]), "Makefile")) as fh:
        assert "fiveeq_carbon.hpp" in fh.read()


def _call(lib, sfx="f64", **kw):
    """fiveeq_carbon_rows_* on fake (never dereferenced) pointers: a valid call of 4 rows x 8 members of the 4 + 1 + 1 layout
    asking for the airborne fraction of every gas, with the arguments of `kw` replaced."""
    P = 0x1000
    a = dict(n_rows=4, n=8, ld=8, rows=P, c_row=24, c_gas=8, T=None, t_row=8, steps=P, drive=P, cum_end=P, n_steps=10, r=None,
             conc_mask=0, gas_mask=7, airborne=None, cumE=None, uptake=None, fraction=P, iirf=None, alpha=None, sink=None, ld_out=8,
             cum_io=None, ga_io=None)
    a.update(kw)
    m = prm.make_model(prm.default_params("multigas"))
    p = lambda v: None if v is None else ctypes.c_void_p(v)                      # noqa: E731
    fn = getattr(lib, f"fiveeq_carbon_rows_{sfx}")
    return fn(ctypes.byref(m), a["n_rows"], a["n"], a["ld"], p(a["rows"]), a["c_row"], a["c_gas"], p(a["T"]), a["t_row"], p(a["steps"]),
              p(a["drive"]), p(a["cum_end"]), a["n_steps"], p(a["r"]), a["conc_mask"], a["gas_mask"], p(a["airborne"]), p(a["cumE"]),
              p(a["uptake"]), p(a["fraction"]), p(a["iirf"]), p(a["alpha"]), p(a["sink"]), a["ld_out"], p(a["cum_io"]), p(a["ga_io"]), None)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_every_refusal_returns_on_the_host_with_a_message(sfx):
    """Each call must come back with its error code before anything is launched: the pointers are fake, and the test runs
    without a GPU."""
    lib = _capi.load()
    P = 0x1000
    for kw, text in [
        (dict(alpha=P, r=P), "need T_rows"), (dict(iirf=P, T=P), "need the r rows"), (dict(sink=P), "needs ga_io"),
        (dict(conc_mask=2), "need cum_io"), (dict(cum_end=None), "need cum_end"), (dict(conc_mask=8), "conc_mask=8"),
        (dict(gas_mask=0), "gas_mask=0"), (dict(gas_mask=8), "gas_mask=8"), (dict(n_rows=-1), "n_rows=-1"), (dict(n=0), "n_members=0"),
        (dict(ld=7), "ld=7"), (dict(ld_out=7), "ld_out=7"), (dict(c_row=7), "c_row_stride=7"), (dict(c_gas=-7), "|c_gas_stride|=7"),
        (dict(alpha=P, r=P, T=P, t_row=7), "t_row_stride=7"), (dict(n_steps=0), "n_steps=0"), (dict(rows=None), "rows is NULL"),
        (dict(steps=None), "steps is NULL"), (dict(drive=None), "drive is NULL"), (dict(fraction=P + 1), "aligned"),
        (dict(steps=P + 2), "steps must be 4-byte aligned"),
    ]:
        assert _call(lib, sfx, **kw) == _capi.E_INVALID, kw
        assert text in lib.fiveeq_last_error().decode(), (kw, lib.fiveeq_last_error().decode())
    # no row: nothing to do, and nothing is launched (airborne of a driven gas needs no state)
    assert _call(lib, sfx, n_rows=0, rows=None, steps=None) == _capi.OK
    assert _call(lib, sfx, n_rows=0, conc_mask=6, fraction=None, airborne=P) == _capi.OK


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_twins_fma_is_one_rounding_of_the_exact_value(dtype):
    rng = np.random.default_rng(4)
    a, b, c = (rng.normal(size=400).astype(dtype) for _ in range(3))
    c[:50] = (-a[:50] * b[:50]).astype(dtype)                                   # heavy cancellation: the product's low bits survive
    got = twin.fma(a, b, c, dtype)
    assert got.dtype == dtype
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = float(got[i])
        lo, hi = float(np.nextafter(got[i], dtype(-np.inf))), float(np.nextafter(got[i], dtype(np.inf)))
        assert abs(exact - Fraction(near)) <= min(abs(exact - Fraction(lo)), abs(exact - Fraction(hi))), i
    assert np.isnan(twin.fma(np.array([np.nan, 1.0]), 2.0, 3.0, dtype)[0]) and twin.fma(np.array([0.0]), -1.0, 0.0, dtype)[0] == 0


def _golden(kind):
    p, N = cases.members(kind)
    E = cases.scenario(kind)[:N_STEPS]
    return p, N, E


def test_twin_alpha_against_the_oracles_alpha_of_the_next_step():
    """alpha at the row of step t, formed from the oracle's own C and T of step t, is the alpha the oracle uses at step t + 1:
    1e-10 relative, the project's fp64 criterion (the only difference: the rounding of C0 + sum of the pools)."""
    p, N, E = _golden("multigas")
    G = 3
    out = npo.run(E, p, N, keep=("C", "T", "alpha"))
    got = twin.carbon_rows_host(out["C"], np.arange(N_STEPS), p, r=cref.r_rows(p, G, N), drive=E, dt=1.0, T_rows=out["T"],
                                want=("alpha", "iirf"))
    ref = out["alpha"][1:]
    err = np.abs(got["alpha"][:-1] - ref) / np.abs(ref)
    print("worst relative difference of alpha:", err.max())
    assert err.max() <= 1e-10


def test_twin_cumE_of_a_concentration_driven_run_against_the_oracle():
    p, N, E = _golden("multigas")
    G = 3
    conc = npo.run(E, p, N)["C"][:, :, 0]                                       # a plausible pathway: member 0's own
    out = npo.run_inverse(conc, p, N)
    got = twin.carbon_rows_host(out["E"], np.arange(N_STEPS), p, drive=conc, dt=1.0, concentration_gases=(0, 1, 2), want=("cumE",))
    err = np.abs(got["cumE"][-1] - out["cumE"]) / np.abs(out["cumE"])
    print("worst relative difference of cumE:", err.max())
    assert err.max() <= 1e-10
    assert np.array_equal(got["cum_end"], got["cumE"][-1])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_exact_identities_of_an_emission_driven_gas(dtype):
    case = cref.synthetic(3, 7, 11, dtype)
    got = cref.host(case, twin.WANT)
    assert all(got[w].dtype == dtype and got[w].shape == (7, 3, 11) for w in twin.WANT)
    with np.errstate(all="ignore"):
        assert np.array_equal(got["uptake"], got["cumE"] - got["airborne"])
        assert np.array_equal(got["fraction"], got["airborne"] / got["cumE"])
    table = twin.cum_end_table(case["drive"][:, :3], 1.0)[case["steps"]].astype(dtype)
    assert np.array_equal(got["cumE"], np.broadcast_to(table[:, :, None], (7, 3, 11)))
    # ... which is column 3 + g of the NEXT step of the run's own drive table
    from fiveeqscm_amd.emissions import make_drive
    drive = make_drive(case["drive"][:, :3])
    assert np.array_equal(carbon.cum_end_table(case["drive"][:, :3], 1.0)[:-1], drive[1:, 3:6])
    # two calls with the state carried are one call
    a = cref.host(case, twin.WANT, rows=slice(0, 3))
    b = cref.host(case, twin.WANT, rows=slice(3, 7), cum0=a["cum_end"], airborne0=a["airborne_end"])
    assert all(np.array_equal(np.concatenate([a[w], b[w]]), got[w], equal_nan=True) for w in twin.WANT)


def test_wrapper_refusals_are_raised_before_any_gpu_call():
    """Host tensors throughout: every ValueError comes before the TypeError that host rows earn, so none of them reached a GPU."""
    torch = pytest.importorskip("torch")
    p = prm.default_params("multigas")
    rows, T = torch.zeros((3, 3, 4), dtype=torch.float64), torch.zeros((3, 4), dtype=torch.float64)
    r = torch.zeros((9, 4), dtype=torch.float64)
    kw = dict(r=r, drive=np.zeros((8, 3)), dt=1.0)
    with pytest.raises(ValueError, match="want"):
        carbon.carbon_rows(rows, [0, 1, 2], p, want=("fraction", "flux"), **kw)
    with pytest.raises(ValueError, match="want"):
        carbon.carbon_rows(rows, [0, 1, 2], p, want=(), **kw)
    with pytest.raises(ValueError, match="need T_rows"):
        carbon.carbon_rows(rows, [0, 1, 2], p, want=("alpha",), **kw)
    with pytest.raises(ValueError, match=r"the sink flux needs rows of consecutive model steps; row 0 holds step 0, row 1 step 2"):
        carbon.carbon_rows(rows, [0, 2, 3], p, want=("sink",), **kw)
    with pytest.raises(ValueError, match="concentration-driven gas needs rows of consecutive"):
        carbon.carbon_rows(rows, [0, 2, 3], p, want=("cumE",), concentration_gases=(1,), **kw)
    with pytest.raises(ValueError, match="rows hold 2 gases, params 3"):
        carbon.carbon_rows(rows[:, :2], [0, 1, 2], p, **kw)
    with pytest.raises(ValueError, match="gases="):
        carbon.carbon_rows(rows, [0, 1, 2], p, gases=(0, 3), **kw)
    with pytest.raises(ValueError, match="concentration_gases"):
        carbon.carbon_rows(rows, [0, 1, 2], p, concentration_gases=(5,), **kw)
    with pytest.raises(ValueError, match="steps"):
        carbon.carbon_rows(rows, [0, 1], p, **kw)
    # non-consecutive steps are fine where nothing is carried: the call gets as far as the host rows
    with pytest.raises(TypeError, match="no CPU fallback"):
        carbon.carbon_rows(rows, [0, 2, 3], p, want=("fraction", "alpha"), T_rows=T, **kw)
