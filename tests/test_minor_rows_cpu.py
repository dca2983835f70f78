"""Per-member minor-gas forcing rows (include/fiveeq.h "MINOR-GAS FORCING ROWS"), the parts that need no GPU: the entry points
and the unchanged ABI, the C ABI's refusals in their order, the NumPy twin against step_minor_gases and against an independent
scalar statement (tests/minor_reference.py) bit for bit, its invariance under row and member splits, the grouping of more than
eight species in both precisions, into=, and the wrappers' refusals."""
import ctypes

import numpy as np
import pytest

import fiveeqscm_amd
from fiveeqscm_amd import _capi, minor_gases
from fiveeqscm_amd.minor_gases import minor_gas_rows_host, step_minor_gases
import minor_reference as ref


def test_the_new_symbols_are_exported_and_bound_and_the_abi_stays():
    lib = _capi.load()
    for sfx in ("f64", "f32"):
        name = "fiveeq_minor_rows_" + sfx
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
        assert len(_capi.SIGNATURES[name][1]) == 13
    assert lib.fiveeq_abi_version() == 13 and lib.fiveeq_sizeof_model() == 448          # additive: nothing existing changed
    assert any(p.endswith("fiveeq_minor.hpp") for p in _capi.SOURCES)
    assert fiveeqscm_amd.minor_gas_rows is minor_gases.minor_gas_rows
    assert fiveeqscm_amd.minor_gas_rows_host is minor_gas_rows_host
    assert {"minor_gas_rows", "minor_gas_rows_host"} <= set(fiveeqscm_amd.__all__)


# ---- the C ABI's refusals ---------------------------------------------------------------------------------------------------
_C = (ctypes.c_double * 8)(*([1.0] * 8))


def _minor(lib, sfx="f64", K=3, n=8, ld=8, n_rows=4, dt=1.0, c=_C, emis=0x1000, tau=0x2000, eff=0x3000, R=0x4000, rows=0x5000,
           acc=0):
    vp = ctypes.c_void_p
    cp = ctypes.cast(c, vp) if c is not None else None
    return getattr(lib, "fiveeq_minor_rows_" + sfx)(K, n, ld, n_rows, dt, cp, vp(emis), vp(tau), vp(eff), vp(R), vp(rows), acc, None)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_minor_rows_refuses_bad_arguments_before_any_launch(sfx):
    """Every pointer here is an address nothing lies at: a call that launched would fault, a refused one returns."""
    lib = _capi.load()
    bad_c = (ctypes.c_double * 8)(1.0, 1.0, float("inf"), 1.0, 1.0, 1.0, 1.0, 1.0)
    nan_c = (ctypes.c_double * 8)(1.0, float("nan"), 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)
    cases = [
        (dict(K=0), "n_species=0 outside 1..8"), (dict(K=9), "n_species=9 outside 1..8"), (dict(K=-1), "n_species=-1"),
        (dict(n=0), "n_members=0 outside"), (dict(n=2 ** 31, ld=2 ** 31), "n_members=2147483648 outside"),
        (dict(n=9), "ld=8 < n_members=9"),
        (dict(n_rows=-1), "n_rows=-1 must be >= 0"),
        (dict(dt=0.0), "dt=0 must be finite and > 0"), (dict(dt=-1.0), "dt=-1 must be"), (dict(dt=float("inf")), "dt=inf must be"),
        (dict(dt=float("nan")), "must be finite and > 0"),
        (dict(c=None), "c is NULL"), (dict(c=bad_c), "c[2]=inf is not finite"), (dict(c=nan_c), "c[1]="),
        (dict(acc=2), "accumulate=2 must be 0 or 1"), (dict(acc=-1), "accumulate=-1 must be 0 or 1"),
        (dict(emis=0), "emis is NULL"), (dict(tau=0), "tau is NULL"), (dict(eff=0), "eff is NULL"), (dict(R=0), "R is NULL"),
        (dict(rows=0), "rows is NULL"),
        (dict(emis=0x1004), "emis must be 8-byte"), (dict(tau=0x2001), "tau must be"), (dict(eff=0x3002), "eff must be"),
        (dict(R=0x4004), "R must be 8-byte"), (dict(rows=0x5001), "rows must be"),
    ]
    for kw, needle in cases:
        rc = _minor(lib, sfx, **kw)
        msg = lib.fiveeq_last_error().decode()
        assert rc == _capi.E_INVALID and needle in msg, (kw, rc, msg)
    # the order: of two bad arguments the earlier one in the documented order names itself
    order = [(dict(K=0), "n_species"), (dict(n=0), "n_members=0"), (dict(n=9), "ld=8"), (dict(n_rows=-1), "n_rows"),
             (dict(dt=0.0), "dt="), (dict(c=bad_c), "c[2]"), (dict(acc=2), "accumulate"), (dict(tau=0), "is NULL"),
             (dict(rows=0x5001), "aligned")]
    for i, (kw, needle) in enumerate(order):
        for later, _ in order[i + 1:]:
            assert _minor(lib, sfx, **{**later, **kw}) == _capi.E_INVALID and needle in lib.fiveeq_last_error().decode(), (kw, later)
    assert _minor(lib, sfx, n_rows=0) == _capi.OK                                        # no rows: nothing launched
    assert _minor(lib, sfx, n_rows=0, rows=0) == _capi.E_INVALID                         # ... after the checks
    if sfx == "f32":
        assert _minor(lib, sfx, n_rows=0, tau=0x2004, eff=0x3004, rows=0x5004) == _capi.OK     # 4-byte rows of fp32


# ---- the twin ---------------------------------------------------------------------------------------------------------------
def _case(K, n, n_steps=12, seed=0):
    rng = np.random.default_rng(1000 * K + n + seed)
    t = np.arange(n_steps)[:, None]
    E = rng.uniform(0.5, 3.0, (1, K)) * (1.0 + 0.1 * t) * np.where(rng.random((n_steps, K)) < 0.15, -0.3, 1.0)
    E[n_steps // 2] = 0.0                                                                # a year without emissions
    tau = rng.uniform(1.5, 250.0, (K, 1)) * rng.uniform(0.7, 1.3, (K, n))
    eff = rng.uniform(0.01, 0.5, (K, 1)) * rng.uniform(0.8, 1.2, (K, n))
    c = rng.uniform(0.05, 0.4, K)
    R0 = rng.uniform(0.0, 5.0, (K, n))
    return E, tau, c, eff, R0


def test_shared_parameters_are_step_minor_gases_bit_for_bit():
    """tau and eff shared by the members: the twin's R after every step (walked through R0=, one row at a time) is
    step_minor_gases' concentration above C0 = 0 bit for bit, and its forcing is the ordered sum of the scalar statement."""
    K, n, n_steps = 5, 3, 12
    E, tau, c, eff, R0 = _case(K, n)
    tau, eff, R0 = tau[:, 0], eff[:, 0], R0[:, 0]
    conc, _ = step_minor_gases(E, tau, c, eff, C0=0.0, R0=R0)
    R, rows = R0, []
    for t in range(n_steps):
        out = minor_gas_rows_host(E[t:t + 1], tau, c, eff, n, R0=R)
        R = out.R
        assert out.species == K and np.array_equal(R, np.repeat(conc[t][:, None], n, 1)), t
        rows.append(out.rows[0])
    full = lambda x: np.repeat(x[:, None], n, 1)                                      # noqa: E731
    want, want_R = ref.rows_scalar(E, c, full(tau), full(eff), full(R0), em1=full(np.expm1(-1.0 / tau)))
    assert np.array_equal(np.array(rows), np.array(want)) and np.array_equal(R, np.array(want_R))
    whole = minor_gas_rows_host(E, tau, c, eff, n, R0=R0)
    assert np.array_equal(whole.rows, np.array(want)) and np.array_equal(whole.R, R)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("K", [1, 3, 8, 17])
def test_twin_equals_the_scalar_statement_and_any_split(K, dtype):
    n, n_steps = 13, 12
    E, tau, c, eff, R0 = _case(K, n)
    f32 = dtype == np.float32
    tq = tau.astype(dtype).astype(np.float64)
    em1 = np.expm1(-1.0 / tq)
    whole = minor_gas_rows_host(E, tau, c, eff, n, R0=R0, dtype=dtype)
    assert np.array_equal(R0, _case(K, n)[4])                                            # the caller's R0 is not advanced
    want, want_R = ref.rows_scalar(E, c, tau, eff, R0, em1=em1, f32=f32)
    assert whole.rows.dtype == dtype and whole.rows.shape == (n_steps, n) and whole.R.shape == (K, n)
    assert np.array_equal(whole.rows, np.array(want, dtype=dtype)) and np.array_equal(whole.R, np.array(want_R))
    assert np.array_equal(minor_gas_rows_host(E, tau, c, eff, n, R0=R0, dtype=dtype, em1=em1).rows, whole.rows)
    # member splits: rows of the design sliced to the shard, and rows given for the shard
    for lo, hi in ((0, 5), (5, 6), (6, 13), (4, 4)):
        part = minor_gas_rows_host(E, tau, c, eff, n, lo, hi, R0=R0, dtype=dtype)
        assert np.array_equal(part.rows, whole.rows[:, lo:hi]) and np.array_equal(part.R, whole.R[:, lo:hi]), (lo, hi)
        shard = minor_gas_rows_host(E, tau[:, lo:hi], c, eff[:, lo:hi], n, lo, hi, R0=R0[:, lo:hi], dtype=dtype)
        assert np.array_equal(shard.rows, part.rows)
    # row splits through R0=
    for cuts in ((5,), (1, 2, 11), tuple(range(1, n_steps))):
        parts, R = [], R0
        for a, b in zip((0,) + cuts, cuts + (n_steps,)):
            out = minor_gas_rows_host(E[a:b], tau, c, eff, n, R0=R, dtype=dtype)
            parts.append(out.rows)
            R = out.R
        assert np.array_equal(np.concatenate(parts), whole.rows) and np.array_equal(R, whole.R), cuts
        if K <= 8:                                   # (one group: the scalar statement's cut is the same walk)
            assert ref.rows_scalar(E, c, tau, eff, R0, em1=em1, f32=f32, cuts=cuts)[0] == want


def test_seventeen_species_fp64_is_one_ordered_sum_and_fp32_rounds_at_the_group_ends():
    K, n, n_steps = 17, 4, 6
    E, tau, c, eff, R0 = _case(K, n, n_steps)
    # fp64: R of every species after every step from step_minor_gases member by member, summed in species order from 0.0
    out = minor_gas_rows_host(E, tau, c, eff, n, R0=R0)
    out32 = minor_gas_rows_host(E, tau, c, eff, n, R0=R0, dtype=np.float32)
    t32, e32 = tau.astype(np.float32).astype(np.float64), eff.astype(np.float32).astype(np.float64)
    for m in range(n):
        conc, _ = step_minor_gases(E, tau[:, m], c, eff[:, m], C0=0.0, R0=R0[:, m])
        conc32, _ = step_minor_gases(E, t32[:, m], c, e32[:, m], C0=0.0, R0=R0[:, m])
        for t in range(n_steps):
            acc = 0.0
            for k in range(K):
                acc = acc + eff[k, m] * conc[t, k]
            assert out.rows[t, m] == acc, (t, m)
            acc = np.float32(0.0)
            for g in ((0, 8), (8, 16), (16, 17)):                                         # three roundings
                wide = float(acc)
                for k in range(*g):
                    wide = wide + e32[k, m] * conc32[t, k]
                acc = np.float32(wide)
            assert out32.rows[t, m] == acc, (t, m)
    assert out32.rows.dtype == np.float32 and not np.array_equal(out32.rows.astype(np.float64), out.rows)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_into_adds_onto_given_rows(dtype):
    K, n, n_steps = 9, 5, 12
    E, tau, c, eff, R0 = _case(K, n)
    start = np.random.default_rng(3).normal(0.0, 0.4, (n_steps, n)).astype(dtype)
    start[0, 0] = -0.0
    rows = start.copy()
    out = minor_gas_rows_host(E, tau, c, eff, n, R0=R0, into=rows, dtype=dtype)
    assert out.rows is rows
    em1 = np.expm1(-1.0 / tau.astype(dtype).astype(np.float64))
    want, _ = ref.rows_scalar(E, c, tau, eff, R0, em1=em1, start=start, f32=dtype == np.float32)
    assert np.array_equal(rows, np.array(want, dtype=dtype))
    assert not np.array_equal(rows, start)
    with pytest.raises(ValueError, match="into"):
        minor_gas_rows_host(E, tau, c, eff, n, into=np.zeros((n_steps, n + 1), dtype=dtype), dtype=dtype)
    with pytest.raises(ValueError, match="into"):
        minor_gas_rows_host(E, tau, c, eff, n, into=np.zeros((n_steps, n), dtype=np.float16), dtype=dtype)


def test_the_wrappers_refuse_bad_lifetimes_emissions_and_shapes():
    K, n = 3, 6
    E, tau, c, eff, R0 = _case(K, n)
    calls = [minor_gas_rows_host]
    try:
        import torch  # noqa: F401
        calls.append(minor_gases.minor_gas_rows)     # refuses on the host before anything is uploaded: no GPU needed
    except ImportError:
        pass
    for fn in calls:
        for bad in (0.0, -1.0, np.inf, np.nan):
            t = tau.copy()
            t[1, 2] = bad
            with pytest.raises(ValueError, match="lifetime"):
                fn(E, t, c, eff, n)
        for bad in (np.inf, np.nan):
            e = E.copy()
            e[3, 1] = bad
            with pytest.raises(ValueError, match="emissions"):
                fn(e, tau, c, eff, n)
        with pytest.raises(ValueError, match="lifetime"):
            fn(E, tau[:, :4], c, eff, n)
        with pytest.raises(ValueError, match="rad_eff"):
            fn(E, tau, c, eff[:2], n)
        with pytest.raises(ValueError, match="emis2conc"):
            fn(E, tau, c[:2], eff, n)
        with pytest.raises(ValueError, match="members"):
            fn(E, tau, c, eff, n, lo=4, hi=7)
        with pytest.raises(ValueError, match="dt="):
            fn(E, tau, c, eff, n, dt=0.0)
        with pytest.raises(ValueError, match="K >= 1"):
            fn(np.zeros((4, 0)), tau, c, eff, n)
    with pytest.raises(ValueError, match="float32"):                                     # a lifetime that is 0 in fp32
        minor_gas_rows_host(E, np.full(K, 1e-60), c, eff[:, 0], n, dtype=np.float32)
    empty = minor_gas_rows_host(E[:0], tau, c, eff, n)
    assert empty.rows.shape == (0, n) and np.array_equal(empty.R, np.zeros((K, n)))
    assert minor_gas_rows_host(E, tau, c, eff, n, lo=2, hi=2).rows.shape == (12, 0)
    one = minor_gas_rows_host(E[:, 0], 12.0, 0.1, 0.2, n)                                # one species: scalars
    assert one.species == 1 and np.array_equal(one.rows, minor_gas_rows_host(E[:, :1], [12.0], [0.1], [0.2], n).rows)
