"""Per-member aerosol forcing rows (include/fiveeq.h "AEROSOL FORCING ROWS"), the parts that need no GPU: the entry points and
the unchanged ABI, the C ABI's refusals in their order, the NumPy twin against an independent scalar statement
(tests/aerosol_reference.py) bit for bit, its invariance under row and member splits, the all-zero rows of emissions equal to
base, into=, the calibration helper, the fp64 twin against a 50-digit evaluation within the derived bound, and the wrappers'
refusals."""
import ctypes
import math

import numpy as np
import pytest

import fiveeqscm_amd
from fiveeqscm_amd import _capi, aerosols
from fiveeqscm_amd.aerosols import aci_scale_for_target_host, aerosol_rows_host
import aerosol_reference as ref


def test_the_new_symbols_are_exported_and_bound_and_the_abi_stays():
    lib = _capi.load()
    for sfx in ("f64", "f32"):
        name = "fiveeq_aerosol_rows_" + sfx
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
        assert len(_capi.SIGNATURES[name][1]) == 13
    assert lib.fiveeq_abi_version() == 13 and lib.fiveeq_sizeof_model() == 448          # additive: nothing existing changed
    names = [p.rsplit("/", 1)[-1] for p in _capi.SOURCES]
    assert names[names.index("fiveeq_minor.hpp") + 1] == "fiveeq_aerosol.hpp", "the new header is not under the stamped source hash"
    for name in ("aerosol_rows", "aerosol_rows_host", "aci_scale_for_target", "aci_scale_for_target_host"):
        assert getattr(fiveeqscm_amd, name) is getattr(aerosols, name) and name in fiveeqscm_amd.__all__, name
    assert aerosols.AEROSOL_MAX == 8


# ---- the C ABI's refusals ---------------------------------------------------------------------------------------------------
_B = (ctypes.c_double * 8)(*([1.0] * 8))


def _aer(lib, sfx="f64", K=3, mask=0b101, n=8, ld=8, n_rows=4, base=_B, emis=0x1000, ari=0x2000, shape=0x3000, beta=0x4000,
         rows=0x5000, acc=0):
    vp = ctypes.c_void_p
    bp = ctypes.cast(base, vp) if base is not None else None
    return getattr(lib, "fiveeq_aerosol_rows_" + sfx)(K, mask, n, ld, n_rows, bp, vp(emis), vp(ari), vp(shape), vp(beta), vp(rows),
                                                      acc, None)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_aerosol_rows_refuses_bad_arguments_before_any_launch(sfx):
    """Every pointer here is an address nothing lies at: a call that launched would fault, a refused one returns."""
    lib = _capi.load()
    inf_b = (ctypes.c_double * 8)(1.0, 1.0, float("inf"), 1.0, 1.0, 1.0, 1.0, 1.0)
    nan_b = (ctypes.c_double * 8)(1.0, float("nan"), 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)
    neg_b = (ctypes.c_double * 8)(-0.5, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)
    cases = [
        (dict(K=0, mask=0), "n_species=0 outside 1..8"), (dict(K=9), "n_species=9 outside 1..8"), (dict(K=-1), "n_species=-1"),
        (dict(mask=0b1000), "aci_mask=0x8 has a bit outside the 3 species"), (dict(mask=-1), "aci_mask="),
        (dict(K=8, mask=0x100), "aci_mask=0x100"),
        (dict(n=0), "n_members=0 outside"), (dict(n=2 ** 31, ld=2 ** 31), "n_members=2147483648 outside"),
        (dict(n=9), "ld=8 < n_members=9"),
        (dict(n_rows=-1), "n_rows=-1 must be >= 0"),
        (dict(base=None), "base is NULL"), (dict(base=inf_b), "base[2]=inf must be finite and >= 0"), (dict(base=nan_b), "base[1]="),
        (dict(base=neg_b), "base[0]=-0.5 must be finite and >= 0"),
        (dict(acc=2), "accumulate=2 must be 0 or 1"), (dict(acc=-1), "accumulate=-1 must be 0 or 1"),
        (dict(emis=0), "emis is NULL"), (dict(ari=0), "ari is NULL"), (dict(shape=0), "shape is NULL"), (dict(beta=0), "beta is NULL"),
        (dict(rows=0), "rows is NULL"),
        (dict(emis=0x1004), "emis must be 8-byte"), (dict(ari=0x2001), "ari must be"), (dict(shape=0x3002), "shape must be"),
        (dict(beta=0x4001), "beta must be"), (dict(rows=0x5001), "rows must be"),
    ]
    for kw, needle in cases:
        rc = _aer(lib, sfx, **kw)
        msg = lib.fiveeq_last_error().decode()
        assert rc == _capi.E_INVALID and needle in msg, (kw, rc, msg)
    # the order: of two bad arguments the earlier one in the documented order names itself
    order = [(dict(K=0), "n_species"), (dict(mask=0b1000), "aci_mask"), (dict(n=0), "n_members=0"), (dict(n=9), "ld=8"),
             (dict(n_rows=-1), "n_rows"), (dict(base=neg_b), "base[0]"), (dict(acc=2), "accumulate"), (dict(ari=0), "is NULL"),
             (dict(rows=0x5001), "aligned")]
    for i, (kw, needle) in enumerate(order):
        for later, _ in order[i + 1:]:
            assert _aer(lib, sfx, **{**later, **kw}) == _capi.E_INVALID and needle in lib.fiveeq_last_error().decode(), (kw, later)
    assert _aer(lib, sfx, n_rows=0) == _capi.OK                                          # no rows: nothing launched
    assert _aer(lib, sfx, n_rows=0, rows=0) == _capi.E_INVALID                           # ... after the checks
    assert _aer(lib, sfx, n_rows=0, mask=0, shape=0, beta=0) == _capi.OK                 # no cloud term: shape and beta may be NULL
    assert _aer(lib, sfx, n_rows=0, mask=0b010, shape=0) == _capi.E_INVALID              # any bit: both are required
    if sfx == "f32":
        assert _aer(lib, sfx, n_rows=0, ari=0x2004, shape=0x3004, beta=0x4004, rows=0x5004) == _capi.OK   # 4-byte rows of fp32


# ---- the twin ---------------------------------------------------------------------------------------------------------------
def _sqrt_log(Y):
    """A stand-in for the logarithm that IEEE 754 pins to the bit in NumPy and in math alike."""
    return np.sqrt(Y)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_twin_equals_the_scalar_statement_and_any_split(K, dtype):
    n, f32 = 13, dtype == np.float32
    for in_aci in ref.masks(K):
        for base_zero in (True, False):
            E, base, ari, shape, beta, _ = ref.case(K, n, in_aci, base_zero)
            whole = aerosol_rows_host(E, base, ari, shape, beta, n, aci=in_aci, log=_sqrt_log, dtype=dtype)
            want = ref.rows_scalar(E, base, ari, shape, beta, in_aci, log=math.sqrt, f32=f32)
            assert whole.rows.dtype == dtype and whole.rows.shape == (ref.N_ROWS, n) and whole.species == K
            assert np.array_equal(whole.rows, np.array(want, dtype=dtype)), (in_aci, base_zero)
            assert (whole.y is None) == (not any(in_aci))
            if any(in_aci):
                assert whole.y.shape == (ref.N_ROWS, n) and (whole.y[ref.ZERO_ROW] == 1.0).all() and (whole.y >= 1.0).all()
                assert (whole.y0 == 1.0).all() == base_zero
            # member splits: rows of the design sliced to the shard, and rows given for the shard
            for lo, hi in ((0, 5), (5, 6), (6, 13), (4, 4)):
                part = aerosol_rows_host(E, base, ari, shape, beta, n, lo, hi, aci=in_aci, log=_sqrt_log, dtype=dtype)
                assert np.array_equal(part.rows, whole.rows[:, lo:hi]), (lo, hi)
                shard = aerosol_rows_host(E, base, ari[:, lo:hi], shape[:, lo:hi], beta[lo:hi], n, lo, hi, aci=in_aci, log=_sqrt_log,
                                          dtype=dtype)
                assert np.array_equal(shard.rows, part.rows)
            # row splits: no state to carry
            for cuts in ((5,), (1, 2, 11), tuple(range(1, ref.N_ROWS))):
                parts = [aerosol_rows_host(E[a:b], base, ari, shape, beta, n, aci=in_aci, log=_sqrt_log, dtype=dtype).rows
                         for a, b in zip((0,) + cuts, cuts + (ref.N_ROWS,))]
                assert np.array_equal(np.concatenate(parts), whole.rows), cuts
            assert ref.rows_scalar(E, base, ari, shape, beta, in_aci, log=math.sqrt, f32=f32, cuts=(5,)) == want
    # a value per species, a scalar beta, aci=None for every species
    E, base, ari, shape, beta, _ = ref.case(K, n, [True] * K, False)
    full = lambda x: np.repeat(x[:, None], n, 1)                                       # noqa: E731
    shared = aerosol_rows_host(E, base, ari[:, 0], shape[:, 0], 0.7, n, log=_sqrt_log, dtype=dtype)
    assert np.array_equal(shared.rows, aerosol_rows_host(E, base, full(ari[:, 0]), full(shape[:, 0]), np.full(n, 0.7), n,
                                                         aci=[True] * K, log=_sqrt_log, dtype=dtype).rows)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_emissions_equal_to_base_give_rows_of_plus_zero(dtype):
    """L is formed by the operations that formed L0, e = +0 for every species: every sign of ari and beta, every mask."""
    K, n = 3, 13
    for in_aci in ref.masks(K):
        _, base, ari, shape, beta, _ = ref.case(K, n, in_aci, False)
        E = np.repeat(base[None], ref.N_ROWS, 0)
        out = aerosol_rows_host(E, base, ari, shape, beta, n, aci=in_aci, dtype=dtype)
        assert (ari > 0).any() and (ari < 0).any() and (beta < 0).any() and (beta == 0).any()
        assert (out.rows == 0).all() and not np.signbit(out.rows).any(), in_aci
        want = ref.rows_scalar(E, base, ari, shape, beta, in_aci, f32=dtype == np.float32)
        assert all(v == 0.0 and math.copysign(1.0, v) == 1.0 for row in want for v in row)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_into_adds_onto_given_rows(dtype):
    K, n = 3, 5
    in_aci = [True, False, True]
    E, base, ari, shape, beta, _ = ref.case(K, n, in_aci, False)
    start = np.random.default_rng(3).normal(0.0, 0.4, (ref.N_ROWS, n)).astype(dtype)
    start[0, 0] = -0.0
    rows = start.copy()
    out = aerosol_rows_host(E, base, ari, shape, beta, n, aci=in_aci, into=rows, log=_sqrt_log, dtype=dtype)
    assert out.rows is rows
    want = ref.rows_scalar(E, base, ari, shape, beta, in_aci, log=math.sqrt, start=start, f32=dtype == np.float32)
    assert np.array_equal(rows, np.array(want, dtype=dtype)) and not np.array_equal(rows, start)
    with pytest.raises(ValueError, match="into"):
        aerosol_rows_host(E, base, ari, shape, beta, n, into=np.zeros((ref.N_ROWS, n + 1), dtype=dtype), dtype=dtype)
    with pytest.raises(ValueError, match="into"):
        aerosol_rows_host(E, base, ari, shape, beta, n, into=np.zeros((ref.N_ROWS, n), dtype=np.float16), dtype=dtype)


# ---- accuracy ---------------------------------------------------------------------------------------------------------------
def test_fp64_twin_against_fifty_digits_within_the_derived_bound(capsys):
    """|F - F_mp| <= error_bound per member and step (tests/aerosol_reference.py derives it from the operation list: every
    listed operation within 0.5 ulp, np.log within 1 ulp):
        gamma_{K+2} A + |beta| (2 gamma'_{K+3} + 2 c u (|ln y| + |ln y0| + 2 gamma'_{K+3}) + u V) + u |beta| V + u |F|,  c = 1,
    A = sum_k |ari_k| |E_k - base_k|, V = |ln y - ln y0| + the logarithms' error, u = 2^-53, times 1.001.  For this case
    (K = 8, every mask, every member class: y = 1, y - 1 < 1e-9, y around sqrt(2) and 2, y > 1e6) the bound lies between
    4e-18 and 1.3e-14 W m-2 where it is not 0 (it is 0, and the twin exact, for a member without ari and without cloud term)."""
    K, n = 8, 9
    worst = 0.0
    for in_aci in ref.masks(K):
        for rot in range(3):
            E, base, ari, shape, beta, _ = ref.case(K, n, in_aci, rot == 1, rot)
            got = aerosol_rows_host(E, base, ari, shape, beta, n, aci=in_aci).rows
            F = ref.rows_mp(E, base, ari, shape, beta, in_aci)
            for m in range(n):
                for t in range(ref.N_ROWS):
                    bound = ref.error_bound(E[t], base, ari[:, m], shape[:, m], beta[m], in_aci, log_ulps=1)
                    err = float(abs(got[t, m] - F[t][m]))
                    assert err <= bound and bound < 1e-13, (in_aci, rot, t, m, err, bound)
                    worst = max(worst, err / bound if bound else 0.0)
    with capsys.disabled():
        print(f"\naerosol rows fp64 twin: worst |F - F_mp| / bound = {worst:.3f}")
    assert worst > 0


# ---- the calibration --------------------------------------------------------------------------------------------------------
def test_calibration_reproduces_the_target_within_one_division_and_one_product():
    """beta = fl(target / mean) and the window mean of the member's cloud term is beta * mean: fl(beta mean) = target (1 + d1)
    (1 + d2) with |d| <= u = 2^-53, so |fl(beta mean) - target| <= (2 u + u^2) |target|.  `mean` is the helper's own: the
    unit-beta rows of the window added in ascending order and divided once.  The rows run with that beta then average to the
    target within the roundings of their own operations, with W = sum_t |beta v_t| over the n_w = b - a rows: w = fl(beta v)
    per row (u W in all), the subtraction from +0 exact, n_w - 1 ordered adds and the division (n_w u W), and the same adds and
    division inside `mean` itself (n_w u W once scaled by beta) — (2 n_w + 2) u W / n_w on top of the bound above."""
    K, n, u = 3, 13, 2.0 ** -53
    in_aci = [True, False, True]
    E, base, _, shape, _, _ = ref.case(K, n, in_aci, False)
    target = -np.random.default_rng(5).uniform(0.2, 1.6, n)
    a, b = 8, 12
    beta = aci_scale_for_target_host(E, base, shape, target, (a, b), n, aci=in_aci)
    unit = aerosol_rows_host(E[a:b], base, np.zeros(K), shape, 1.0, n, aci=in_aci).rows
    total = unit[0]
    for t in range(1, b - a):
        total = total + unit[t]
    mean = total / (b - a)
    assert beta.shape == (n,) and (beta > 0).all() and np.array_equal(beta, target / mean)
    assert (np.abs(beta * mean - target) <= (2 * u + u * u) * np.abs(target)).all()
    rows = aerosol_rows_host(E, base, np.zeros(K), shape, beta, n, aci=in_aci).rows
    got = rows[a:b].sum(0) / (b - a)
    slack = (2 * (b - a) + 2) * u *np.abs(rows[a:b]).sum(0) / (b - a)
    assert (np.abs(got - target) <= (2 * u + u * u) * np.abs(target) + slack).all()
    # a scalar target, and any shard split: elementwise operations, the same bits
    one = aci_scale_for_target_host(E, base, shape, -1.0, (a, b), n, aci=in_aci)
    parts = [aci_scale_for_target_host(E, base, shape, -1.0, (a, b), n, lo, hi, aci=in_aci) for lo, hi in ((0, 5), (5, 5), (5, 13))]
    assert np.array_equal(np.concatenate(parts), one) and parts[1].shape == (0,)
    # a member whose emissions equal base over the window is named
    flat = E.copy()
    flat[a:b] = base
    with pytest.raises(ValueError, match="member 2: its cloud term averages to 0"):
        aci_scale_for_target_host(flat, base, shape, -1.0, (a, b), n, lo=2, aci=in_aci)
    for bad in ((3, 3), (-1, 4), (5, 13), 4):
        with pytest.raises(ValueError, match="window"):
            aci_scale_for_target_host(E, base, shape, -1.0, bad, n, aci=in_aci)


# ---- the wrappers' refusals -------------------------------------------------------------------------------------------------
def test_the_wrappers_refuse_bad_emissions_shapes_and_species():
    K, n = 3, 6
    E, base, ari, shape, beta, _ = ref.case(K, n, [True] * K, False, seed=2)
    calls = [aerosol_rows_host]
    try:
        import torch  # noqa: F401
        calls.append(aerosols.aerosol_rows)          # refuses on the host before anything is uploaded: no GPU needed
    except ImportError:
        pass
    for fn in calls:
        for bad in (-1.0, np.inf, np.nan):
            e = E.copy()
            e[3, 1] = bad
            with pytest.raises(ValueError, match="emissions"):
                fn(e, base, ari, shape, beta, n)
            bb = base.copy()
            bb[1] = bad
            with pytest.raises(ValueError, match="base"):
                fn(E, bb, ari, shape, beta, n)
        for bad in (0.0, -1.0, np.inf, np.nan, 1e-320):                                  # 1e-320: its reciprocal is not finite
            s = shape.copy()
            s[1, 2] = bad
            with pytest.raises(ValueError, match="shape"):
                fn(E, base, ari, s, beta, n)
            if fn is aerosol_rows_host:                                                  # ... where it is read, and only there
                assert np.isfinite(fn(E, base, ari, s, beta, n, aci=[True, False, True]).rows).all()
        with pytest.raises(ValueError, match="at most 8"):
            fn(np.ones((4, 9)), np.zeros(9), np.zeros(9), np.ones(9), 1.0, n)
        for bad in ([True, False], [1, 0, 1], "yes", [[True] * K]):
            with pytest.raises(ValueError, match="aci"):
                fn(E, base, ari, shape, beta, n, aci=bad)
        with pytest.raises(ValueError, match="ari"):
            fn(E, base, ari[:, :4], shape, beta, n)
        with pytest.raises(ValueError, match="shape"):
            fn(E, base, ari, shape[:2], beta, n)
        with pytest.raises(ValueError, match="shape"):
            fn(E, base, ari, None, beta, n)
        with pytest.raises(ValueError, match="beta"):
            fn(E, base, ari, shape, beta[:4], n)
        with pytest.raises(ValueError, match="beta"):
            fn(E, base, ari, shape, np.nan, n)
        with pytest.raises(ValueError, match="base"):
            fn(E, base[:2], ari, shape, beta, n)
        with pytest.raises(ValueError, match="members"):
            fn(E, base, ari, shape, beta, n, lo=4, hi=7)
        with pytest.raises(ValueError, match="K >= 1"):
            fn(np.zeros((4, 0)), base, ari, shape, beta, n)
    with pytest.raises(ValueError, match="float32"):                                     # a shape that is 0 in fp32
        aerosol_rows_host(E, base, ari[:, 0], np.full(K, 1e-60), 1.0, n, dtype=np.float32)
    none = aerosol_rows_host(E, base, ari, None, None, n, aci=[False] * K)              # no cloud term: shape and beta unread
    lin = np.array(ref.rows_scalar(E, base, ari, shape, beta, [False] * K))
    assert np.array_equal(none.rows, lin) and none.y is None
    assert aerosol_rows_host(E[:0], base, ari, shape, beta, n).rows.shape == (0, n)
    one = aerosol_rows_host(E[:, 0], base[0], ari[0, 0], shape[0, 0], 0.5, n)            # one species: scalars
    assert one.species == 1 and np.array_equal(one.rows, aerosol_rows_host(E[:, :1], base[:1], [ari[0, 0]], [shape[0, 0]], 0.5, n).rows)
