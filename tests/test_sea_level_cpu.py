"""Per-member sea-level rows (include/fiveeq.h "SEA-LEVEL ROWS"), the parts that need no GPU: the entry points and the unchanged
ABI, the C ABI's refusals in their order, the NumPy twin against an independent scalar statement (tests/sea_level_reference.py)
bit for bit, its invariance under row and member cuts, the closed forms at 50 digits, and the wrappers' refusals."""
import ctypes

import numpy as np
import pytest

import fiveeqscm_amd
from fiveeqscm_amd import _capi, sea_level
from fiveeqscm_amd.sea_level import SeaLevelComponents, SeaLevelRows, sea_level_rows_host
import sea_level_reference as ref


def test_the_new_symbols_are_exported_and_bound_and_the_abi_stays():
    lib = _capi.load()
    for sfx in ("f64", "f32"):
        name = "fiveeq_sea_level_rows_" + sfx
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
        assert len(_capi.SIGNATURES[name][1]) == 20
    assert lib.fiveeq_abi_version() == 13 and lib.fiveeq_sizeof_model() == 448          # additive: nothing existing changed
    assert any(p.endswith("fiveeq_sea.hpp") for p in _capi.SOURCES)
    for name in ("SeaLevelComponents", "SeaLevelRows", "sea_level_rows", "sea_level_rows_host"):
        assert getattr(fiveeqscm_amd, name) is getattr(sea_level, name) and name in fiveeqscm_amd.__all__


# ---- the C ABI's refusals ---------------------------------------------------------------------------------------------------
def _sea(lib, sfx="f64", S=2, J=3, mask=0b010, n=8, ld=8, n_rows=4, dt=1.0, T=0x1000, t_row=8, t_scen=64, par=0x2000, heat=0x3000,
         h_row=8, h_scen=64, eta=0x4000, S_io=0x5000, total=0x6000, comps=0x7000, ld_out=8):
    vp = ctypes.c_void_p
    return getattr(lib, "fiveeq_sea_level_rows_" + sfx)(S, J, mask, n, ld, n_rows, dt, vp(T), t_row, t_scen, vp(par), vp(heat), h_row,
                                                        h_scen, vp(eta), vp(S_io), vp(total), vp(comps), ld_out, None)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_sea_level_rows_refuses_bad_arguments_before_any_launch(sfx):
    """Every pointer here is an address nothing lies at: a call that launched would fault, a refused one returns."""
    lib = _capi.load()
    cases = [
        (dict(S=0), "n_scen=0 outside 1..64"), (dict(S=65), "n_scen=65 outside 1..64"),
        (dict(J=0), "n_comp=0 outside 1..6"), (dict(J=7, mask=0), "n_comp=7 outside 1..6"), (dict(J=-1), "n_comp=-1"),
        (dict(mask=0b1000), "rate_mask=0x8 has a bit outside the 3 components"), (dict(mask=-1), "rate_mask="),
        (dict(n=0), "n_members=0 outside"), (dict(n=2 ** 31, ld=2 ** 31), "n_members=2147483648 outside"),
        (dict(n=9), "ld=8 < n_members=9"),
        (dict(n_rows=-1), "n_rows=-1 must be >= 0"),
        (dict(dt=0.0), "dt=0 must be finite and > 0"), (dict(dt=-1.0), "dt=-1 must be"), (dict(dt=float("inf")), "dt=inf must be"),
        (dict(dt=float("nan")), "must be finite and > 0"),
        (dict(t_row=7), "t_row_stride=7 < ld=8"), (dict(t_scen=0), "t_scen_stride=0 < ld=8"),
        (dict(h_row=7), "h_row_stride=7 < ld=8"), (dict(h_scen=-8), "h_scen_stride=-8 < ld=8"),
        (dict(eta=0), "heat without eta: eta is NULL"),
        (dict(ld_out=7), "ld_out=7 < n_members=8"),
        (dict(T=0), "T_rows is NULL"), (dict(par=0), "par is NULL"), (dict(S_io=0), "S_io is NULL"), (dict(total=0), "total is NULL"),
        (dict(T=0x1001), "T_rows must be"), (dict(par=0x2004), "par must be 8-byte"), (dict(heat=0x3004), "heat must be 8-byte"),
        (dict(eta=0x4004), "eta must be 8-byte"), (dict(S_io=0x5004), "S_io must be 8-byte"), (dict(total=0x6004), "total must be 8-byte"),
        (dict(comps=0x7004), "comps must be 8-byte"),
    ]
    for kw, needle in cases:
        rc = _sea(lib, sfx, **kw)
        msg = lib.fiveeq_last_error().decode()
        assert rc == _capi.E_INVALID and needle in msg, (kw, rc, msg)
    # the order: of two bad arguments the earlier one in the documented order names itself
    order = [(dict(S=0), "n_scen"), (dict(J=0, mask=0), "n_comp"), (dict(mask=0b1000), "rate_mask"), (dict(n=0), "n_members=0"),
             (dict(n=9, ld_out=9), "ld=8 <"), (dict(n_rows=-1), "n_rows"), (dict(dt=0.0), "dt="), (dict(t_row=7), "t_row_stride"),
             (dict(t_scen=7), "t_scen_stride"), (dict(h_row=7), "h_row_stride"), (dict(h_scen=7), "h_scen_stride"),
             (dict(eta=0), "heat without eta"), (dict(ld_out=7), "ld_out"), (dict(par=0), "is NULL"), (dict(total=0x6001), "aligned")]
    for i, (kw, needle) in enumerate(order):
        for later, _ in order[i + 1:]:
            assert _sea(lib, sfx, **{**later, **kw}) == _capi.E_INVALID and needle in lib.fiveeq_last_error().decode(), (kw, later)
    assert _sea(lib, sfx, n_rows=0) == _capi.OK                                          # no rows: nothing launched
    assert _sea(lib, sfx, n_rows=0, total=0) == _capi.E_INVALID                          # ... after the checks
    # heat, eta and comps are optional; without heat its strides and eta are not looked at
    assert _sea(lib, sfx, n_rows=0, heat=0, eta=0, h_row=0, h_scen=0, comps=0) == _capi.OK
    # 4-byte alignment serves fp32 T rows and nothing else
    assert (_sea(lib, sfx, n_rows=0, T=0x1004) == _capi.OK) == (sfx == "f32")
    assert _sea(lib, sfx, n_rows=0, T=0x1004, S_io=0x5004) == _capi.E_INVALID


# ---- the twin ---------------------------------------------------------------------------------------------------------------
def _case(J, n, Sc=1, K=12, seed=0, heat=False):
    """Mixed kinds, per-member parameters, some caps that bind, a T path that rises and falls."""
    rng = np.random.default_rng(100 * J + n + seed)
    kinds = tuple("rate" if j % 3 == 1 else "relax" for j in range(J))
    tau = rng.uniform(2.0, 400.0, (J, 1)) * rng.uniform(0.6, 1.5, (J, n))
    a = rng.uniform(0.05, 0.5, (J, 1)) * rng.uniform(0.8, 1.2, (J, n))
    b = rng.uniform(-0.02, 0.06, (J, n))
    T0 = rng.uniform(-0.3, 0.6, (J, n))
    cap = np.where(rng.random((J, n)) < 0.4, rng.uniform(0.05, 0.3, (J, n)), np.inf)
    rate = np.array([k == "rate" for k in kinds])[:, None]
    a, b, cap = np.where(rate, a * 0.01, a), np.where(rate, b * 0.01, b), np.where(rate, cap * 0.01, cap)
    T = (np.linspace(0.2, 2.6, K)[None, :, None] * rng.uniform(0.5, 1.5, (Sc, 1, n)) + rng.normal(0.0, 0.15, (Sc, K, n)))
    S0 = rng.uniform(-0.02, 0.1, (Sc, J, n))
    H = np.cumsum(rng.uniform(0.2, 1.0, (Sc, K, n)), axis=1) if heat else None
    eta = rng.uniform(0.8e-3, 1.6e-3, n) if heat else None
    return kinds, (tau, a, b, T0, cap), T, S0, H, eta


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("heat", [False, True])
@pytest.mark.parametrize("J", [1, 3, 6])
def test_twin_equals_the_scalar_statement_and_any_cut(J, heat, dtype):
    n, K, Sc = 7, 12, 2
    kinds, par, T, S0, H, eta = _case(J, n, Sc, K, heat=heat)
    comp = SeaLevelComponents([f"c{j}" for j in range(J)], kinds, *par)
    Tq = T.astype(dtype)
    steps = np.arange(40, 40 + K)
    both = ("total", "components")
    whole = sea_level_rows_host(Tq, steps, comp, dt=1.0, heat=H, expansion=eta, state=S0, want=both)
    assert np.array_equal(S0, _case(J, n, Sc, K, heat=heat)[3])                          # the caller's state is not advanced
    em1 = np.expm1(-1.0 / par[0])
    want_tot, want_cmp, want_S = ref.rows_scalar(Tq.tolist(), kinds, [p.tolist() for p in par], S0.tolist(), em1.tolist(), 1.0,
                                                 None if H is None else H.tolist(), None if eta is None else eta.tolist(),
                                                 f32=dtype == np.float32)
    assert whole.total.dtype == np.float64 and whole.total.shape == (Sc, K, n) and whole.components.shape == (Sc, K, J, n)
    assert np.array_equal(whole.total, np.array(want_tot)) and np.array_equal(whole.components, np.array(want_cmp))
    assert np.array_equal(whole.S_end, np.array(want_S)) and np.array_equal(whole.steps, steps)
    assert np.array_equal(sea_level_rows_host(Tq, steps, comp, dt=1.0, heat=H, expansion=eta, state=S0, em1=em1).total, whole.total)
    if "rate" in kinds:                                                                  # the kinds differ, and the cap binds somewhere
        e = (par[1] + par[2] * (T[0, -1] - par[3])) * (T[0, -1] - par[3])
        assert (e > par[4]).any() and (e <= par[4]).any()
    # one scenario alone, without the scenario axis
    one = sea_level_rows_host(Tq[1], steps, comp, dt=1.0, heat=None if H is None else H[1], expansion=eta, state=S0[1], want=both)
    assert np.array_equal(one.total, whole.total[1]) and np.array_equal(one.components, whole.components[1])
    # row cuts through state=: an earlier result, and its S_end as an array
    for cuts in ((5,), (1, 2, 11), tuple(range(1, K))):
        parts, state = [], S0
        for a, b in zip((0,) + cuts, cuts + (K,)):
            out = sea_level_rows_host(Tq[:, a:b], steps[a:b], comp, dt=1.0, heat=None if H is None else H[:, a:b], expansion=eta,
                                      state=state, want=both)
            parts.append(out)
            state = out if len(parts) % 2 else out.S_end
        assert np.array_equal(np.concatenate([p.total for p in parts], axis=1), whole.total), cuts
        assert np.array_equal(np.concatenate([p.components for p in parts], axis=1), whole.components), cuts
        assert np.array_equal(parts[-1].S_end, whole.S_end)
    # member cuts: parameters over the design sliced by members=, and parameters given for the shard
    for lo, hi in ((0, 3), (3, 4), (4, 7)):
        cut = lambda x: None if x is None else x[..., lo:hi]                             # noqa: E731
        part = sea_level_rows_host(Tq[..., lo:hi], steps, comp, dt=1.0, heat=cut(H), expansion=cut(eta), state=S0[..., lo:hi],
                                   want=both, members=(lo, hi))
        assert np.array_equal(part.total, whole.total[..., lo:hi]) and np.array_equal(part.components, whole.components[..., lo:hi])
        own = SeaLevelComponents(comp.names, kinds, *(p[:, lo:hi] for p in par))
        shard = sea_level_rows_host(Tq[..., lo:hi], steps, own, dt=1.0, heat=cut(H), expansion=cut(eta), state=S0[..., lo:hi])
        assert np.array_equal(shard.total, part.total) and np.array_equal(shard.S_end, whole.S_end[..., lo:hi])


def test_shared_parameters_nan_rows_and_relative_to():
    K, n = 12, 5
    comp = SeaLevelComponents(("expansion", "glaciers", "greenland"), ("relax", "relax", "rate"), [80.0, 120.0, 1.0], [0.4, 0.3, 0.002],
                              [0.0, -0.02, 0.0004], 0.0 * np.ones(3), [np.inf, 0.35, np.inf])
    T = np.linspace(0.1, 2.0, K)[:, None] * np.linspace(0.8, 1.2, n)[None, :]
    steps = np.arange(K)
    out = sea_level_rows_host(T, steps, comp, dt=1.0, want=("total", "components"))
    wide = SeaLevelComponents(comp.names, comp.kind, *(np.repeat(getattr(comp, p)[:, None], n, 1) for p in ("tau", "a", "b", "T0", "cap")))
    assert np.array_equal(sea_level_rows_host(T, steps, wide, dt=1.0).total, out.total)
    # a NaN row: that member is NaN from the row on, the others keep their bits
    bad = T.copy()
    bad[5, 2] = np.nan
    nan = sea_level_rows_host(bad, steps, comp, dt=1.0)
    assert np.isnan(nan.total[5:, 2]).all() and np.array_equal(nan.total[:5], out.total[:5])
    assert np.array_equal(np.delete(nan.total, 2, axis=1), np.delete(out.total, 2, axis=1)) and np.isnan(nan.S_end[:, 2]).all()
    # anomalies: each member's mean over the window's steps taken off
    rel = out.relative_to((3, 7))
    assert np.array_equal(rel.total, out.total - out.total[3:7].mean(axis=0, keepdims=True)) and rel.S_end is None
    assert np.array_equal(rel.components, out.components - out.components[3:7].mean(axis=0, keepdims=True))
    assert np.abs(rel.total[3:7].mean(axis=0)).max() < 1e-16
    with pytest.raises(ValueError, match="holds none"):
        out.relative_to((20, 30))
    with pytest.raises(ValueError, match="cannot be continued"):
        sea_level_rows_host(T, steps + K, comp, dt=1.0, state=rel)
    only = sea_level_rows_host(T, steps, comp, dt=1.0, want=("components",))
    assert only.total is None and np.array_equal(only.components, out.components)
    empty = sea_level_rows_host(T[:0], steps[:0], comp, dt=1.0)
    assert empty.total.shape == (0, n) and np.array_equal(empty.S_end, np.zeros((3, n)))


def test_closed_form_at_fifty_digits():
    """Constant T, 300 steps, tau in {2, 50, 3000} years, a relax and a rate component, four parameter classes (a cap that
    binds, x < 0, a quadratic term, a start above equilibrium) against  Seq + (S0 - Seq) exp(-n dt / tau)  and
    S0 + n dt Seq  evaluated with mpmath at 50 digits, at rows 1, 10, 100 and 300.
    Measured (the twin with np.expm1, glibc): largest relative error 3.53e-15, at row 300 of the rate component (300 rounded
    additions of a rounded product); the relax components stay at or below 7.4e-16.  The assertion is 4 times the measured value,
    ref.CLOSED_FORM_BOUND; the margin covers an expm1 that differs by an ulp."""
    T, par, S0, dt = ref.closed_form_case()
    comp = SeaLevelComponents(("relax", "rate"), ref.CLOSED_FORM_KINDS, *(np.array(p) for p in par))
    out = sea_level_rows_host(np.array(T), np.arange(ref.CLOSED_FORM_STEPS), comp, dt=dt, state=np.array(S0), want=("components",))
    cap = np.array(par[4])
    x = np.array(T[0]) - np.array(par[3])
    e = (np.array(par[1]) + np.array(par[2]) * x) * x
    assert (e > cap).any() and (x < 0).any()                                             # the classes are what they say
    worst, where = ref.closed_form_worst(out.components)
    print(f"closed form: worst relative error {worst:.3e} at (row, kind, member) {where}; bound {ref.CLOSED_FORM_BOUND:.3e}")
    assert ref.CLOSED_FORM_BOUND == 4 * ref.CLOSED_FORM_MEASURED
    assert worst <= ref.CLOSED_FORM_BOUND, (worst, where)


# ---- the wrappers' refusals -------------------------------------------------------------------------------------------------
def test_the_wrappers_refuse_what_would_be_silently_wrong():
    K, n = 6, 4
    comp = SeaLevelComponents(("a", "b"), ("relax", "rate"), [50.0, 1.0], [0.3, 0.002], [0.0, 0.0], [0.0, 0.0], [np.inf, np.inf])
    T = np.ones((K, n))
    steps = np.arange(10, 10 + K)
    with pytest.raises(ValueError, match="row 2 holds step 12, row 3 step 14"):          # a gap, named
        sea_level_rows_host(T, np.array([10, 11, 12, 14, 15, 16]), comp, dt=1.0)
    with pytest.raises(ValueError, match="consecutive"):
        sea_level_rows_host(T, steps[::-1].copy(), comp, dt=1.0)
    with pytest.raises(ValueError, match="one per row"):
        sea_level_rows_host(T, steps[:-1], comp, dt=1.0)
    first = sea_level_rows_host(T, steps, comp, dt=1.0)
    with pytest.raises(ValueError, match="first new step 17 does not follow the state's last step 15"):
        sea_level_rows_host(T, steps + K + 1, comp, dt=1.0, state=first)
    with pytest.raises(ValueError, match="first new step 15 does not follow"):
        sea_level_rows_host(T, steps + K - 1, comp, dt=1.0, state=first)
    assert sea_level_rows_host(T, steps + K, comp, dt=1.0, state=first).total.shape == (K, n)
    with pytest.raises(ValueError, match="state: want"):
        sea_level_rows_host(T, steps, comp, dt=1.0, state=np.zeros((3, n)))
    with pytest.raises(ValueError, match="come together"):                               # expansion without heat, and the reverse
        sea_level_rows_host(T, steps, comp, dt=1.0, expansion=1e-3)
    with pytest.raises(ValueError, match="come together"):
        sea_level_rows_host(T, steps, comp, dt=1.0, heat=np.ones((K, n)))
    with pytest.raises(ValueError, match="expansion: want"):
        sea_level_rows_host(T, steps, comp, dt=1.0, heat=np.ones((K, n)), expansion=np.ones(n + 1))
    with pytest.raises(ValueError, match="heat: want"):
        sea_level_rows_host(T, steps, comp, dt=1.0, heat=np.ones((K, n + 1)), expansion=1e-3)
    with pytest.raises(ValueError, match="dt="):
        sea_level_rows_host(T, steps, comp, dt=0.0)
    with pytest.raises(ValueError, match="want:"):
        sea_level_rows_host(T, steps, comp, dt=1.0, want=("rise",))
    with pytest.raises(ValueError, match="SeaLevelComponents"):
        sea_level_rows_host(T, steps, {"tau": 1.0}, dt=1.0)
    # the components
    seven = [f"c{j}" for j in range(7)]
    with pytest.raises(ValueError, match="7 components: want 1..6"):
        SeaLevelComponents(seven, "relax", np.ones(7), np.ones(7), np.ones(7), np.ones(7), np.ones(7))
    ok = dict(tau=[50.0, 1.0], a=[0.3, 0.002], b=[0.0, 0.0], T0=[0.0, 0.0], cap=[np.inf, np.inf])
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="tau"):
            SeaLevelComponents(("a", "b"), ("relax", "rate"), **{**ok, "tau": [bad, 1.0]})
        SeaLevelComponents(("a", "b"), ("relax", "rate"), **{**ok, "tau": [50.0, bad]})  # a rate component has no tau
    for name in ("a", "b", "T0"):
        for bad in (np.inf, np.nan):
            with pytest.raises(ValueError, match=f"^{name}: want finite"):
                SeaLevelComponents(("a", "b"), ("relax", "rate"), **{**ok, name: [0.1, bad]})
    with pytest.raises(ValueError, match="cap: NaN"):
        SeaLevelComponents(("a", "b"), ("relax", "rate"), **{**ok, "cap": [np.nan, 1.0]})
    SeaLevelComponents(("a", "b"), ("relax", "rate"), **{**ok, "cap": [-np.inf, 1.0]})
    with pytest.raises(ValueError, match="kind"):
        SeaLevelComponents(("a", "b"), ("relax", "decay"), **ok)
    with pytest.raises(ValueError, match="a: want"):
        SeaLevelComponents(("a", "b"), ("relax", "rate"), **{**ok, "a": [0.1]})
    with pytest.raises(ValueError, match="rows over 5 members, the other parameters' over 4"):
        SeaLevelComponents(("a", "b"), "relax", **{**ok, "tau": np.ones((2, 4)), "a": np.ones((2, 5))})
    per_member = SeaLevelComponents(("a", "b"), "relax", **{**ok, "tau": np.full((2, 9), 30.0)})
    with pytest.raises(ValueError, match="cover neither"):
        sea_level_rows_host(T, steps, per_member, dt=1.0, members=(6, 10))
    assert sea_level_rows_host(T, steps, per_member, dt=1.0, members=(5, 9)).total.shape == (K, n)
    # host rows have no device path
    import torch
    with pytest.raises(TypeError, match="no CPU fallback"):
        sea_level.sea_level_rows(torch.ones((K, n), dtype=torch.float64), steps, comp, dt=1.0)
    with pytest.raises(ValueError, match="want a tensor"):
        sea_level.sea_level_rows(T, steps, comp, dt=1.0)
