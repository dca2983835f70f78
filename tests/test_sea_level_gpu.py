"""Per-member sea-level rows on the MI355X (include/fiveeq.h "SEA-LEVEL ROWS"): the C entry points into guarded buffers against
the NumPy twin fed the device primitive's own expm1 bits — exact, fp64 and fp32 T rows — at every lane edge and member class;
the thermosteric term; invariance under row and member cuts and views; fp64 accuracy against the 50-digit closed forms; and
the rows through EnsembleEngine.sea_level_rows into trajectory_metrics and score_rows."""
import ctypes

import numpy as np
import pytest
import torch

from fiveeqscm_amd import _capi, _rowargs, constrain, emissions
from fiveeqscm_amd import params as prm
from fiveeqscm_amd.engine import EnsembleEngine
from fiveeqscm_amd.metrics import trajectory_metrics
from fiveeqscm_amd.sea_level import SeaLevelComponents, sea_level_rows, sea_level_rows_host, sea_steps_host
import metrics_reference
import sea_level_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float64, torch.float32]
NP_OF = {torch.float64: np.float64, torch.float32: np.float32}
SENTINEL = -777.25
N_ROWS = 12
GUARD_ROWS = 2
BOTH = ("total", "components")


def _ptr(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _probe_em1(x):
    """fe_expm1_neg of fp64 x (any shape) as the device computes it: fiveeq_math_probe_f64(op = 0)."""
    lib = _capi.load()
    x_d = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).reshape(-1)).to(DEV)
    y_d = torch.empty_like(x_d)
    with torch.cuda.device(DEV):
        _capi.check(lib, lib.fiveeq_math_probe_f64(0, x_d.numel(), _ptr(x_d), _ptr(y_d), _stream()))
    torch.cuda.synchronize()
    return y_d.cpu().numpy().reshape(np.shape(x))


def _guarded(lead, rows, n, ld, dtype, data=None):
    """A sentinel buffer lead + [rows + GUARD_ROWS, ld] with `data` (lead + [rows, n]) inside."""
    buf = torch.full(tuple(lead) + (rows + GUARD_ROWS, ld), SENTINEL, dtype=dtype, device=DEV)
    if data is not None:
        buf[..., :rows, :n] = torch.from_numpy(np.ascontiguousarray(data)).to(DEV)
    return buf


def _device(dtype, T, par, mask, S0, heat=None, eta=None, ld=None, comps=True, dt=1.0, elsewhere=None):
    """One fiveeq_sea_level_rows_* call into guarded buffers: T [Sc, K, n] (NumPy, the kernel precision), par [5, J, n], S0
    [Sc, J, n].  Checks every guard — columns [n, ld) and the rows behind the last — and returns (total, comps, S_end) as
    NumPy arrays of the members' columns."""
    Sc, K, n = T.shape
    J = par.shape[1]
    ld = n if ld is None else ld
    ld_out = ld + 3 if ld > n else n
    T_b = _guarded((Sc,), K, n, ld, dtype, T)
    par_b = torch.full((5, J, ld), SENTINEL, dtype=torch.float64, device=DEV)               # [5][n_comp][ld]: no rows between
    par_b[..., :n] = torch.from_numpy(np.ascontiguousarray(par)).to(DEV)
    H_b = None if heat is None else _guarded((Sc,), K, n, ld, torch.float64, heat)
    eta_b = None if eta is None else _guarded((), 1, n, ld, torch.float64, eta[None])
    S_b = torch.full((Sc, J, ld), SENTINEL, dtype=torch.float64, device=DEV)
    S_b[..., :n] = torch.from_numpy(S0).to(DEV)
    tot_b = torch.full((Sc * K + GUARD_ROWS, ld_out), SENTINEL, dtype=torch.float64, device=DEV)
    cmp_b = torch.full((Sc * K * J + GUARD_ROWS, ld_out), SENTINEL, dtype=torch.float64, device=DEV)
    lib = _capi.load()
    fn = lib.fiveeq_sea_level_rows_f64 if dtype == torch.float64 else lib.fiveeq_sea_level_rows_f32
    with torch.cuda.device(DEV):
        _capi.check(lib, fn(Sc, J, mask, n, ld, K, dt, _ptr(T_b), ld, (K + GUARD_ROWS) * ld, _ptr(par_b), _ptr(H_b), ld,
                            (K + GUARD_ROWS) * ld, _ptr(eta_b), _ptr(S_b), _ptr(tot_b), _ptr(cmp_b) if comps else None, ld_out,
                            _stream()))
    torch.cuda.synchronize()
    tot, cmp = tot_b.cpu().numpy(), cmp_b.cpu().numpy()
    assert (tot[:, n:] == SENTINEL).all() and (tot[Sc * K:] == SENTINEL).all(), "total: a guard was written"
    assert (S_b[..., n:] == SENTINEL).all().item(), "S_io: a guard column was written"
    if comps:
        assert (cmp[:, n:] == SENTINEL).all() and (cmp[Sc * K * J:] == SENTINEL).all(), "comps: a guard was written"
    else:
        assert (cmp == SENTINEL).all(), "comps = NULL, and yet the buffer passed elsewhere was written"
    assert (par_b[..., n:] == SENTINEL).all().item()
    for b in (T_b, H_b, eta_b):                                                          # the inputs are read, never written
        if b is not None:
            assert (b[..., n:] == SENTINEL).all().item() and (b[..., -GUARD_ROWS:, :] == SENTINEL).all().item()
    return (tot[:Sc * K, :n].reshape(Sc, K, n), cmp[:Sc * K * J, :n].reshape(Sc, K, J, n) if comps else None, S_b[..., :n].cpu().numpy())


def _twin(dtype, T, par, mask, S0, heat=None, eta=None, dt=1.0):
    S = S0.copy()
    with np.errstate(all="ignore"):
        em1 = _probe_em1(-dt / par[0])
    tot, cmp = sea_steps_host(T, par, mask, dt, S, heat, eta, em1, comps=True)
    return tot, cmp, S


def _edge_lanes(n):
    return sorted({0, 63, 64, n - 1} & set(range(n)))


def _case(J, n, Sc=1, K=N_ROWS, heat=False, classes=True):
    """Per-member parameters with the member classes rotated over lanes 0, 63, 64 and the last one; T rises in every member,
    so that a cap binds from some row on."""
    rng = np.random.default_rng(1000 * J + n)
    mask = sum(1 << j for j in range(J) if j % 3 == 1)
    tau = rng.uniform(2.0, 400.0, (J, 1)) * rng.uniform(0.6, 1.5, (J, n))
    a = rng.uniform(0.05, 0.5, (J, 1)) * rng.uniform(0.8, 1.2, (J, n))
    b = rng.uniform(-0.02, 0.06, (J, n))
    T0 = rng.uniform(-0.3, 0.1, (J, n))
    cap = np.full((J, n), np.inf)
    T = np.linspace(0.2, 2.6, K)[None, :, None] * rng.uniform(0.5, 1.5, (Sc, 1, n)) + rng.uniform(0.0, 0.05, (Sc, 1, n))
    binds = []
    if classes:
        edge = _edge_lanes(n)
        for k, m in enumerate(edge):
            for c in ((k + n + J) % 6, (k + n + J + 3) % 6):
                if c == 0:
                    tau[0, m] = 1e-3                                                     # the clamp: em1 = -1
                elif c == 1:
                    tau[0, m] = 1e9
                elif c == 2:                                                             # a cap that binds from some row on
                    e = (a[0, m] + b[0, m] * (T[0, :, m] - T0[0, m])) * (T[0, :, m] - T0[0, m])
                    cap[0, m] = 0.5 * (e[K // 2 - 1] + e[K // 2])
                    binds.append(m)
                elif c == 3:
                    T0[0, m] = T.max() + 0.5                                             # x < 0 in every row
                elif c == 4:
                    a[0, m] = b[0, m] = 0.0
                elif J >= 2:                                                             # a rate and a relax component alike
                    a[1, m], b[1, m], T0[1, m] = a[0, m], b[0, m], T0[0, m]
    for m in binds:                                                                      # a condition on the inputs, checked here
        x = T[0, :, m] - T0[0, m]
        e = (a[0, m] + b[0, m] * x) * x
        assert (e > cap[0, m]).any() and (e <= cap[0, m]).any() and np.isinf(np.delete(cap[0], binds)).all()
    S0 = rng.uniform(-0.02, 0.1, (Sc, J, n))
    H = np.cumsum(rng.uniform(0.2, 1.0, (Sc, K, n)), axis=1) if heat else None
    eta = rng.uniform(0.8e-3, 1.6e-3, n) if heat else None
    return mask, np.stack([tau, a, b, T0, cap]), T, S0, H, eta


def _same(got, want, where):
    for g, w, name in zip(got, want, ("total", "comps", "S_io")):
        nan = np.isnan(w)                                      # a NaN is a NaN (its sign and payload are not part of the contract)
        assert np.array_equal(np.isnan(g), nan), (where, name)
        assert np.array_equal(np.where(nan, 0.0, g).view(np.int64), np.where(nan, 0.0, w).view(np.int64)), (where, name)


# ---- exact bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("J", [1, 3, 6])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_rows_equal_the_twin_bit_for_bit(n, J, dtype):
    mask, par, T, S0, _, _ = _case(J, n)
    Tq = T.astype(NP_OF[dtype])
    want = _twin(dtype, Tq, par, mask, S0)
    assert np.isfinite(want[0]).all()
    for ld in (n, n + 7):
        _same(_device(dtype, Tq, par, mask, S0, ld=ld), want, (n, J, ld))


def test_the_binding_cap_and_the_clamp_are_met():
    """Over the parametrisation above the classes reach the twin as they are meant to: somewhere the cap binds, somewhere
    em1 is exactly -1 (tau = 1e-3) and somewhere 1 + em1 rounds to 1 - 2^-53's neighbour (tau = 1e9)."""
    seen = set()
    for n in (1, 63, 64, 65, 256, 257):
        for J in (1, 3, 6):
            _, par, T, _, _, _ = _case(J, n)
            for m in _edge_lanes(n):
                x = T[0, :, m] - par[3, 0, m]
                e = (par[1, 0, m] + par[2, 0, m] * x) * x
                seen |= {("cap", m == n - 1)} if (e > par[4, 0, m]).any() else set()
                seen |= {"clamp"} if par[0, 0, m] == 1e-3 else set()
                seen |= {"slow"} if par[0, 0, m] == 1e9 else set()
                seen |= {"x<0"} if (x < 0).all() else set()
                seen |= {"zero"} if par[1, 0, m] == 0.0 else set()
                seen |= {"alike"} if J >= 2 and par[1, 1, m] == par[1, 0, m] else set()
    assert {"clamp", "slow", "x<0", "zero", "alike"} <= seen and any(isinstance(s, tuple) for s in seen)
    assert _probe_em1(np.array([-1.0 / 1e-3]))[0] == -1.0 and -1e-9 * 1.01 < _probe_em1(np.array([-1e-9]))[0] < -1e-9 * 0.99


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_row_poisons_its_own_lane_only(dtype):
    n, J = 65, 3
    mask, par, T, S0, _, _ = _case(J, n)
    Tq = T.astype(NP_OF[dtype])
    clean = _device(dtype, Tq, par, mask, S0)
    for lane in (0, 63, 64):
        bad = Tq.copy()
        bad[0, 5, lane] = np.nan
        got = _device(dtype, bad, par, mask, S0, ld=n + 7)
        _same(got, _twin(dtype, bad, par, mask, S0), lane)
        assert np.isnan(got[0][0, 5:, lane]).all() and np.isnan(got[2][0, :, lane]).all() and not np.isnan(got[0][0, :5]).any()
        others = np.delete(np.arange(n), lane)
        for g, c in zip(got, clean):
            assert np.array_equal(g[..., others], c[..., others]), lane


# ---- heat and eta -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("J", [1, 6])
def test_the_thermosteric_term_and_comps_null(J, dtype):
    n, Sc = 65, 2
    mask, par, T, S0, H, eta = _case(J, n, Sc, heat=True)
    Tq = T.astype(NP_OF[dtype])
    want = _twin(dtype, Tq, par, mask, S0, H, eta)
    plain = _twin(dtype, Tq, par, mask, S0)
    assert not np.array_equal(want[0], plain[0]) and np.array_equal(want[1], plain[1])   # eta H enters the total alone
    for ld in (n, n + 7):
        _same(_device(dtype, Tq, par, mask, S0, H, eta, ld=ld), want, ld)
        tot, none, S = _device(dtype, Tq, par, mask, S0, H, eta, ld=ld, comps=False)     # asserts the other buffer untouched
        assert none is None and np.array_equal(tot, want[0]) and np.array_equal(S, want[2])


# ---- splits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Sc", [1, 3])
def test_row_cuts_member_cuts_and_views(Sc, dtype):
    n, J, K = 65, 3, N_ROWS
    mask, par, T, S0, H, eta = _case(J, n, Sc, heat=True)
    Tq = T.astype(NP_OF[dtype])
    whole = _device(dtype, Tq, par, mask, S0, H, eta)
    _same(whole, _twin(dtype, Tq, par, mask, S0, H, eta), Sc)
    # rows 5 + 7 through S_io
    first = _device(dtype, Tq[:, :5], par, mask, S0, H[:, :5], eta, ld=n + 7)
    second = _device(dtype, Tq[:, 5:], par, mask, first[2], H[:, 5:], eta)
    assert np.array_equal(np.concatenate([first[0], second[0]], 1), whole[0])
    assert np.array_equal(np.concatenate([first[1], second[1]], 1), whole[1]) and np.array_equal(second[2], whole[2])
    # members 40 + 25
    for lo, hi in ((0, 40), (40, 65)):
        part = _device(dtype, Tq[..., lo:hi], par[..., lo:hi], mask, S0[..., lo:hi], H[..., lo:hi], eta[lo:hi])
        for g, w in zip(part, whole):
            assert np.array_equal(g, w[..., lo:hi]), (lo, hi)
    # the wrapper: a column-sliced view of a wider buffer is read in place and equals its contiguous copy, which equals the C call
    comp = SeaLevelComponents([f"c{j}" for j in range(J)], ["rate" if mask >> j & 1 else "relax" for j in range(J)], *par)
    steps = np.arange(7, 7 + K)
    wide = torch.full((Sc, K, n + 9), float("nan"), dtype=dtype, device=DEV)
    wide_h = torch.full((Sc, K, n + 9), float("nan"), dtype=torch.float64, device=DEV)
    view, view_h = wide[..., 3:3 + n], wide_h[..., 3:3 + n]
    view.copy_(torch.from_numpy(Tq))
    view_h.copy_(torch.from_numpy(H))
    assert _rowargs.walk_in_place(view, n)[0].data_ptr() == view.data_ptr() and view.stride(-2) == n + 9
    drop = (lambda t: t) if Sc > 1 else (lambda t: t[0])
    S0_d = torch.from_numpy(S0).to(DEV)
    got = sea_level_rows(drop(view), steps, comp, dt=1.0, heat=drop(view_h), expansion=eta, state=drop(S0_d), want=BOTH)
    flat = sea_level_rows(drop(view).contiguous(), steps, comp, dt=1.0, heat=drop(view_h).contiguous(), expansion=eta, state=drop(S0_d),
                          want=BOTH)
    for name, w in zip(("total", "components", "S_end"), whole):
        assert torch.equal(getattr(got, name), getattr(flat, name)), name
        assert np.array_equal(getattr(got, name).cpu().numpy(), drop(w)), name
    assert np.array_equal(S0_d.cpu().numpy(), S0)                                        # the caller's state is not advanced
    a = sea_level_rows(drop(view)[..., :5, :], steps[:5], comp, dt=1.0, heat=drop(view_h)[..., :5, :], expansion=eta, state=drop(S0_d))
    b = sea_level_rows(drop(view)[..., 5:, :], steps[5:], comp, dt=1.0, heat=drop(view_h)[..., 5:, :], expansion=eta, state=a)
    assert torch.equal(torch.cat([a.total, b.total], dim=-2), got.total) and torch.equal(b.S_end, got.S_end)
    with pytest.raises(ValueError, match="does not follow"):
        sea_level_rows(drop(view)[..., 5:, :], steps[5:] + 1, comp, dt=1.0, heat=drop(view_h)[..., 5:, :], expansion=eta, state=a)


# ---- accuracy -----------------------------------------------------------------------------------------------------------------
def test_fp64_rows_against_the_closed_form_at_fifty_digits():
    """The device's components under constant T (tests/sea_level_reference.py's case: 300 steps, tau in {2, 50, 3000}, relax
    and rate) against the 50-digit closed forms, at the bound the CPU test recorded: 4 x 3.54e-15."""
    T, par, S0, dt = ref.closed_form_case()
    T, par, S0 = np.array(T)[None], np.array(par), np.array(S0)[None]
    _, comps, _ = _device(torch.float64, T, par, 0b10, S0, dt=dt)
    worst, where = ref.closed_form_worst(comps[0])
    print(f"closed form on the device: worst relative error {worst:.3e} at (row, kind, member) {where}; bound {ref.CLOSED_FORM_BOUND:.3e}")
    assert worst <= ref.CLOSED_FORM_BOUND, (worst, where)


# ---- through the engine -------------------------------------------------------------------------------------------------------
N_ENG, N_STEPS = 65, 20


def _components(N):
    rng = np.random.default_rng(31)
    return SeaLevelComponents(("expansion", "glaciers", "greenland"), ("relax", "relax", "rate"),
                              tau=np.array([[80.0], [150.0], [1.0]]) * rng.uniform(0.7, 1.4, (3, N)), a=[0.42, 0.38, 0.0021],
                              b=np.array([[0.0], [-0.03], [0.0005]]) * rng.uniform(0.5, 1.5, (3, N)), T0=[0.0, 0.0, 0.1],
                              cap=[np.inf, 0.41, np.inf])


def _engine(dtype, scen, **kw):
    p = prm.sample_ensemble_shard(prm.default_params("multigas"), N_ENG)
    E = emissions.rcp_like_emissions(N_STEPS, 3)
    if scen:
        E = np.stack([E, E])
        E[1, 8:, 0] *= 1.5
    eng = EnsembleEngine(p, N_ENG, E, dtype=dtype, device=DEV, **kw)
    eng.run(mode="per_step")
    torch.cuda.synchronize()
    return eng


def _twin_of(comp, T, steps, dt, heat=None, eta=None):
    par = comp.block(T.shape[-1])
    with np.errstate(all="ignore"):
        em1 = _probe_em1(-dt / par[0])
    return sea_level_rows_host(T, steps, comp, dt=dt, heat=heat, expansion=eta, want=BOTH, em1=em1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scen", [False, True])
def test_engine_sea_level_rows(scen, dtype):
    eng = _engine(dtype, scen)
    comp = _components(N_ENG)
    before = [t.clone() for t in (eng.R, eng.S, eng.T, eng.C)]
    got = eng.sea_level_rows(comp, want=BOTH)
    direct = sea_level_rows(eng.T, eng.out_steps, comp, dt=eng.dt, want=BOTH)
    T = eng.T.cpu().numpy()
    want = _twin_of(comp, T, eng.out_steps, eng.dt)
    assert tuple(got.total.shape) == ((2,) if scen else ()) + (N_STEPS, N_ENG) and got.total.dtype == torch.float64
    for name in ("total", "components", "S_end"):
        assert torch.equal(getattr(got, name), getattr(direct, name)), name
        assert np.array_equal(getattr(got, name).cpu().numpy(), getattr(want, name)), name
    assert np.array_equal(got.steps, eng.out_steps)
    if scen:
        assert not torch.equal(got.total[0], got.total[1])
        for s in range(2):
            assert torch.equal(eng.sea_level_rows(comp, scenario=s).total, got.total[s]), s
    # the thermosteric term from the engine's own heat uptake
    eta = np.random.default_rng(5).uniform(0.9e-3, 1.5e-3, N_ENG)
    H = eng.forcing_rows(want=("H",)).H
    warm = eng.sea_level_rows(comp, expansion=eta, want=BOTH)
    want_h = _twin_of(comp, T, eng.out_steps, eng.dt, H.cpu().numpy(), eta)
    assert np.array_equal(warm.total.cpu().numpy(), want_h.total) and torch.equal(warm.components, got.components)
    assert not torch.equal(warm.total, got.total)
    # rows= and state= cut the stored rows; H stays that of the whole run
    a = eng.sea_level_rows(comp, expansion=eta, rows=slice(0, 8))
    b = eng.sea_level_rows(comp, expansion=eta, rows=slice(8, None), state=a)
    assert torch.equal(torch.cat([a.total, b.total], dim=-2), warm.total) and torch.equal(b.S_end, warm.S_end)
    for t, w in zip((eng.R, eng.S, eng.T, eng.C), before):                               # reads the engine, writes nothing
        assert torch.equal(t, w)


def test_member_forcing_engine_refuses_expansion_and_serves_relax_only():
    rows = torch.zeros((N_STEPS, N_ENG), dtype=torch.float64, device=DEV)
    eng = _engine(torch.float64, False, member_forcing=rows)
    comp = _components(N_ENG)
    with pytest.raises(ValueError, match="member_forcing= are not part of it"):
        eng.sea_level_rows(comp, expansion=1.2e-3)
    got = eng.sea_level_rows(comp)
    assert np.array_equal(got.total.cpu().numpy(), _twin_of(comp, eng.T.cpu().numpy(), eng.out_steps, eng.dt).total)
    skipping = EnsembleEngine(prm.sample_ensemble_shard(prm.default_params("co2"), 8), 8, emissions.rcp_like_emissions(N_STEPS, 1),
                              device=DEV, output_steps=[3, 4, 5, 9])
    skipping.run(mode="per_step")
    one = SeaLevelComponents("expansion", "relax", 80.0, 0.4, 0.0, 0.0, np.inf)
    with pytest.raises(ValueError, match="row 2 holds step 5, row 3 step 9"):
        skipping.sea_level_rows(one)
    assert tuple(skipping.sea_level_rows(one, rows=slice(0, 3)).total.shape) == (3, 8)


@pytest.mark.parametrize("scen", [False, True])
def test_the_rows_go_where_stored_rows_go(scen):
    """trajectory_metrics with a level in metres and score_rows against a record of anomalies take the rows as they are; both
    equal their own host references on the downloaded rows."""
    eng = _engine(torch.float64, scen)
    sl = eng.sea_level_rows(_components(N_ENG))
    rows = sl.total.cpu().numpy()
    level = float(np.median(rows[..., -1, :])) * 0.5
    m = trajectory_metrics(sl.total, sl.steps, levels=(level,), windows=((5, 15),))
    for s in range(2 if scen else 1):
        want = metrics_reference.reference(rows[s] if scen else rows, sl.steps, (level,), ((5, 15),))
        pick = (lambda t: t[s]) if scen else (lambda t: t)                               # noqa: E731
        metrics_reference.assert_equal({key: pick(getattr(m, key)).cpu().numpy() for key in want}, want, s)
    assert int((m.first >= 0).sum()) > 0                                                 # the level is crossed
    one = sl.relative_to((2, 6)).total
    one = one[1] if scen else one
    years = 2000.0 + np.arange(N_STEPS)
    mean = one.cpu().numpy().mean(1)
    obs = constrain.Observations.from_years(years, years[6::3], mean[6::3] + 0.002, 0.01, (2000.0, 2003.0))
    got = constrain.score_rows(one, sl.steps, obs)
    assert np.array_equal(got.cpu().numpy(), constrain.misfit_numpy(one.cpu().numpy(), obs.table))
