"""Forcing rows on the MI355X (include/fiveeq.h, "FORCING ROWS"; fiveeqscm_amd/diagnose.py): the replay against the stored T
bit for bit, F and F_gas against the oracle's step_forc, N and H against the NumPy twin fed the device's F, the invariances
(member range, row stride, split of the rows over calls, launch form), rows made by hand, the scenario axis, the engine's
refusals and the rows downstream in constrain.score_rows.

Shapes: 24 steps, every step stored; N in {1, 3, 63, 64, 65, 129, 131} — the tails of 2- and 4-member lanes and of a wave —
as the engine lays them out (row stride N) and embedded in rows of stride N + 5 (odd for even N: the element-access path) and
of a stride that is a multiple of 4 (16-byte accesses with a ragged tail); and once one workgroup tile plus three members,
where one call makes the 16-byte and the element launch, beside the same rows from a base one element off."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fiveeqscm_amd import _diagnose_host as twin  # noqa: E402
from fiveeqscm_amd import constrain, diagnose, emissions, params  # noqa: E402
from fiveeqscm_amd.forcing import ExternalForcings, ScenarioForcings  # noqa: E402
from oracle import fiveeq_oracle as npo  # noqa: E402

pytestmark = pytest.mark.gpu

N_STEPS = 24
SIZES = (1, 3, 63, 64, 65, 129, 131)
N_MAX = 131
DTYPES = {"f64": torch.float64, "f32": torch.float32}
# fp32 F and F_gas against the fp64 oracle on the same stored (fp32) C: |got - ref| / max(|ref|, FLOOR) W m-2.  MEASURED over
# every case of test_forcing_values (both layouts, both modes, with and without scales, every N): see FP32_MEASURED below; the
# bound is twice that, for box-to-box headroom of the hardware log / sqrt (profiles/r17/forcing_rows.txt).
FP32_FLOOR = 1e-2
FP32_MEASURED = 4.6786e-05      # multigas, plain, per-step and fused alike (co2: 4.4423e-05)
FP32_BOUND = 2.0 * FP32_MEASURED


def _table():
    t = np.arange(N_STEPS)
    return np.stack([-0.9 * (t + 1.0) / N_STEPS, np.where(t % 7 == 3, -2.5, 0.0)], 1)


def _params(kind, N, forc):
    base = params.default_params("co2" if kind == "co2" else "multigas")
    p = params.sample_ensemble_shard(base, N_MAX, 0, N)              # members [0, N) of ONE design: N = 64 is a range of N = 131
    if forc:
        G = params.n_gas_of(base)
        sc = params.sample_forcing_scales(base, N_MAX, 0, N, ranges=[(0.8, 1.2)] * G + [(0.3, 2.0), (0.5, 1.5)])
        p["f_scale"], p["fx_scale"] = sc[:G], sc[G:]
    return p


def _emissions(kind):
    return emissions.rcp_like_emissions(N_STEPS, 1 if kind == "co2" else 3)


def _engine(kind, sfx, mode, forc, N, **kw):
    from fiveeqscm_amd.engine import EnsembleEngine
    eng = EnsembleEngine(_params(kind, N, forc), N, _emissions(kind), dtype=DTYPES[sfx], device="cuda:0",
                         forcing=ExternalForcings(_table()) if forc else None, **kw)
    eng.run(mode=mode)
    torch.cuda.synchronize()
    return eng


@functools.lru_cache(maxsize=None)
def _run(kind, sfx, mode, forc, N):
    """One run, kept for every test that reads it (nothing writes into an engine's rows after the run)."""
    return _engine(kind, sfx, mode, forc, N)


def _embed(t, ld):
    """t [.., N] as the first N columns of rows of stride ld."""
    buf = torch.full(tuple(t.shape[:-1]) + (ld,), float("nan"), dtype=t.dtype, device=t.device)
    view = buf[..., :t.shape[-1]]
    view.copy_(t)
    return view


def _diag(eng, ld=None, rows=slice(None), members=None, **kw):
    """diagnose.forcing_rows on the engine's rows: as they lie (ld None), or embedded in rows of stride ld; members: the
    first `members` columns, in place."""
    put = (lambda t: t) if ld is None else (lambda t: _embed(t, ld))
    cut = (lambda t: t) if members is None else (lambda t: t[..., :members])
    return diagnose.forcing_rows(cut(put(eng.C))[rows], eng.out_steps[rows], eng.params, q=cut(put(eng.q)), F_ext=eng.drive, dt=eng.dt,
                                 T_rows=cut(put(eng.T))[rows], fscale=None if eng.fscale is None else cut(put(eng.fscale)),
                                 X=eng.fext, **kw)


def _strides(N):
    return (None, N + 5, (N + 3) // 4 * 4 + 4)


def _same(a, b):
    """torch.equal with NaN equal to NaN (a row made by hand may hold one)."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


# ---- 1. the replay ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forc", [False, True], ids=["plain", "scales"])
@pytest.mark.parametrize("mode", ["per_step", "fused"])
@pytest.mark.parametrize("kind", ["co2", "multigas"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_replay_reproduces_the_stored_T_bit_for_bit(sfx, kind, mode, forc):
    """The thermal step repeated on the diagnosed F from the initial boxes gives the stored T in every bit and ends in the
    engine's S: the diagnosed F is the stepping kernel's F — for rows of the per-step and the fused kernel (fp32: packed and
    unpacked lanes), both layouts, with and without forcing scales (K = 2, non-unit scales)."""
    for N in SIZES:
        eng = _run(kind, sfx, mode, forc, N)
        res = eng.forcing_rows(want=("F",), replay=True)
        assert res.replay_mismatches == 0, (N, res.replay_mismatches)
        assert torch.equal(res.S_end, eng.S), N
        for ld in _strides(N)[1:]:
            r2 = _diag(eng, ld, want=("F",), S_begin=torch.zeros_like(eng.S))
            assert r2.replay_mismatches == 0 and torch.equal(r2.S_end, eng.S) and torch.equal(r2.F, res.F), (N, ld)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_replay_control_one_ulp_of_q_in_one_member_is_found_in_that_member_only(sfx):
    """The control of the test above: the same call with q[1] (the fast box, whose step weighs q F most) of ONE member moved by
    one ulp reports mismatches, and only that member's boxes end elsewhere."""
    N, m = 65, 37
    eng = _run("multigas", sfx, "per_step", True, N)
    q = eng.q.clone()
    q[1, m] = torch.nextafter(q[1, m], q[1, m] * 2)
    res = diagnose.forcing_rows(eng.C, eng.out_steps, eng.params, q=q, F_ext=eng.drive, dt=eng.dt, T_rows=eng.T, fscale=eng.fscale,
                                X=eng.fext, want=("F",), S_begin=torch.zeros_like(eng.S))
    assert 0 < res.replay_mismatches <= N_STEPS
    differs = (res.S_end != eng.S).any(0)
    assert differs[m] and int(differs.sum()) == 1


# ---- 2. the forcing values ----------------------------------------------------------------------------------------------------
def _oracle_forcing(eng):
    """F_gas and F in fp64 NumPy from the oracle's step_forc on the STORED C, the scales and tables applied in NumPy."""
    C = eng.C.double().cpu().numpy()
    G = C.shape[1]
    C0 = np.asarray(eng.params["PI_conc"], dtype=np.float64).reshape(G)
    f = np.asarray(eng.params["f"], dtype=np.float64).reshape(G, 3)
    Fg = np.stack([npo.step_forc(C[:, g], C0[g], f[g]) for g in range(G)], 1)
    fext = eng.drive.double().cpu().numpy()[eng.out_steps, 6]
    if eng.fscale is None:
        return Fg, twin.total_forcing(Fg, fext)
    return Fg, twin.total_forcing(Fg, fext, eng.fscale.double().cpu().numpy(), eng.forcing.table[eng.out_steps])


_fp32_worst = {}


@pytest.mark.parametrize("forc", [False, True], ids=["plain", "scales"])
@pytest.mark.parametrize("mode", ["per_step", "fused"])
@pytest.mark.parametrize("kind", ["co2", "multigas"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_forcing_values(sfx, kind, mode, forc, capsys):
    """F and F_gas against the oracle on the stored C: fp64 pointwise at 1e-10 |ref| + 1e-13; fp32 at twice the measured worst
    deviation (FP32_MEASURED, relative with a 1e-2 W m-2 floor)."""
    worst = 0.0
    for N in SIZES:
        eng = _run(kind, sfx, mode, forc, N)
        ref_g, ref = _oracle_forcing(eng)
        for ld in _strides(N):
            res = _diag(eng, ld, want=("F", "F_gas"))
            for got, want in ((res.F, ref), (res.F_gas, ref_g)):
                got = got.double().cpu().numpy()
                assert np.isfinite(got).all()
                if sfx == "f64":
                    assert np.all(np.abs(got - want) <= 1e-10 * np.abs(want) + 1e-13), (N, ld)
                else:
                    worst = max(worst, float((np.abs(got - want) / np.maximum(np.abs(want), FP32_FLOOR)).max()))
    if sfx == "f32":
        _fp32_worst[(kind, mode, forc)] = worst
        with capsys.disabled():
            print(f"\n  fp32 forcing rows vs the fp64 oracle, worst |got - ref| / max(|ref|, {FP32_FLOOR}): {kind} {mode} "
                  f"{'scales' if forc else 'plain'} {worst:.3e} (worst so far {max(_fp32_worst.values()):.3e})")
        assert worst <= FP32_BOUND, (worst, FP32_BOUND)


@pytest.mark.parametrize("mode", ["per_step", "fused"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_unit_scales_with_a_zero_table_give_the_bits_of_the_plain_run(sfx, mode):
    N = 65
    plain = _run("multigas", sfx, mode, False, N)
    from fiveeqscm_amd.engine import EnsembleEngine
    eng = EnsembleEngine(_params("multigas", N, False), N, _emissions("multigas"), dtype=DTYPES[sfx], device="cuda:0",
                         forcing=ExternalForcings(np.zeros((N_STEPS, 2))))
    eng.run(mode=mode)
    assert eng.fscale is not None and torch.equal(eng.C, plain.C)
    a, b = eng.forcing_rows(want=("F", "F_gas", "N", "H")), plain.forcing_rows(want=("F", "F_gas", "N", "H"))
    for name in ("F", "F_gas", "N", "H"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


# ---- 3. imbalance and heat ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forc", [False, True], ids=["plain", "scales"])
@pytest.mark.parametrize("kind", ["co2", "multigas"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_imbalance_and_heat_are_the_twin_fed_the_device_forcing(sfx, kind, forc):
    """N and H are single IEEE operations on F and the stored T: the NumPy twin fed the DEVICE's F gives their bits."""
    for N in SIZES:
        eng = _run(kind, sfx, "per_step", forc, N)
        for ld in _strides(N):
            res = _diag(eng, ld, want=("F", "N", "H"))
            Nn = twin.imbalance(res.F.cpu().numpy(), eng.T.cpu().numpy(), eng.q.cpu().numpy())
            H = twin.heat(Nn, eng.dt)
            assert res.N.dtype == DTYPES[sfx] and res.H.dtype == torch.float64
            assert torch.equal(res.N.cpu(), torch.from_numpy(Nn)), (N, ld)
            assert torch.equal(res.H.cpu(), torch.from_numpy(H)), (N, ld)


# ---- 4. layout and split invariance -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["co2", "multigas"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_outputs_do_not_depend_on_member_range_stride_split_or_launch_form(sfx, kind):
    names = ("F", "F_gas", "N", "H")
    big, small = _run(kind, sfx, "per_step", True, 131), _run(kind, sfx, "per_step", True, 64)
    S0 = torch.zeros_like(big.S)
    whole = _diag(big, want=names, S_begin=S0)
    # members [0, 64) out of N = 131 (in place: stride 131), against N = 64 alone
    part = _diag(big, members=64, want=names, S_begin=S0[:, :64])
    alone = _diag(small, want=names, S_begin=torch.zeros_like(small.S))
    for name in names + ("S_end",):
        assert torch.equal(getattr(part, name), getattr(whole, name)[..., :64]), name
        assert torch.equal(getattr(part, name), getattr(alone, name)), name
    assert whole.replay_mismatches == part.replay_mismatches == alone.replay_mismatches == 0
    for eng in (big, small, _run(kind, sfx, "per_step", True, 65)):
        N = eng.n_members
        z = torch.zeros_like(eng.S)
        base = _diag(eng, want=names, S_begin=z)
        # ld odd against even (and a multiple of 4)
        odd, even = (_diag(eng, ld, want=names, S_begin=z) for ld in ((N + 5) | 1, (N + 3) // 4 * 4 + 4))
        for name in names + ("S_end",):
            assert torch.equal(getattr(odd, name), getattr(even, name)) and torch.equal(getattr(odd, name), getattr(base, name)), name
        # the rows split 10 + 14 over two calls, the state carried
        a = _diag(eng, rows=slice(0, 10), want=names, S_begin=z)
        b = _diag(eng, rows=slice(10, None), want=names, S_begin=a.S_end, heat0=a.H[-1])
        for name in names:
            assert torch.equal(torch.cat([getattr(a, name), getattr(b, name)]), getattr(base, name)), name
        assert torch.equal(b.S_end, base.S_end) and a.replay_mismatches + b.replay_mismatches == 0
        # F alone (the row-parallel grid) against F beside N and H (a lane carries its members through the rows)
        for ld in _strides(N):
            assert torch.equal(_diag(eng, ld, want=("F",)).F, base.F), ld
            assert torch.equal(_diag(eng, ld, want=("F", "N", "H")).F, base.F), ld


def _embed_at(t, ld, off):
    """t [.., N] as the first N columns of rows of stride ld that begin `off` elements into a 16-byte aligned buffer."""
    lead = tuple(t.shape[:-1])
    flat = torch.full((off + int(np.prod(lead)) * ld,), float("nan"), dtype=t.dtype, device=t.device)
    view = flat[off:].view(lead + (ld,))[..., :t.shape[-1]]
    view.copy_(t)
    assert flat.data_ptr() % 16 == 0 and view.data_ptr() == flat.data_ptr() + off * t.element_size()
    return view


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_a_tile_and_three_members_in_both_launches_and_from_a_base_one_element_off(sfx):
    """One workgroup tile plus three members, rows of a stride that is a multiple of 16 bytes: aligned rows give the 16-byte
    launch on [0, n_vec) and the element launch on the three (fp64: one) members from n_vec > 0 in ONE call; the same rows one
    element into the buffer give the element launch alone.  Both replay the stored T in every bit and end in the engine's S,
    agree with each other in every bit of F, F_gas, N and H, and give N and H of the twin fed the device's F; fp64 F and F_gas
    against the oracle at the bound of test_forcing_values (its fp32 bound is a measurement over that test's own cases)."""
    from fiveeqscm_amd import _capi
    from fiveeqscm_amd.engine import EnsembleEngine
    width = 8 if sfx == "f64" else 4
    per16, tile = 16 // width, int(_capi.load().fiveeq_forcing_rows_tile(width))
    N = tile + 3
    ld = (N + 3) // 4 * 4 + 4
    assert N // per16 * per16 >= tile and N % per16 != 0 and ld % per16 == 0
    base = params.default_params("multigas")
    p = params.sample_ensemble_shard(base, N, 0, N)
    sc = params.sample_forcing_scales(base, N, 0, N, ranges=[(0.8, 1.2)] * 3 + [(0.3, 2.0), (0.5, 1.5)])
    p["f_scale"], p["fx_scale"] = sc[:3], sc[3:]
    eng = EnsembleEngine(p, N, _emissions("multigas"), dtype=DTYPES[sfx], device="cuda:0", forcing=ExternalForcings(_table()))
    eng.run(mode="per_step")
    torch.cuda.synchronize()
    names = ("F", "F_gas", "N", "H")
    res = {}
    for off in (0, 1):
        put = lambda t: _embed_at(t, ld, off)                                                 # noqa: E731
        res[off] = r = diagnose.forcing_rows(put(eng.C), eng.out_steps, eng.params, q=put(eng.q), F_ext=eng.drive, dt=eng.dt,
                                             T_rows=put(eng.T), fscale=put(eng.fscale), X=eng.fext, want=names,
                                             S_begin=torch.zeros_like(eng.S))
        assert r.replay_mismatches == 0 and torch.equal(r.S_end, eng.S), off
        Nn = twin.imbalance(r.F.cpu().numpy(), eng.T.cpu().numpy(), eng.q.cpu().numpy())
        assert torch.equal(r.N.cpu(), torch.from_numpy(Nn)) and torch.equal(r.H.cpu(), torch.from_numpy(twin.heat(Nn, eng.dt))), off
    for name in names:
        assert torch.equal(getattr(res[0], name), getattr(res[1], name)), name
    if sfx == "f64":
        ref_g, ref = _oracle_forcing(eng)
        for got, want in ((res[0].F, ref), (res[0].F_gas, ref_g)):
            assert np.all(np.abs(got.cpu().numpy() - want) <= 1e-10 * np.abs(want) + 1e-13)


# ---- 5. rows by hand ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_rows_by_hand_guards_nan_and_the_preindustrial_row(sfx, capsys):
    """C <= 0 (no log term, sqrt C reads 0), NaN, and C = C0 (F exactly F_ext), 4 + 1 + 1 layout, N = 65: NaN reaches F and N of
    its member in its row, H from that row on, and no other member."""
    dt, N, K, G = DTYPES[sfx], 65, 6, 3
    p = _params("multigas", N, False)
    C0 = np.asarray(p["PI_conc"], dtype=np.float64)
    f = np.asarray(p["f"], dtype=np.float64).reshape(G, 3)
    rng = np.random.default_rng(5)
    C = (C0[None, :, None] * rng.uniform(1.0, 2.5, size=(K, G, N)))
    C[2, 0, 5], C[1, 1, 7], C[4, 2, 7], C[3, 2, 9] = -1.0, 0.0, -0.0, np.nan
    C[:, :, 11] = C0[None, :]
    C = torch.from_numpy(C).to("cuda:0", dt)
    T = torch.from_numpy(rng.normal(1.0, 0.3, size=(K, N))).to("cuda:0", dt)
    q = torch.from_numpy(np.asarray(p["q"])).to("cuda:0", dt)
    steps = np.arange(3, 3 + K)
    F_ext = np.linspace(-0.5, 0.75, 12)
    res = diagnose.forcing_rows(C, steps, p, q=q, F_ext=F_ext, dt=1.0, T_rows=T, want=("F", "F_gas", "N", "H"))
    Ch = C.cpu().numpy()
    ref_g = np.stack([npo.step_forc(Ch[:, g].astype(np.float64), C0[g], f[g]) for g in range(G)], 1)
    ref = twin.total_forcing(ref_g, F_ext[steps])
    got_g, got = res.F_gas.double().cpu().numpy(), res.F.double().cpu().numpy()
    fin = np.ones((K, N), dtype=bool)
    fin[3, 9] = False
    tol = (lambda r: 1e-10 * np.abs(r) + 1e-13) if sfx == "f64" else (lambda r: 4e-6 * np.maximum(np.abs(r), 1.0))
    # (fp32 here: a coarse bound, four ulp(float) of max(|F_g|, 1) with f1 ln and f3 sqrt terms of O(1..10): the guards'
    # values are what this test is about, the fp32 accuracy is test_forcing_values')
    assert np.all(np.abs(got - ref)[fin] <= tol(ref)[fin])
    assert np.all((np.abs(got_g - ref_g) <= tol(ref_g)) | np.isnan(ref_g))
    # the guard's values spelt out: C <= 0 leaves f2 (C - C0) - f3 sqrt C0
    for (k, g, m) in ((2, 0, 5), (1, 1, 7), (4, 2, 7)):
        want = f[g, 1] * (Ch[k, g, m] - C0[g]) - f[g, 2] * np.sqrt(C0[g])
        assert abs(got_g[k, g, m] - want) <= tol(np.array(want)), (k, g, m)
    with capsys.disabled():
        print(f"\n  rows by hand {sfx}: F - F_ext of the member at C = C0: {np.abs(got[:, 11] - F_ext[steps].astype(Ch.dtype)).max():.3e}; "
              f"F_gas there: {np.abs(got_g[:, :, 11]).max(0)}")
    assert torch.equal(res.F[:, 11].cpu(), torch.from_numpy(F_ext[steps]).to(dt)), "C = C0: F is exactly F_ext"
    # NaN: F and N of member 9 in row 3, H from row 3 on, nobody else
    nanF, nanN, nanH = res.F.isnan().cpu().numpy(), res.N.isnan().cpu().numpy(), res.H.isnan().cpu().numpy()
    want_row = ~fin
    want_on = np.zeros((K, N), dtype=bool)
    want_on[3:, 9] = True
    assert np.array_equal(nanF, want_row) and np.array_equal(nanN, want_row) and np.array_equal(nanH, want_on)
    assert bool(res.F_gas[3, 2, 9].isnan()) and int(res.F_gas.isnan().sum()) == 1
    Nn = twin.imbalance(res.F.cpu().numpy(), T.cpu().numpy(), q.cpu().numpy())
    assert _same(res.N.cpu(), torch.from_numpy(Nn)) and _same(res.H.cpu(), torch.from_numpy(twin.heat(Nn, 1.0)))


# ---- 6. the scenario axis -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_scenario_axis_equals_the_single_scenario_engines(sfx):
    from fiveeqscm_amd.engine import EnsembleEngine
    N = 65
    p = _params("multigas", N, True)
    E = _emissions("multigas")
    E2 = np.stack([E, E])
    E2[1, 8:, 0] *= 1.5
    sf = ScenarioForcings(np.stack([_table(), 0.5 * _table()]))
    names = ("F", "F_gas", "N", "H")
    eng = EnsembleEngine(p, N, E2, dtype=DTYPES[sfx], device="cuda:0", forcing=sf)
    eng.run(mode="per_step")
    both = eng.forcing_rows(want=names, replay=True)
    assert both.replay_mismatches == [0, 0] and tuple(both.F.shape) == (2, N_STEPS, N) and tuple(both.F_gas.shape) == (2, N_STEPS, 3, N)
    assert torch.equal(both.S_end, eng.S)
    for s in range(2):
        one = EnsembleEngine(p, N, E2[s], dtype=DTYPES[sfx], device="cuda:0", forcing=sf.scenario(s))
        one.run(mode="per_step")
        alone = one.forcing_rows(want=names, replay=True)
        picked = eng.forcing_rows(want=names, scenario=s)
        assert alone.replay_mismatches == 0
        for name in names:
            assert torch.equal(getattr(both, name)[s], getattr(alone, name)), (s, name)
            assert torch.equal(getattr(picked, name), getattr(alone, name)), (s, name)
    assert not torch.equal(both.F[0], both.F[1])


# ---- 7. the engine's refusals -------------------------------------------------------------------------------------------------
def test_engine_refusals():
    from fiveeqscm_amd.engine import EnsembleEngine
    N = 64
    p, E = _params("co2", N, False), _emissions("co2")
    eng = EnsembleEngine(p, N, E, dtype=torch.float32, device="cuda:0", compensated=True)
    with pytest.raises(ValueError, match="unrounded|UNROUNDED"):
        eng.forcing_rows()
    conc = np.linspace(278.0, 400.0, N_STEPS).reshape(-1, 1)
    eng = EnsembleEngine(p, N, conc, device="cuda:0", concentration_driven=True)
    with pytest.raises(ValueError, match="concentration-driven"):
        eng.forcing_rows()
    eng = EnsembleEngine(p, N, E, device="cuda:0", store_concentrations=False)
    with pytest.raises(ValueError, match="no stored concentrations"):
        eng.forcing_rows()
    eng = EnsembleEngine(p, N, E, device="cuda:0", output_steps=[3, 4, 5, 9])
    eng.run(mode="per_step")
    with pytest.raises(ValueError, match="every step from 0"):
        eng.forcing_rows(replay=True)
    with pytest.raises(ValueError, match=r"row 2 holds step 5, row 3 step 9"):
        eng.forcing_rows(want=("H",))
    assert tuple(eng.forcing_rows(want=("F", "N")).N.shape) == (4, N)          # F and N need no consecutive steps
    with pytest.raises(TypeError, match="no CPU fallback"):
        diagnose.forcing_rows(eng.C.cpu(), eng.out_steps, p, q=eng.q, F_ext=eng.drive, dt=1.0)
    with pytest.raises(ValueError, match="need T_rows"):
        diagnose.forcing_rows(eng.C, eng.out_steps, p, q=eng.q, F_ext=eng.drive, dt=1.0, want=("N",))


# ---- 8. downstream ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_heat_rows_feed_score_rows(sfx):
    """The rows are usable where the module says they are: a heat-content record scored against res.H by the score pass equals
    misfit_numpy on the same rows bit for bit (the score pass's own contract)."""
    eng = _run("multigas", sfx, "per_step", True, 129)
    res = eng.forcing_rows(want=("H", "F"))
    years = 2000.0 + np.arange(N_STEPS)
    Hm = res.H.cpu().numpy().mean(1)
    obs = constrain.Observations.from_years(years, years[6::3], Hm[6::3] - Hm[:4].mean() + 0.1, 0.5, (2000.0, 2003.0))
    got = constrain.score_rows(res.H, eng.out_steps, obs)
    assert np.array_equal(got.cpu().numpy(), constrain.misfit_numpy(res.H.cpu().numpy(), obs.table))
    band = constrain.Observations.absolute(years, years[-1:], [float(res.F[-1].double().mean())], 0.3)
    gotF = constrain.score_rows(res.F, eng.out_steps, band)
    assert np.array_equal(gotF.cpu().numpy(), constrain.misfit_numpy(res.F.cpu().numpy(), band.table))
