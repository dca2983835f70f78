"""Per-member forcing scales on the MI355X (include/fiveeq.h "FORCING SCALES"): against the frozen oracle run member by
member on scaled coefficients and a summed F_ext (no step code shared), unit scales against the plain engine bit for bit,
the same bits in every form, the misfit rows against constrain.misfit_numpy, fp32 against the CPU reference, a checkpoint
round trip and the refusals.  (smoke() has a forcing leg of its own.)"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from fiveeqscm_amd import _capi, constrain, emissions, scenario
from fiveeqscm_amd import params as prm
from fiveeqscm_amd.constrain import Observations
from fiveeqscm_amd.engine import EnsembleEngine
from fiveeqscm_amd.forcing import ExternalForcings
from forcing_reference import forcing_numpy
from oracle import fiveeq_oracle as npo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STEPS = 300
GASES = {"co2": 1, "multigas": 3}
MODES = ("per_step", "graph", "fused", "ksteps")


def _table(n_steps=N_STEPS, G=3):
    """Three categories: a negative aerosol-like ramp following the CO2 emissions, volcanic spikes, an 11-step sinusoid."""
    E = emissions.rcp_like_emissions(n_steps, G)
    tt = np.arange(n_steps)
    X = np.stack([-1.1 * E[:, 0] / E[:, 0].max(), np.where(tt % 37 == 5, -2.5, 0.0), 0.1 * np.sin(2 * np.pi * tt / 11.0)], 1)
    return E, ExternalForcings(X, ("aerosol", "volcanic", "solar")), 0.02 * tt / n_steps


@functools.lru_cache(maxsize=None)
def _case(kind, N, n_steps=N_STEPS):
    """(params with f_scale / fx_scale rows, E, table, F_ext): gas scales in 0.8..1.2, aerosol 0.3..2.0, the others 0.5..1.5."""
    G = GASES[kind]
    base = prm.default_params(kind)
    p = prm.sample_ensemble_shard(base, N)
    s = prm.sample_forcing_scales(base, N, ranges=[(0.8, 1.2)] * G + [(0.3, 2.0), (0.5, 1.5), (0.5, 1.5)], seed=7)
    p["f_scale"], p["fx_scale"] = s[:G], s[G:]
    E, fx, Fx = _table(n_steps, G)
    return p, E, fx, Fx


@functools.lru_cache(maxsize=None)
def _reference(kind, N, n_steps=N_STEPS):
    p, E, fx, Fx = _case(kind, N, n_steps)
    return forcing_numpy(E, p, N, fx, p["f_scale"], p["fx_scale"], F_ext=Fx)


def _run(p, N, E, mode="per_step", split=None, packing=1, **kw):
    """(C, T, R, S[, misfit]) on the host after a run of every step in `mode` (or split = (step, mode, mode))."""
    lib = _capi.load()
    prev = lib.fiveeq_set_f32_packing(packing)
    try:
        eng = EnsembleEngine(p, N, E, device="cuda:0", **kw)
        if split:
            eng.run(0, split[0], mode=split[1])
            eng.run(split[0], eng.n_steps, mode=split[2])
        else:
            eng.run(mode=mode, **({"k_steps": 8} if mode == "ksteps" else {}))
        torch.cuda.synchronize()
        out = [getattr(eng, k).cpu() for k in ("C", "T", "R", "S")] + ([eng.misfit.cpu()] if eng.misfit is not None else [])
        eng.close()
        return out
    finally:
        lib.fiveeq_set_f32_packing(prev)


def _plain(p):
    return {k: v for k, v in p.items() if k not in ("f_scale", "fx_scale")}


# ---- 1. against the frozen oracle, member by member ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["co2", "multigas"])
def test_fp64_against_the_oracle_run_member_by_member(kind):
    """For each member the oracle runs alone with f[g] multiplied by the member's gas scale and F_ext + X @ sx as its
    external forcing: no step code shared with the engine, and not the NumPy restatement either.  Every stored C and T of
    every form within |a - b| <= 1e-10 |b| + 1e-13, no exceptions."""
    N = 48
    G = GASES[kind]
    p, E, fx, Fx = _case(kind, N)
    base_f = np.asarray(prm.default_params(kind)["f"], float).reshape(G, 3)
    C_ref, T_ref = np.empty((N_STEPS, G, N)), np.empty((N_STEPS, N))
    for m in range(N):
        pm = _plain(p)
        for k in ("r0", "rC", "rT", "q"):
            pm[k] = np.asarray(p[k])[:, m:m + 1]
        pm["f"] = base_f * p["f_scale"][:, m][:, None]
        o = npo.run(E, pm, 1, F_ext=Fx + fx.table @ p["fx_scale"][:, m])
        C_ref[:, :, m], T_ref[:, m] = o["C"][:, :, 0], o["T"][:, 0]
    assert int((np.sign(T_ref[1:]) != np.sign(T_ref[:-1])).sum()) > 0       # T goes through zero: the absolute term is used
    # ... and the vectorised restatement the larger cases use agrees with it far inside the bound
    ref = _reference(kind, N)
    for a, b in ((ref["C"], C_ref), (ref["T"], T_ref)):
        assert (np.abs(a - b) / (1e-10 * np.abs(b) + 1e-13)).max() <= 1e-2
    for mode in MODES:
        C, T = _run(p, N, E, mode, F_ext=Fx, forcing=fx)[:2]
        for name, got, want in (("C", C.numpy(), C_ref), ("T", T.numpy(), T_ref)):
            err = np.abs(got - want) / (1e-10 * np.abs(want) + 1e-13)
            print(f"{kind} {mode} {name}: worst err/bound {err.max():.3g}")
            assert np.isfinite(got).all() and err.max() <= 1.0, (kind, mode, name, float(err.max()))


@pytest.mark.parametrize("kind", ["co2", "multigas"])
def test_fp64_larger_ensemble_against_the_numpy_restatement(kind):
    N = 4096 + 37
    p, E, fx, Fx = _case(kind, N)
    ref = _reference(kind, N)
    for mode in ("per_step", "fused"):
        C, T = _run(p, N, E, mode, F_ext=Fx, forcing=fx)[:2]
        for name, got in (("C", C.numpy()), ("T", T.numpy())):
            err = np.abs(got - ref[name]) / (1e-10 * np.abs(ref[name]) + 1e-13)
            assert np.isfinite(got).all() and err.max() <= 1.0, (kind, mode, name, float(err.max()))


# ---- 2. unit scales are the plain engine, bit for bit ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["co2", "multigas"])
def test_unit_scales_are_the_plain_run_bit_for_bit(kind, dtype):
    N = 3000 + 1
    p, E, fx, Fx = _case(kind, N)
    plain = _plain(p)

    def run(mode, forcing, params):
        eng = EnsembleEngine(params, N, E, F_ext=Fx, dtype=dtype, forcing=forcing, collect_stats=True, device="cuda:0")
        eng.run(mode=mode)
        torch.cuda.synchronize()
        out = [getattr(eng, k).cpu() for k in ("C", "T", "R", "S", "T_stats")]
        eng.close()
        return out

    rng = np.random.default_rng(5)
    any_sx = dict(plain, fx_scale=rng.uniform(-3.0, 3.0, (3, N)))
    for mode in ("per_step", "fused"):
        want = run(mode, None, plain)
        cases = {"K=0": (ExternalForcings(np.zeros((N_STEPS, 0))), plain),
                 "zero table, unit sx": (ExternalForcings(np.zeros((N_STEPS, 3))), plain),
                 "zero table, any finite sx": (ExternalForcings(np.zeros((N_STEPS, 3))), any_sx)}
        for what, (forcing, params) in cases.items():
            got = run(mode, forcing, params)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (mode, what)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["co2", "multigas"])
def test_no_category_fused_reads_no_table(kind, dtype):
    """K = 0 with scale rows far shorter than a table would be (G N < 4 n_steps): the fused kernel must stage no table
    record — there is none, and the C ABI takes fext = NULL.  A guard page cannot be asked for here, so the check is the
    contract's own: the plain run's bits, through the engine (whose table pointer is then a zero-column buffer) and through
    the C ABI with fext = NULL, per step and fused, in spans that cross several refills of the drive chunk."""
    N, n_steps = 64, 750
    G = GASES[kind]
    base = prm.default_params(kind)
    p = prm.sample_ensemble_shard(base, N)
    E = emissions.rcp_like_emissions(n_steps, G)
    assert G * N < 4 * n_steps
    want = _run(p, N, E, "fused", dtype=dtype)
    none = ExternalForcings(np.zeros((n_steps, 0)))
    for mode in ("fused", "ksteps", "per_step", "graph"):
        got = _run(p, N, E, mode, dtype=dtype, forcing=none)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), (kind, mode)
    for form, k in ((_capi.FORM_FUSED, 0), (_capi.FORM_FUSED, 200), (_capi.FORM_PER_STEP, 0)):
        eng = EnsembleEngine(p, N, E, dtype=dtype, forcing=none, device="cuda:0")
        rc = eng._fn("run_forc")(*eng._run_args(0, n_steps), eng._ptr(eng.fscale), None, 0, None, None, form, k, eng._stream())
        _capi.check(eng.lib, rc)
        torch.cuda.synchronize()
        got = [getattr(eng, name).cpu() for name in ("C", "T", "R", "S")]
        assert all(torch.equal(a, b) for a, b in zip(got, want)), (kind, form, k)
        plan = ctypes.c_void_p()
        eng.reset_state()
        rc = eng._fn("plan_create_forc")(*eng._run_args(0, n_steps), eng._ptr(eng.fscale), None, 0, None, None, ctypes.byref(plan))
        _capi.check(eng.lib, rc)
        _capi.check(eng.lib, eng.lib.fiveeq_plan_launch(plan, eng._stream()))
        torch.cuda.synchronize()
        assert torch.equal(eng.T.cpu(), want[1]), (kind, "plan")
        eng.lib.fiveeq_plan_destroy(plan)
        eng.close()


def test_non_finite_scale_rows_are_refused():
    N = 256
    p, E, fx, Fx = _case("multigas", N)
    for name in ("f_scale", "fx_scale"):
        bad = np.array(p[name], copy=True)
        bad[0, 7] = np.inf if name == "f_scale" else np.nan
        with pytest.raises(ValueError, match="non-finite"):
            EnsembleEngine(dict(p, **{name: bad}), N, E, forcing=fx, device="cuda:0")


# ---- 3. the same bits in every form -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def obs():
    y, T, s = scenario.read_observations_csv(os.path.join(ROOT, "tests", "golden", "obs_synthetic.csv"))
    years = 1750.0 + np.arange(N_STEPS)
    keep = y < years[-1]
    return Observations.from_years(years, y[keep], T[keep], s[keep], baseline=(1900, 1950))


@pytest.mark.parametrize("with_obs", [False, True])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["co2", "multigas"])
def test_every_form_gives_the_same_bits(kind, dtype, with_obs, obs):
    N = 3000 + 1                                                  # ragged: the last packed lane holds one member
    p, E, fx, Fx = _case(kind, N)
    kw = dict(F_ext=Fx, forcing=fx, dtype=dtype, observations=obs if with_obs else None)
    ref = _run(p, N, E, per_step_streams=1, **kw)
    assert ref[1].abs().sum() > 0 and (not with_obs or ref[4].abs().sum() > 0)
    plain = _run(_plain(p), N, E, per_step_streams=1, F_ext=Fx, dtype=dtype)
    assert not torch.equal(plain[1], ref[1])                      # the scales do something
    runs = {
        "per_step/2": _run(p, N, E, per_step_streams=2, **kw),
        "graph": _run(p, N, E, "graph", **kw),
        "fused/None": _run(p, N, E, "fused", fused_span=None, **kw),
        "fused/7": _run(p, N, E, "fused", fused_span=7, **kw),
        "ksteps/8": _run(p, N, E, "ksteps", **kw),
        "auto": _run(p, N, E, "auto", **kw),
        "chunk-major": _run(p, N, E, chunk_members=1024, per_step_streams=1, **kw),
        "chunk-major/graph": _run(p, N, E, "graph", chunk_members=1024, **kw),
        "split": _run(p, N, E, split=(101, "per_step", "per_step"), **kw),
        "split/mixed": _run(p, N, E, split=(126, "fused", "per_step"), **kw),
    }
    if dtype == torch.float32:
        runs["unpacked/per_step"] = _run(p, N, E, packing=0, **kw)
        runs["unpacked/fused"] = _run(p, N, E, "fused", packing=0, **kw)
    for name, got in runs.items():
        assert len(got) == len(ref) and all(torch.equal(a, b) for a, b in zip(got, ref)), (name, kind, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("form", [_capi.FORM_PER_STEP, _capi.FORM_FUSED])
def test_a_sub_range_starting_at_an_odd_member_through_the_c_abi(dtype, form):
    """Members [m0, m0 + n) of the engine's rows with m0 odd (fp32: rows not 8-byte aligned, the one-member-per-lane kernels)
    give the bits of the whole-ensemble run, and nothing outside the range is written."""
    N, m0, n = 1000, 333, 258
    p, E, fx, Fx = _case("multigas", N)
    whole = EnsembleEngine(p, N, E, F_ext=Fx, forcing=fx, dtype=dtype, device="cuda:0")
    whole.run(mode="per_step")
    eng = EnsembleEngine(p, N, E, F_ext=Fx, forcing=fx, dtype=dtype, device="cuda:0")
    w = eng._w
    a = eng._run_args(0, N_STEPS, m0, n)
    rc = eng._fn("run_forc")(*a, eng._ptr(eng.fscale, m0 * w), eng._ptr(eng.fext), 3, None, None, form, 0, eng._stream())
    _capi.check(eng.lib, rc)
    torch.cuda.synchronize()
    for name in ("C", "T", "R", "S"):
        got, want = getattr(eng, name), getattr(whole, name)
        assert torch.equal(got[..., m0:m0 + n], want[..., m0:m0 + n]), name
        assert not got[..., :m0].any() and not got[..., m0 + n:].any(), name
    whole.close()
    eng.close()


# ---- 4. the misfit rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["co2", "multigas"])
def test_misfit_rows_are_misfit_numpy_of_the_stored_T_bit_for_bit(kind, dtype, obs):
    N = 2000 + 1
    p, E, fx, Fx = _case(kind, N)
    for mode in MODES:
        out = _run(p, N, E, mode, F_ext=Fx, forcing=fx, dtype=dtype, observations=obs)
        want = torch.from_numpy(constrain.misfit_numpy(out[1].numpy(), obs.table))
        assert torch.equal(out[4].view(torch.int64), want.view(torch.int64)), (kind, mode)


# ---- 5. fp32 against the CPU reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["co2", "multigas"])
def test_fp32_against_the_cpu_reference(kind):
    """The project's fp32 bounds (tests/test_golden_fiveeq.py): C 5e-6 relative, T 3e-5 relative + 2e-6 K.  The forcing of
    this case takes T through zero (volcanic spikes on a cooling aerosol ramp), which no fp32 check here did before."""
    N = 2048 + 1
    p, E, fx, Fx = _case(kind, N)
    ref = _reference(kind, N)
    for mode, packing in (("per_step", 1), ("fused", 1), ("fused", 0)):
        C, T = _run(p, N, E, mode, packing=packing, F_ext=Fx, forcing=fx, dtype=torch.float32)[:2]
        C, T = C.double().numpy(), T.double().numpy()
        errC = (np.abs(C - ref["C"]) / np.abs(ref["C"])).max()
        errT = (np.abs(T - ref["T"]) / (3e-5 * np.abs(ref["T"]) + 2e-6)).max()
        print(f"fp32 {kind} {mode} packing={packing}: C worst rel {errC:.3g} (bound 5e-6), T worst err/bound {errT:.3g}")
        assert np.isfinite(C).all() and np.isfinite(T).all()
        assert errC <= 5e-6, (kind, mode, float(errC))
        assert errT <= 1.0, (kind, mode, float(errT))


# ---- 6. checkpoints, branching, accounting, refusals ---------------------------------------------------------------------------
def test_checkpoint_round_trip_mid_run(obs):
    N = 1500
    p, E, fx, Fx = _case("multigas", N)
    kw = dict(F_ext=Fx, forcing=fx, observations=obs, device="cuda:0")
    straight = EnsembleEngine(p, N, E, **kw)
    straight.run(mode="per_step")
    first = EnsembleEngine(p, N, E, **kw)
    first.run(0, 140, mode="fused")
    state = first.state_dict()
    assert state["forcing_sha256"] == fx.sha256 and len(state["fscale_sha256"]) == 64
    second = EnsembleEngine(p, N, E, **kw)
    second.load_state_dict(state)
    second.run(state["t_next"], N_STEPS, mode="per_step")
    torch.cuda.synchronize()
    for name in ("R", "S", "misfit"):
        assert torch.equal(getattr(second, name), getattr(straight, name)), name
    assert torch.equal(second.T[140:], straight.T[140:]) and torch.equal(second.C[140:], straight.C[140:])
    # another table, other scale rows, or no forcing at all: refused, with the engine as it was
    other_p = dict(p, fx_scale=np.asarray(p["fx_scale"]) * 1.01)
    for eng in (EnsembleEngine(p, N, E, **dict(kw, forcing=ExternalForcings(fx.table * 0.5, fx.names))),
                EnsembleEngine(other_p, N, E, **kw),
                EnsembleEngine(_plain(p), N, E, F_ext=Fx, observations=obs, device="cuda:0")):
        with pytest.raises(ValueError, match="forcing set"):
            eng.load_state_dict(state)
        assert eng.t_next == 0 and not eng.R.any()
        eng.close()
    first.fscale[3] *= 1.5                                        # rows edited after a checkpoint was taken: a new set
    assert first.state_dict()["fscale_sha256"] != state["fscale_sha256"]
    with pytest.raises(ValueError, match="forcing set"):
        first.load_state_dict(EnsembleEngine(_plain(p), N, E, F_ext=Fx, observations=obs, device="cuda:0").state_dict())
    for eng in (straight, first, second):
        eng.close()


def test_a_projection_branches_from_a_history_run_through_R0_S0():
    N, cut = 1200, 170
    p, E, fx, Fx = _case("multigas", N)
    whole = EnsembleEngine(p, N, E, F_ext=Fx, forcing=fx, device="cuda:0")
    whole.run(mode="fused")
    hist = EnsembleEngine(p, N, E[:cut], F_ext=Fx[:cut], forcing=ExternalForcings(fx.table[:cut], fx.names), device="cuda:0")
    hist.run(mode="per_step")
    torch.cuda.synchronize()
    assert torch.equal(hist.T, whole.T[:cut])
    # the projection: the whole drive table (cumulative emissions continue), started at the cut from the history's state
    proj = EnsembleEngine(p, N, E, F_ext=Fx, forcing=fx, R0=hist.R, S0=hist.S, device="cuda:0")
    proj.run(cut, N_STEPS, mode="ksteps", k_steps=16)
    torch.cuda.synchronize()
    assert torch.equal(proj.T[cut:], whole.T[cut:]) and torch.equal(proj.R, whole.R)
    for eng in (whole, hist, proj):
        eng.close()


def test_byte_accounting_and_refusals(obs):
    N = 512
    p, E, fx, Fx = _case("multigas", N)
    eng = EnsembleEngine(p, N, E, F_ext=Fx, forcing=fx, device="cuda:0")
    plain = EnsembleEngine(_plain(p), N, E, F_ext=Fx, device="cuda:0")
    assert plain.bytes_per_member_step("per_step") == 248.0
    assert eng.bytes_per_member_step("per_step") == 248.0 + 8 * (3 + 3)
    assert eng.bytes_per_member_step("ksteps", 8) == plain.bytes_per_member_step("ksteps", 8) + 8 * 6 / 8
    assert tuple(eng.fscale.shape) == (6, N) and eng.small_form() == 0
    assert eng.resolve_mode("auto")[0] in ("per_step", "ksteps")
    with pytest.raises(ValueError, match="mode 'small'"):
        eng.run(mode="small")
    eng.close()
    plain.close()
    refusals = [
        (dict(hist=(-1.0, 3.0, 64)), "hist="),
        (dict(concentration_driven=True), "concentration_driven"),
        (dict(compensated=True, dtype=torch.float32), "compensated"),
    ]
    for kw, needle in refusals:
        with pytest.raises(ValueError, match=needle):
            EnsembleEngine(p, N, E, F_ext=Fx, forcing=fx, device="cuda:0", **kw)
    with pytest.raises(ValueError, match="scenario"):
        EnsembleEngine(p, N, np.stack([E, E]), forcing=fx, device="cuda:0")
    with pytest.raises(ValueError, match="steps for a run"):
        EnsembleEngine(p, N, E[:100], forcing=fx, device="cuda:0")
    with pytest.raises(ValueError, match="need forcing="):
        EnsembleEngine(p, N, E, device="cuda:0")
    with pytest.raises(ValueError, match="fx_scale"):
        EnsembleEngine(dict(p, fx_scale=np.ones((2, N))), N, E, forcing=fx, device="cuda:0")


def test_device_sampler_is_the_host_sampler_bit_for_bit():
    base = prm.default_params("multigas")
    ranges = [(0.8, 1.2)] * 3 + [(0.3, 2.0)]
    host = prm.sample_forcing_scales(base, 100000, 777, 5000, ranges)
    dev = prm.sample_forcing_scales(base, 100000, 777, 5000, ranges, device="cuda:0")
    assert dev.dtype == torch.float64 and np.array_equal(dev.cpu().numpy(), host)
    # ... and device rows go into the engine as they are
    N = 5000 - 777
    p = prm.sample_ensemble_shard(base, 100000, 777, 5000, device="cuda:0")
    p["f_scale"], p["fx_scale"] = dev[:3], dev[3:]
    E, fx, Fx = _table()
    fx1 = ExternalForcings(fx.table[:, :1], fx.names[:1])
    eng = EnsembleEngine(p, N, E, F_ext=Fx, forcing=fx1, device="cuda:0")
    assert np.array_equal(eng.fscale.cpu().numpy(), host)
    eng.run(mode="fused")
    torch.cuda.synchronize()
    assert torch.isfinite(eng.T).all()
    eng.close()

