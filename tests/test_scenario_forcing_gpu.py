"""Per-member forcing scales under the scenario axis on the MI355X (include/fiveeq.h "FORCING SCALES UNDER THE SCENARIO AXIS"):
member-scenario (m, s) of a scenario engine with forcing=ScenarioForcings is bit for bit member m of a single-scenario
forcing= engine on scenario s's emissions, F_ext and category table — in every run form, precision and packing — and agrees
pointwise with the NumPy restatement; the tables are read per scenario, unit scales are the plain scenario engine, sub-ranges
write nothing outside themselves, and statistics, summaries, checkpoints and the branch workflow carry over."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from fiveeqscm_amd import _capi, emissions, scenario
from fiveeqscm_amd import params as prm
from fiveeqscm_amd.constrain import Observations
from fiveeqscm_amd.engine import EnsembleEngine
from fiveeqscm_amd.forcing import ExternalForcings, ScenarioForcings
from forcing_reference import forcing_numpy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GASES = {"co2": 1, "multigas": 3}
NAMES = ("aerosol", "volcanic", "solar", "other")
CO2_FACTORS = (0.5, 1.0, 1.5, 0.75, 1.25)
KEYS = ("C", "T", "R", "S")


def _inputs(kind, S, K, n_steps, cut):
    """(E [S, n_steps, G], F_ext [S, n_steps], ScenarioForcings [S, n_steps, K]): the scenarios share the history [0, cut) and
    scale the CO2 emissions after it; the aerosol table is proportional to the scenario's own CO2 emissions, the volcanic one
    spikes (the same in every scenario), then an 11-step sinusoid and a ramp that differs by scenario."""
    G = GASES[kind]
    base = emissions.rcp_like_emissions(n_steps, G)
    tt = np.arange(n_steps)
    E = np.repeat(base[None], S, axis=0)
    for s in range(S):
        E[s, cut:, 0] *= CO2_FACTORS[s % len(CO2_FACTORS)] * (1.0 + 0.01 * (s // len(CO2_FACTORS)))
    F = np.stack([0.05 * s * np.sin(tt / (7.0 + s)) + 0.02 * tt / n_steps for s in range(S)])
    cols = [-1.1 * E[:, :, 0] / base[:, 0].max(),
            np.repeat(np.where(tt % 37 == 5, -2.5, 0.0)[None], S, axis=0),
            np.repeat((0.1 * np.sin(2 * np.pi * tt / 11.0))[None], S, axis=0),
            np.stack([np.where(tt >= cut, 0.002 * (s + 1) * (tt - cut), 0.0) for s in range(S)])]
    return E, F, ScenarioForcings(np.stack(cols[:K], axis=2) if K else np.zeros((S, n_steps, 0)), NAMES[:K])


@functools.lru_cache(maxsize=None)
def _params(kind, N, K):
    """Parameters with scale rows: gas scales in (0.8, 1.2), aerosol (0.3, 2.0), volcanic and the others (0.5, 1.5)."""
    G = GASES[kind]
    base = prm.default_params(kind)
    p = prm.sample_ensemble_shard(base, N)
    s = prm.sample_forcing_scales(base, N, ranges=([(0.8, 1.2)] * G + [(0.3, 2.0), (0.5, 1.5), (0.5, 1.5), (0.5, 1.5)])[:G + K],
                                  seed=7)
    p["f_scale"] = s[:G]
    if K:
        p["fx_scale"] = s[G:]
    return p


def _plain(p):
    return {k: v for k, v in p.items() if k not in ("f_scale", "fx_scale")}


def _out(eng, keys=KEYS):
    torch.cuda.synchronize()
    return {k: getattr(eng, k).cpu() for k in keys}


def _single(p, N, E, F, sf, s, mode="per_step", keys=KEYS, **kw):
    """Scenario s alone: a single-scenario forcing= engine on its emissions, F_ext and table."""
    eng = EnsembleEngine(p, N, E[s], F_ext=F[s], forcing=sf.scenario(s), device="cuda:0", **kw)
    eng.run(mode=mode)
    out = _out(eng, keys)
    eng.close()
    return out


def _scen(p, N, E, F, sf, mode="per_step", split=None, run_kw=None, keys=KEYS, **kw):
    eng = EnsembleEngine(p, N, E, F_ext=F, forcing=sf, device="cuda:0", **kw)
    if split:
        eng.run(0, split[0], mode=split[1])
        eng.run(split[0], eng.n_steps, mode=split[2])
    else:
        eng.run(mode=mode, **(run_kw or {}))
        assert eng.last_mode != "small"
    out = _out(eng, keys)
    eng.close()
    return out


def _assert_scenarios(got, singles, what):
    for s, ref in enumerate(singles):
        for k in ref:
            assert torch.equal(got[k][s], ref[k]), (what, s, k)


# ---- 1. bit identity with single-scenario forcing engines ----------------------------------------------------------------
FORMS = [("per_step", dict(), None), ("graph", dict(), None), ("fused", dict(fused_span=None), None),
         ("fused", dict(fused_span=7), None), ("ksteps", dict(), dict(k_steps=8)), ("auto", dict(), None)]
# 37 is a refill boundary of no fused form (they stage 25 or 125 steps per refill)
SPLITS = [(37, "fused", "fused"), (37, "per_step", "fused"), (37, "fused", "per_step")]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["co2", "multigas"])
def test_every_member_scenario_is_the_single_scenario_forcing_engine_bit_for_bit(kind, dtype):
    """N in {1, 63, 64, 65, 1000, 4133} x S in {1, 2, 5} x K in {0, 1, 2, 4}: odd N (and N = 1) run fp32 one member per lane,
    even N two; 140 steps cross the refills of both staging lengths.  Every run form, and runs split at step 37."""
    n_steps, cut = 140, 50
    for N in (1, 63, 64, 65, 1000, 4133):
        for K in (0, 1, 2, 4):
            p = _params(kind, N, K)
            E5, F5, sf5 = _inputs(kind, 5, K, n_steps, cut)
            singles = [_single(p, N, E5, F5, sf5, s, dtype=dtype) for s in range(5)]
            assert all(r["T"].abs().sum() > 0 for r in singles)
            for S in (1, 2, 5):
                E, F, sf = E5[:S], F5[:S], ScenarioForcings(sf5.table[:S], sf5.names)
                for mode, kw, run_kw in FORMS:
                    got = _scen(p, N, E, F, sf, mode, run_kw=run_kw, dtype=dtype, **kw)
                    assert tuple(got["T"].shape) == (S, n_steps, N)
                    _assert_scenarios(got, singles[:S], (kind, dtype, N, S, K, mode, kw))
                for split in SPLITS:
                    got = _scen(p, N, E, F, sf, split=split, dtype=dtype)
                    _assert_scenarios(got, singles[:S], (kind, dtype, N, S, K, split))


@pytest.mark.parametrize("kind", ["co2", "multigas"])
def test_fp32_packed_and_unpacked_lanes_give_the_same_bits(kind):
    N, S, K, n_steps = 1000, 3, 2, 140
    p = _params(kind, N, K)
    E, F, sf = _inputs(kind, S, K, n_steps, 50)
    lib = _capi.load()
    runs = {}
    for packing in (1, 0):
        prev = lib.fiveeq_set_f32_packing(packing)
        try:
            for mode in ("per_step", "fused"):
                runs[(packing, mode)] = _scen(p, N, E, F, sf, mode, dtype=torch.float32)
        finally:
            lib.fiveeq_set_f32_packing(prev)
    ref = runs[(1, "per_step")]
    for key, got in runs.items():
        assert all(torch.equal(got[k], ref[k]) for k in KEYS), (kind, key)


# ---- 2. pointwise against the NumPy restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["co2", "multigas"])
def test_fp64_pointwise_against_the_numpy_restatement_per_scenario(kind):
    """rcp_like_emissions over 750 steps, CO2 scaled by 0.5 / 1.0 / 1.5 after step 270, gas scales in (0.8, 1.2), aerosol
    scales in (0.3, 2.0) on a table proportional to the scenario's CO2 emissions, volcanic scales in (0.5, 1.5) on spikes,
    F_ext per scenario.  Every stored C and T of every member, scenario and step within |a - b| <= 1e-10 |b| + 1e-13."""
    N, S, K, n_steps = 256, 3, 2, 750
    G = GASES[kind]
    p = _params(kind, N, K)
    E, F, sf = _inputs(kind, S, K, n_steps, 270)
    assert [float(E[s, 300, 0] / E[1, 300, 0]) for s in range(S)] == [0.5, 1.0, 1.5]
    refs = [forcing_numpy(E[s], p, N, sf.table[s], p["f_scale"], p["fx_scale"], F_ext=F[s]) for s in range(S)]
    T_all = np.stack([r["T"] for r in refs])
    assert np.isfinite(T_all).all() and all(np.isfinite(r["C"]).all() for r in refs)
    print(f"{kind}: reference T from {T_all.min():.3g} to {T_all.max():.3g} K, smallest |T| {np.abs(T_all).min():.3g}")
    assert int((np.sign(T_all[:, 1:]) != np.sign(T_all[:, :-1])).sum()) > 0   # T goes through zero ...
    assert np.abs(T_all).min() < 1e-7 and T_all.min() < -0.4 and T_all.max() > 3.5     # ... closely: the absolute term is used
    for mode in ("per_step", "fused"):
        got = _scen(p, N, E, F, sf, mode, keys=("C", "T"))
        for s in range(S):
            for name in ("C", "T"):
                a, b = got[name][s].numpy(), refs[s][name]
                assert a.shape == b.shape == ((n_steps, G, N) if name == "C" else (n_steps, N))
                err = np.abs(a - b) / (1e-10 * np.abs(b) + 1e-13)
                print(f"{kind} {mode} scenario {s} {name}: worst err/bound {err.max():.3g}")
                assert np.isfinite(a).all() and err.max() <= 1.0, (kind, mode, s, name, float(err.max()))


# ---- 3. unit scales are the plain scenario engine ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["co2", "multigas"])
def test_unit_scales_are_the_plain_scenario_engine_bit_for_bit(kind, dtype):
    """Unit scales with K = 0 (through the engine, and through the C ABI with fext = NULL, which the contract says is not
    read), and any finite scales on an all-zero table: the bits of the scenario engine without forcing=.  64 members over
    300 steps: several refills of either staging length, scale rows far shorter than a table."""
    N, S, n_steps = 64, 3, 300
    G = GASES[kind]
    p = _plain(_params(kind, N, 0))
    E, F, _ = _inputs(kind, S, 0, n_steps, 120)
    assert G * N < 4 * n_steps
    plain = EnsembleEngine(p, N, E, F_ext=F, dtype=dtype, device="cuda:0")
    plain.run(mode="per_step")
    want = _out(plain, KEYS)
    plain.close()
    none = ScenarioForcings(np.zeros((S, n_steps, 0)))
    zero = ScenarioForcings(np.zeros((S, n_steps, 3)))
    any_sx = dict(p, fx_scale=np.random.default_rng(5).uniform(-3.0, 3.0, (3, N)))
    for what, forcing, params in (("K=0", none, p), ("zero table", zero, p), ("zero table, any sx", zero, any_sx)):
        for mode, kw, run_kw in FORMS:
            got = _scen(params, N, E, F, forcing, mode, run_kw=run_kw, dtype=dtype, **kw)
            assert all(torch.equal(got[k], want[k]) for k in KEYS), (kind, dtype, what, mode, kw)
    for form, k in ((_capi.FORM_FUSED, 0), (_capi.FORM_FUSED, 90), (_capi.FORM_PER_STEP, 0)):
        eng = EnsembleEngine(p, N, E, F_ext=F, dtype=dtype, forcing=none, device="cuda:0")
        a = eng._run_args(0, n_steps, n_scen=S)
        rc = eng._fn("run_scen_forc")(*a, eng._ptr(eng.fscale), None, 0, form, k, eng._stream())
        _capi.check(eng.lib, rc)
        got = _out(eng)
        assert all(torch.equal(got[k], want[k]) for k in KEYS), (kind, dtype, form, k)
        plan = ctypes.c_void_p()
        eng.reset_state()
        rc = eng._fn("plan_create_scen_forc")(*a, eng._ptr(eng.fscale), None, 0, ctypes.byref(plan))
        _capi.check(eng.lib, rc)
        _capi.check(eng.lib, eng.lib.fiveeq_plan_launch(plan, eng._stream()))
        torch.cuda.synchronize()
        assert torch.equal(eng.T.cpu(), want["T"]) and torch.equal(eng.R.cpu(), want["R"]), (kind, dtype, "plan")
        eng.lib.fiveeq_plan_destroy(plan)
        eng.close()


# ---- 4. the tables are read per scenario -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("mode", ["per_step", "fused"])
def test_each_scenario_reads_its_own_table(mode, dtype):
    """Two scenarios with EQUAL emissions and F_ext but different tables: their T differ, and swapping the tables swaps the
    results bit for bit."""
    N, K, n_steps = 1000, 2, 140
    p = _params("multigas", N, K)
    E3, F3, sf3 = _inputs("multigas", 3, K, n_steps, 50)
    E, F = np.stack([E3[1], E3[1]]), np.stack([F3[1], F3[1]])
    tabs = np.stack([sf3.table[0], sf3.table[2]])
    assert not np.array_equal(tabs[0], tabs[1])
    ab = _scen(p, N, E, F, ScenarioForcings(tabs, sf3.names), mode, dtype=dtype)
    ba = _scen(p, N, E, F, ScenarioForcings(tabs[::-1], sf3.names), mode, dtype=dtype)
    assert not torch.equal(ab["T"][0], ab["T"][1]) and not torch.equal(ab["S"][0], ab["S"][1])
    for k in KEYS:
        assert torch.equal(ab[k][0], ba[k][1]) and torch.equal(ab[k][1], ba[k][0]), (mode, k)
    same = _scen(p, N, E, F, ScenarioForcings.shared(ExternalForcings(tabs[0], sf3.names), 2), mode, dtype=dtype)
    for k in KEYS:
        assert torch.equal(same[k][0], same[k][1]) and torch.equal(same[k][0], ab[k][0]), (mode, k)


# ---- 5. sub-ranges, ld > n, chunks and stream halves ----------------------------------------------------------------------------
@pytest.mark.parametrize("m0,n", [(320, 258), (333, 258), (0, 1), (999, 1)])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("form", [_capi.FORM_PER_STEP, _capi.FORM_FUSED])
def test_a_member_sub_range_writes_nothing_outside_itself(form, dtype, m0, n):
    """Members [m0, m0 + n) of rows of length ld = 1000 > n through the C ABI (m0 odd: fp32 rows not 8-byte aligned, the
    one-member-per-lane kernels): inside, the bits of the whole-ensemble run; outside, sentinels in the state, the stored
    rows and the statistics records stay as they were, in every scenario."""
    N, S, K, n_steps = 1000, 3, 2, 60
    p = _params("multigas", N, K)
    E, F, sf = _inputs("multigas", S, K, n_steps, 20)
    whole = EnsembleEngine(p, N, E, F_ext=F, forcing=sf, dtype=dtype, collect_stats=True, device="cuda:0")
    whole.run(mode="per_step")
    eng = EnsembleEngine(p, N, E, F_ext=F, forcing=sf, dtype=dtype, collect_stats=True, device="cuda:0")
    eng._wave_stats()
    SENT = -777.25
    inside = torch.zeros(N, dtype=torch.bool, device="cuda:0")
    inside[m0:m0 + n] = True
    for name in KEYS:
        getattr(eng, name)[..., ~inside] = SENT
    w0, w1 = m0 // 64, m0 // 64 + (n + 63) // 64                  # the records this call addresses
    eng.T_stats[:] = SENT
    a = eng._run_args(0, n_steps, m0, n, n_scen=S)
    rc = eng._fn("run_scen_forc")(*a, eng._ptr(eng.fscale, m0 * eng._w), eng._ptr(eng.fext), K, form, 0, eng._stream())
    _capi.check(eng.lib, rc)
    torch.cuda.synchronize()
    for name in KEYS:
        got, want = getattr(eng, name), getattr(whole, name)
        assert torch.equal(got[..., inside], want[..., inside]), name
        assert bool((got[..., ~inside] == SENT).all()), name
    st = eng.T_stats
    assert bool((st[:, :w0] == SENT).all()) and bool((st[:, w1:] == SENT).all())
    assert not bool((st[:, w0:w1] == SENT).any())
    if m0 % 64 == 0 and n >= 64:                                   # whole waves of the range are whole waves of the ensemble
        full = w0 + n // 64
        assert torch.equal(st[:, w0:full, :, 2:], whole.T_stats[:, w0:full, :, 2:])       # min, max: exact in either form
    whole.close()
    eng.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_chunks_and_two_stream_halves_are_bit_identical_to_one_launch(dtype):
    N, S, K, n_steps = 3000 + 1, 3, 2, 140
    p = _params("multigas", N, K)
    E, F, sf = _inputs("multigas", S, K, n_steps, 50)
    want = _scen(p, N, E, F, sf, chunk_members=None, per_step_streams=1, dtype=dtype)
    for kw in (dict(chunk_members=1024), dict(per_step_streams=2), dict(chunk_members=1024, per_step_streams=2)):
        for mode in ("per_step", "graph"):
            eng = EnsembleEngine(p, N, E, F_ext=F, forcing=sf, dtype=dtype, device="cuda:0", **kw)
            assert len(eng.per_step_launches()) > 1
            eng.run(mode=mode)
            got = _out(eng)
            eng.close()
            assert all(torch.equal(got[k], want[k]) for k in KEYS), (kw, mode)
    got = _scen(p, N, E, F, sf, split=(37, "per_step", "graph"), chunk_members=1024, per_step_streams=2, dtype=dtype)
    assert all(torch.equal(got[k], want[k]) for k in KEYS)


# ---- 6. graph replay ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_graph_replay_equals_eager(dtype):
    N, S, K, n_steps = 1000, 3, 4, 140
    p = _params("multigas", N, K)
    E, F, sf = _inputs("multigas", S, K, n_steps, 50)
    want = _scen(p, N, E, F, sf, "per_step", dtype=dtype)
    eng = EnsembleEngine(p, N, E, F_ext=F, forcing=sf, dtype=dtype, device="cuda:0")
    plans = eng.prepare_graph()
    for replay in range(3):                                        # the same captured plans, replayed from the initial state
        eng.reset_state()
        eng.C.zero_()
        eng.T.zero_()
        eng.run(mode="graph")
        assert eng.prepare_graph() is plans
        got = _out(eng)
        assert all(torch.equal(got[k], want[k]) for k in KEYS), replay
    eng.close()


# ---- 7. statistics and summaries ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["per_step", "fused"])
def test_statistics_and_summaries_equal_the_single_scenario_forcing_engine(mode):
    N, S, K, n_steps = 3000, 3, 2, 140
    p = _params("multigas", N, K)
    E, F, sf = _inputs("multigas", S, K, n_steps, 50)
    eng = EnsembleEngine(p, N, E, F_ext=F, forcing=sf, collect_stats=True, device="cuda:0")
    eng.run(mode=mode)
    steps = [10, 50, n_steps - 1]
    keep = torch.from_numpy(np.random.default_rng(5).random(N) < 0.4).to("cuda:0")
    for s in range(S):
        one = EnsembleEngine(p, N, E[s], F_ext=F[s], forcing=sf.scenario(s), collect_stats=True, device="cuda:0")
        one.run(mode=mode)
        assert torch.equal(eng.stats_sums(scenario=s).cpu(), one.stats_sums().cpu()), s
        for k, v in one.stats().items():
            assert torch.equal(torch.as_tensor(eng.stats(scenario=s)[k]).cpu(), torch.as_tensor(v).cpu()), (s, k)
        for kw in (dict(), dict(accepted=keep), dict(gas=0, accepted=keep)):
            a, b = eng.gather_summary(steps, scenario=s, **kw), one.gather_summary(steps, **kw)
            assert sorted(a) == sorted(b)
            for k in a:
                assert torch.equal(torch.as_tensor(a[k]).cpu(), torch.as_tensor(b[k]).cpu()), (s, kw.keys(), k)
        one.close()
    with pytest.raises(ValueError, match="scenario"):
        eng.stats()
    eng.close()


# ---- 8. the branch workflow -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_scenario_projection_branches_from_a_constrained_forcing_history(dtype):
    """History: one scenario, forcing= + observations=, to t_branch.  Projection: a scenario engine over the whole timeline with
    per-scenario tables and the same scale rows, started from the history's state.  From t_branch on it is, bit for bit, the
    whole-timeline single-scenario forcing runs."""
    N, S, K, n_steps, cut = 1200, 3, 2, 300, 170
    p = _params("multigas", N, K)
    E, F, sf = _inputs("multigas", S, K, n_steps, cut)
    assert all(np.array_equal(E[s, :cut], E[0, :cut]) and np.array_equal(sf.table[s, :cut], sf.table[0, :cut]) for s in range(S))
    F[:, :cut] = F[0, :cut]                                        # one history
    y, T_obs, sig = scenario.read_observations_csv(os.path.join(ROOT, "tests", "golden", "obs_synthetic.csv"))
    years = 1750.0 + np.arange(cut)
    keep = y < years[-1]
    obs = Observations.from_years(years, y[keep], T_obs[keep], sig[keep], baseline=(1850, 1900))
    hist = EnsembleEngine(p, N, E[0, :cut], F_ext=F[0, :cut], forcing=ExternalForcings(sf.table[0, :cut], sf.names),
                          observations=obs, dtype=dtype, store_trajectory=False, device="cuda:0")
    hist.run(mode="fused")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(hist.chi2()).all())
    refs = [_single(p, N, E, F, sf, s, dtype=dtype) for s in range(S)]
    for mode in ("auto", "per_step", "fused"):
        proj = EnsembleEngine(p, N, E, F_ext=F, forcing=sf, R0=hist.R, S0=hist.S, dtype=dtype, device="cuda:0")
        proj.run(cut, n_steps, mode=mode)
        got = _out(proj)
        proj.close()
        for s, ref in enumerate(refs):
            assert torch.equal(got["R"][s], ref["R"]) and torch.equal(got["S"][s], ref["S"]), (mode, s)
            assert torch.equal(got["T"][s][cut:], ref["T"][cut:]) and torch.equal(got["C"][s][cut:], ref["C"][cut:]), (mode, s)
    hist.close()


def test_checkpoint_round_trip_and_refusals_on_the_engine():
    N, S, K, n_steps = 1500, 3, 2, 140
    p = _params("multigas", N, K)
    E, F, sf = _inputs("multigas", S, K, n_steps, 50)
    kw = dict(F_ext=F, forcing=sf, device="cuda:0")
    straight = EnsembleEngine(p, N, E, **kw)
    straight.run(mode="per_step")
    first = EnsembleEngine(p, N, E, **kw)
    first.run(0, 61, mode="fused")
    state = first.state_dict()
    assert state["forcing_sha256"] == sf.sha256 and len(state["fscale_sha256"]) == 64 and state["n_scenarios"] == S
    second = EnsembleEngine(p, N, E, **kw)
    second.load_state_dict(state)
    second.run(state["t_next"], n_steps, mode="per_step")
    torch.cuda.synchronize()
    for name in ("R", "S"):
        assert torch.equal(getattr(second, name), getattr(straight, name)), name
    assert torch.equal(second.T[:, 61:], straight.T[:, 61:]) and torch.equal(second.C[:, 61:], straight.C[:, 61:])
    other_p = dict(p, fx_scale=np.asarray(p["fx_scale"]) * 1.01)
    for eng in (EnsembleEngine(p, N, E, **dict(kw, forcing=ScenarioForcings(sf.table * 0.5, sf.names))),
                EnsembleEngine(p, N, E, **dict(kw, forcing=ScenarioForcings(sf.table[::-1], sf.names))),
                EnsembleEngine(other_p, N, E, **kw),
                EnsembleEngine(_plain(p), N, E, F_ext=F, device="cuda:0")):
        with pytest.raises(ValueError, match="forcing set"):
            eng.load_state_dict(state)
        assert eng.t_next == 0 and not eng.R.any()
        eng.close()
    for eng in (straight, first, second):
        eng.close()


# ---- 9. byte accounting and the refusals ----------------------------------------------------------------------------------------
def test_byte_accounting_counts_the_shared_scale_rows_once_per_member():
    N, S, K = 512, 4, 2
    p = _params("multigas", N, K)
    E, F, sf = _inputs("multigas", S, K, 60, 20)
    w, SP, G = 8, 6, 3
    eng = EnsembleEngine(p, N, E, F_ext=F, forcing=sf, store_trajectory=False, device="cuda:0")
    plain = EnsembleEngine(_plain(p), N, E, F_ext=F, store_trajectory=False, device="cuda:0")
    one = EnsembleEngine(p, N, E[0], F_ext=F[0], forcing=sf.scenario(0), store_trajectory=False, device="cuda:0")
    assert plain.bytes_per_member_step("per_step") == w * (2 * SP + 4) + w * (3 * G + 2) / S
    assert eng.bytes_per_member_step("per_step") == w * (2 * SP + 4) + w * (3 * G + 2 + G + K) / S == 160.0
    assert one.bytes_per_member_step("per_step") == w * (2 * SP + 3 * G + 6 + G + K) == 256.0
    # the scale rows are the part the scenario loop amortises: the forcing form's ratio is below the plain form's
    plain_one = w * (2 * SP + 3 * G + 6)
    assert eng.bytes_per_member_step("per_step") / 256.0 < plain.bytes_per_member_step("per_step") / plain_one
    assert eng.bytes_per_member_step("ksteps", 8) == plain.bytes_per_member_step("ksteps", 8) + w * (G + K) / 8
    stored = EnsembleEngine(p, N, E, F_ext=F, forcing=sf, device="cuda:0")
    assert stored.bytes_per_member_step("per_step") == 160.0 + w * (G + 1)
    assert tuple(eng.fscale.shape) == (G + K, N) and tuple(eng.fext.shape) == (S, 60, 4)
    # the schedules count them once per member too
    rows = S * (SP + 2) + 3 * G + 2 + (G + K)                     # per member: S states, one set of parameter and scale rows
    fits = (256 << 20) // (w * rows)
    assert EnsembleEngine.auto_chunk(fits, SP, G, torch.float64, n_scenarios=S, extra_rows=G + K) == 0
    assert EnsembleEngine.auto_chunk(fits + 1, SP, G, torch.float64, n_scenarios=S, extra_rows=G + K) > 0
    assert EnsembleEngine.auto_chunk(fits + 1, SP, G, torch.float64, n_scenarios=S, extra_rows=0) == 0
    assert eng.small_form() == 0 and eng.resolve_mode("auto")[0] in ("per_step", "ksteps")
    for e in (eng, plain, one, stored):
        e.close()


def test_the_refusals():
    N, S, K, n_steps = 256, 2, 2, 60
    p = _params("multigas", N, K)
    E, F, sf = _inputs("multigas", S, K, n_steps, 20)
    fx = sf.scenario(0)
    # one table with several scenarios: still refused, naming the scenario axis and pointing to ScenarioForcings
    with pytest.raises(ValueError, match="scenario axis") as exc:
        EnsembleEngine(p, N, E, F_ext=F, forcing=fx, device="cuda:0")
    assert "ScenarioForcings" in str(exc.value)
    with pytest.raises(ValueError, match="several scenarios"):
        EnsembleEngine(p, N, E[0], F_ext=F[0], forcing=sf, device="cuda:0")      # ScenarioForcings with 2-D emissions
    with pytest.raises(ValueError, match="tables of 3 scenarios for emissions of 2"):
        EnsembleEngine(p, N, E, F_ext=F, forcing=ScenarioForcings.shared(fx, 3), device="cuda:0")
    with pytest.raises(ValueError, match="steps for a run"):
        EnsembleEngine(p, N, E[:, :40], F_ext=F[:, :40], forcing=sf, device="cuda:0")
    tab = np.zeros((n_steps, 4))
    tab[:10, 2] = 0.1
    for kw in (dict(observations=Observations(tab)), dict(hist=(-1.0, 5.0, 64)), dict(concentration_driven=True),
               dict(compensated=True, dtype=torch.float32)):
        with pytest.raises(ValueError, match="scenarios"):
            EnsembleEngine(p, N, E, F_ext=F, forcing=sf, device="cuda:0", **kw)
    with pytest.raises(ValueError, match="need forcing="):
        EnsembleEngine(p, N, E, F_ext=F, device="cuda:0")
    with pytest.raises(ValueError, match="fx_scale"):
        EnsembleEngine(dict(p, fx_scale=np.ones((3, N))), N, E, F_ext=F, forcing=sf, device="cuda:0")
    two_gas = {k: (v[:2] if k in ("a", "tau", "r0", "rC", "rT", "ra", "PI_conc", "emis2conc", "f") else v)
               for k, v in prm.default_params("multigas").items()}
    with pytest.raises(ValueError, match="no forcing form"):
        EnsembleEngine(prm.sample_ensemble(two_gas, N), N, E[:, :, :2], forcing=sf, device="cuda:0")
    eng = EnsembleEngine(p, N, E, F_ext=F, forcing=sf, small_lanes=1, device="cuda:0")
    with pytest.raises(ValueError, match="small"):
        eng.run(mode="small")
    eng.close()
