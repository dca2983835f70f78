"""The scenario axis on the MI355X: one parameter ensemble under S emission scenarios is, member-scenario by member-scenario,
bit for bit S single-scenario engines — in every mode, precision, packing, chunking and stream split — and agrees with the C
oracle; branching from a history run, per-scenario statistics and summaries, checkpoints and the refusals."""
import numpy as np
import pytest
import torch

from fiveeqscm_amd import _capi, emissions
from fiveeqscm_amd import params as prm
from fiveeqscm_amd.engine import EnsembleEngine

pytestmark = pytest.mark.gpu

N_STEPS = 300
T_BRANCH = 120
GAS_KEYS = ("a", "tau", "r0", "rC", "rT", "ra", "PI_conc", "emis2conc", "f")


def _scenarios(n_steps, S, G=3, t_branch=T_BRANCH):
    """S synthetic scenarios that share the history [0, t_branch) and scale future emissions low ... high; per-scenario
    F_ext."""
    base = emissions.rcp_like_emissions(n_steps, G)
    E = np.repeat(base[None], S, axis=0)
    for s in range(S):
        E[s, t_branch:] *= 0.4 + 0.35 * s
    t = np.arange(n_steps)
    F = np.stack([0.05 * s * np.sin(t / (7.0 + s)) for s in range(S)])
    return E, F


def _two_gas(base):
    return {k: (v[:2] if k in GAS_KEYS else v) for k, v in base.items()}


@pytest.fixture(scope="module")
def ens():
    N = 3000
    return prm.sample_ensemble(prm.default_params("multigas"), N), N


def _sync_cpu(t):
    torch.cuda.synchronize()
    return None if t is None else t.cpu()


def _singles(p, N, E, F, dtype, **kw):
    out = []
    for s in range(E.shape[0]):
        eng = EnsembleEngine(p, N, E[s], F_ext=F[s], dtype=dtype, device="cuda:0", **kw)
        eng.run(mode="per_step")
        out.append({k: _sync_cpu(getattr(eng, k)) for k in ("C", "T", "R", "S")})
        eng.close()
    return out


def _assert_equal_to_singles(eng, singles):
    got = {k: _sync_cpu(getattr(eng, k)) for k in ("C", "T", "R", "S")}
    for s, ref in enumerate(singles):
        for k in ("C", "T", "R", "S"):
            assert torch.equal(got[k][s], ref[k]), (s, k)


MODES = [("per_step", {}), ("graph", {}), ("fused", {"fused_span": None}), ("fused", {"fused_span": 128}),
         ("ksteps", {}), ("auto", {})]


@pytest.mark.parametrize("dtype,packing", [(torch.float64, 1), (torch.float32, 1), (torch.float32, 0)])
def test_every_mode_is_bit_identical_to_single_scenario_engines(ens, dtype, packing):
    p, N = ens
    E, F = _scenarios(N_STEPS, 4)
    lib = _capi.load()
    prev = lib.fiveeq_set_f32_packing(packing)
    try:
        singles = _singles(p, N, E, F, dtype)
        for mode, kw in MODES:
            eng = EnsembleEngine(p, N, E, F_ext=F, dtype=dtype, device="cuda:0", **kw)
            assert eng.n_scenarios == 4 and tuple(eng.T.shape) == (4, N_STEPS, N) and tuple(eng.R.shape) == (4, 6, N)
            eng.run(mode=mode, **({"k_steps": 8} if mode == "ksteps" else {}))
            assert eng.last_mode != "small"
            _assert_equal_to_singles(eng, singles)
            eng.close()
        # step() by step()
        eng = EnsembleEngine(p, N, E, F_ext=F, dtype=dtype, device="cuda:0")
        for t in range(N_STEPS):
            eng.step(t)
        _assert_equal_to_singles(eng, singles)
        eng.close()
    finally:
        lib.fiveeq_set_f32_packing(prev)


@pytest.mark.parametrize("kind", ["co2", "multigas", "two_gas"])
def test_fp64_against_the_c_oracle_for_each_scenario(kind):
    from oracle import c_oracle
    base = prm.default_params("multigas" if kind != "co2" else "co2")
    if kind == "two_gas":
        base = _two_gas(base)
    G = prm.n_gas_of(base)
    N = 1000
    p = prm.sample_ensemble(base, N)
    E, F = _scenarios(N_STEPS, 3, G)
    eng = EnsembleEngine(p, N, E, F_ext=F, device="cuda:0")
    eng.run(mode="per_step")
    C, T = _sync_cpu(eng.C).numpy(), _sync_cpu(eng.T).numpy()
    for s in range(3):
        want = c_oracle.run(E[s], p, N, F_ext=F[s])
        for name, got in (("C", C[s]), ("T", T[s])):
            err = np.abs(got - want[name]) / (1e-10 * np.abs(want[name]) + 1e-13)
            assert np.isfinite(got).all() and err.max() <= 1.0, (kind, s, name, float(err.max()))
    eng.close()


@pytest.mark.parametrize("N,dtype", [(1, torch.float64), (63, torch.float64), (65, torch.float32), (257, torch.float64),
                                     (101, torch.float32)])
def test_ragged_ensembles(N, dtype):
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    E, F = _scenarios(80, 3, t_branch=40)
    singles = _singles(p, N, E, F, dtype)
    for mode in ("per_step", "fused"):
        eng = EnsembleEngine(p, N, E, F_ext=F, dtype=dtype, device="cuda:0")
        eng.run(mode=mode)
        _assert_equal_to_singles(eng, singles)
        eng.close()


@pytest.mark.parametrize("S", [1, 3, 5, 64])
def test_scenario_counts(S):
    N = 300
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    E, F = _scenarios(60, S, t_branch=20)
    E = E * (1.0 + 0.01 * np.arange(S))[:, None, None]           # 64 distinct scenarios
    picks = sorted({0, S // 2, S - 1})
    singles = _singles(p, N, E[picks], F[picks], torch.float64)
    for mode in ("per_step", "ksteps"):
        eng = EnsembleEngine(p, N, E, F_ext=F, device="cuda:0")
        assert eng.n_scenarios == S and tuple(eng.T.shape) == (S, 60, N)
        eng.run(mode=mode, **({"k_steps": 16} if mode == "ksteps" else {}))
        got = {k: _sync_cpu(getattr(eng, k)) for k in ("C", "T", "R", "S")}
        for i, s in enumerate(picks):
            for k in ("C", "T", "R", "S"):
                assert torch.equal(got[k][s], singles[i][k]), (S, s, k, mode)
        eng.close()


def test_chunks_and_two_streams_are_bit_identical_to_one_launch(ens):
    p, N = ens
    E, F = _scenarios(N_STEPS, 3)
    ref = EnsembleEngine(p, N, E, F_ext=F, chunk_members=None, per_step_streams=1, device="cuda:0")
    ref.run(mode="per_step")
    want = {k: _sync_cpu(getattr(ref, k)) for k in ("C", "T", "R", "S")}
    for kw in ({"chunk_members": 1024}, {"per_step_streams": 2}, {"chunk_members": 1024, "per_step_streams": 2}):
        for mode in ("per_step", "graph"):
            eng = EnsembleEngine(p, N, E, F_ext=F, device="cuda:0", **kw)
            assert len(eng.per_step_launches()) > 1
            eng.run(mode=mode)
            for k in ("C", "T", "R", "S"):
                assert torch.equal(_sync_cpu(getattr(eng, k)), want[k]), (kw, mode, k)
            eng.close()
    ref.close()


def test_branching_from_a_history_run(ens):
    """History engine (one scenario) to T_BRANCH, then an S-scenario engine over the whole timeline started from its state at
    the branch: the same bits as an S-scenario engine run from step 0 over scenarios that share the history."""
    p, N = ens
    E, _ = _scenarios(N_STEPS, 4)
    full = EnsembleEngine(p, N, E, device="cuda:0")
    full.run(mode="per_step")
    hist = EnsembleEngine(p, N, E[0], device="cuda:0", store_trajectory=False)
    hist.run(0, T_BRANCH, mode="fused")
    torch.cuda.synchronize()
    br = EnsembleEngine(p, N, E, R0=hist.R, S0=hist.S, device="cuda:0")
    br.run(T_BRANCH, N_STEPS, mode="auto")
    for k in ("R", "S"):
        assert torch.equal(_sync_cpu(getattr(br, k)), _sync_cpu(getattr(full, k))), k
    assert torch.equal(_sync_cpu(br.T)[:, T_BRANCH:], _sync_cpu(full.T)[:, T_BRANCH:])
    assert torch.equal(_sync_cpu(br.C)[:, T_BRANCH:], _sync_cpu(full.C)[:, T_BRANCH:])
    for e in (full, hist, br):
        e.close()


@pytest.mark.parametrize("mode", ["per_step", "fused"])
def test_per_scenario_statistics_and_summaries(ens, mode):
    p, N = ens
    E, F = _scenarios(N_STEPS, 3)
    eng = EnsembleEngine(p, N, E, F_ext=F, collect_stats=True, device="cuda:0")
    eng.run(mode=mode)
    steps = [10, T_BRANCH, N_STEPS - 1]
    keep = torch.from_numpy(np.random.default_rng(5).random(N) < 0.4).to("cuda:0")
    T = _sync_cpu(eng.T).numpy()
    for s in range(3):
        one = EnsembleEngine(p, N, E[s], F_ext=F[s], collect_stats=True, device="cuda:0")
        one.run(mode=mode)
        assert torch.equal(eng.stats_sums(scenario=s).cpu(), one.stats_sums().cpu()), s
        for k, v in one.stats().items():
            assert torch.equal(torch.as_tensor(eng.stats(scenario=s)[k]).cpu(), torch.as_tensor(v).cpu()), (s, k)
        one.close()
        sm = eng.gather_summary(steps, percentiles=(5.0, 50.0, 95.0), scenario=s)
        assert np.array_equal(sm["percentiles"].numpy(), np.percentile(T[s][steps], (5.0, 50.0, 95.0), axis=1).T)
        sm = eng.gather_summary(steps, percentiles=(5.0, 50.0, 95.0), scenario=s, accepted=keep)
        sel = T[s][steps][:, keep.cpu().numpy()]
        assert np.array_equal(sm["percentiles"].numpy(), np.percentile(sel, (5.0, 50.0, 95.0), axis=1).T)
        assert int(sm["count"][0]) == int(keep.sum())
        h = eng.T_histogram(-1.0, 5.0, 64, rows=steps, scenario=s).cpu()
        assert int(h.sum()) == 3 * N
    with pytest.raises(ValueError, match="scenario"):
        eng.stats()
    with pytest.raises(ValueError, match="scenario"):
        eng.gather_summary(steps)
    with pytest.raises(ValueError, match="scenario"):
        eng.T_histogram(-1.0, 5.0, 64, scenario=3)
    eng.close()


def test_checkpoint_resume_and_refusals(ens):
    p, N = ens
    E, F = _scenarios(N_STEPS, 3)
    ref = EnsembleEngine(p, N, E, F_ext=F, collect_stats=True, device="cuda:0")
    ref.run(0, 170, mode="per_step")                # the schedule of the interrupted run, uninterrupted (the wave records
    ref.run(170, N_STEPS, mode="fused")             # of the two forms may sum in another order)
    a = EnsembleEngine(p, N, E, F_ext=F, collect_stats=True, device="cuda:0")
    a.run(0, 170, mode="per_step")
    state = a.state_dict()
    assert state["n_scenarios"] == 3 and len(state["drive_sha256"]) == 64
    b = EnsembleEngine(p, N, E, F_ext=F, collect_stats=True, device="cuda:0")
    b.load_state_dict(state)
    b.run(state["t_next"], N_STEPS, mode="fused")
    for k in ("R", "S"):
        assert torch.equal(_sync_cpu(getattr(b, k)), _sync_cpu(getattr(ref, k))), k
    assert torch.equal(_sync_cpu(b.T)[:, 170:], _sync_cpu(ref.T)[:, 170:])
    for s in range(3):
        got, want = b.stats_sums(scenario=s).cpu(), ref.stats_sums(scenario=s).cpu()
        assert torch.equal(got[170:], want[170:])                  # records of the resumed run
        assert torch.equal(got[:170], torch.from_numpy(state["_step_sums"][s, :170]))    # folded by the saver
    other = EnsembleEngine(p, N, E * 1.01, F_ext=F, collect_stats=True, device="cuda:0")
    with pytest.raises(ValueError, match="scenario set"):
        other.load_state_dict(state)
    two = EnsembleEngine(p, N, E[:2], F_ext=F[:2], collect_stats=True, device="cuda:0")
    with pytest.raises(ValueError, match="scenario set"):
        two.load_state_dict(state)
    single = EnsembleEngine(p, N, E[0], F_ext=F[0], collect_stats=True, device="cuda:0")
    s_state = single.state_dict()
    assert "n_scenarios" not in s_state and "drive_sha256" not in s_state       # single-scenario checkpoints gain no keys
    with pytest.raises(ValueError, match="scenario set"):
        a.load_state_dict(s_state)
    with pytest.raises(ValueError, match="scenario set"):
        single.load_state_dict(state)
    for e in (ref, a, b, other, two, single):
        e.close()


def test_the_refusals(ens):
    p, N = ens
    E, F = _scenarios(60, 2, t_branch=20)
    from fiveeqscm_amd.constrain import Observations
    tab = np.zeros((60, 4))
    tab[:10, 2] = 0.1                                              # a baseline period, no observation
    for kw in ({"concentration_driven": True}, {"hist": (-1.0, 5.0, 64)}, {"compensated": True, "dtype": torch.float32},
               {"observations": Observations(tab)}):
        with pytest.raises(ValueError, match="scenarios"):
            EnsembleEngine(p, N, E, device="cuda:0", **kw)
    eng = EnsembleEngine(p, N, E, device="cuda:0", small_lanes=1)
    with pytest.raises(ValueError, match="small"):
        eng.run(mode="small")
    assert eng.small_form() == 0 and eng.resolve_mode("auto")[0] != "small"
    with pytest.raises(ValueError, match="R0"):
        EnsembleEngine(p, N, E, R0=np.zeros((3, 7, N)), device="cuda:0")
    with pytest.raises(ValueError, match="scenario_names"):
        EnsembleEngine(p, N, E, scenario_names=["a"], device="cuda:0")
    with pytest.raises(ValueError, match="scenario_names"):
        EnsembleEngine(p, N, E[0], scenario_names=["a"], device="cuda:0")
    with pytest.raises(ValueError, match="at most"):
        EnsembleEngine(p, N, np.repeat(E[:1], 65, axis=0), device="cuda:0")
    assert EnsembleEngine(p, N, E[0], device="cuda:0").n_scenarios == 1
    eng.close()


def test_bytes_per_member_scenario_step(ens):
    p, N = ens
    E, _ = _scenarios(60, 4, t_branch=20)
    eng = EnsembleEngine(p, N, E, store_trajectory=False, device="cuda:0")
    one = EnsembleEngine(p, N, E[0], store_trajectory=False, device="cuda:0")
    w, SP, G = 8, 6, 3
    assert eng.bytes_per_member_step("per_step") == w * (2 * SP + 4) + w * (3 * G + 2) / 4
    assert one.bytes_per_member_step("per_step") == w * (2 * SP + 4 * G + 7 - (G + 1))
    assert 0.68 < eng.bytes_per_member_step("per_step") / one.bytes_per_member_step("per_step") < 0.70
    eng.close()
    one.close()


def test_full_size_one_million_members_four_scenarios_against_the_oracle():
    """1M parameter members x 4 scenarios, three gases, fp64, per-step (the bandwidth-bound form), on a fixed sample of
    members against the C oracle."""
    from oracle import c_oracle
    N, n_steps = 1_000_000, 200
    base = prm.default_params("multigas")
    p = prm.sample_ensemble(base, N)
    E, F = _scenarios(n_steps, 4, t_branch=100)
    out = [50, 120, n_steps - 1]
    eng = EnsembleEngine(p, N, E, F_ext=F, output_steps=out, store_concentrations=False, device="cuda:0")
    eng.run(mode="per_step")
    T = _sync_cpu(eng.T).numpy()
    R = _sync_cpu(eng.R).numpy()
    pick = np.unique(np.r_[0, 1, N - 1, np.random.default_rng(11).integers(0, N, 253)])
    sub = {k: (np.asarray(v)[:, pick] if np.ndim(v) == 2 and np.shape(v)[1] == N else v) for k, v in p.items()}
    for s in range(4):
        want = c_oracle.run(E[s], sub, pick.size, F_ext=F[s])
        err = np.abs(T[s][:, pick] - want["T"][out]) / (1e-10 * np.abs(want["T"][out]) + 1e-13)
        assert np.isfinite(T[s]).all() and err.max() <= 1.0, (s, float(err.max()))
        errR = np.abs(R[s][:, pick] - want["R"]) / (1e-10 * np.abs(want["R"]) + 1e-13)
        assert errR.max() <= 1.0, (s, float(errR.max()))
    eng.close()
