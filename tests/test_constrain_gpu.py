"""Constrained runs on the MI355X: the in-loop misfit accumulators against the C oracle, the same bits in every form, no change
to the model's own outputs, checkpoint / resume, the refusals, the constrained summary and a science check on the fixture."""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

from fiveeqscm_amd import _capi, constrain, emissions, scenario
from fiveeqscm_amd import params as prm
from fiveeqscm_amd.constrain import Observations
from fiveeqscm_amd.engine import EnsembleEngine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STEPS = 750
RUN_YEARS = 1750.0 + np.arange(N_STEPS)


@pytest.fixture(scope="module")
def obs():
    y, T, s = scenario.read_observations_csv(os.path.join(ROOT, "tests", "golden", "obs_synthetic.csv"))
    return Observations.from_years(RUN_YEARS, y, T, s, baseline=(1900, 1950))


@pytest.fixture(scope="module")
def ens():
    N = 3000
    return prm.sample_ensemble(prm.default_params("multigas"), N), emissions.rcp_like_emissions(N_STEPS, 3), N


def _misfit(eng):
    torch.cuda.synchronize()
    return eng.misfit.cpu()


def test_fp64_accumulators_against_the_c_oracle(obs, ens):
    from oracle import c_oracle
    p, E, N = ens
    eng = EnsembleEngine(p, N, E, observations=obs, store_trajectory=False, device="cuda:0")
    eng.run(mode="fused")
    got = _misfit(eng).numpy()
    T = c_oracle.run(E, p, N, keep=("T",))["T"]
    want = constrain.misfit_numpy(T, obs.table)
    tab = obs.table
    d = T - tab[:, 0:1]
    scale = np.stack([(tab[:, 2:3] * np.abs(T)).sum(0), (tab[:, 1:2] * np.abs(d)).sum(0), (tab[:, 1:2] * d * d).sum(0)])
    err = np.abs(got - want) / (1e-10 * scale)
    assert np.isfinite(got).all() and err.max() <= 1.0, float(err.max())
    assert torch.allclose(eng.chi2().cpu(), torch.from_numpy(constrain.chi2_from_misfit(want, obs.P)), rtol=1e-9, atol=1e-9)
    eng.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_misfit_rows_are_the_same_bits_in_every_form(obs, ens, dtype):
    p, E, N = ens
    lib = _capi.load()

    def rows(mode="per_step", packing=1, split=None, **kw):
        prev = lib.fiveeq_set_f32_packing(packing)
        try:
            eng = EnsembleEngine(p, N, E, observations=obs, dtype=dtype, store_trajectory=False, device="cuda:0", **kw)
            if split:
                eng.run(0, split[0], mode=split[1])
                eng.run(split[0], N_STEPS, mode=split[2])
            else:
                eng.run(mode=mode, **({"k_steps": 8} if mode == "ksteps" else {}))
            out = _misfit(eng)
            eng.close()
            return out
        finally:
            lib.fiveeq_set_f32_packing(prev)

    ref = rows(per_step_streams=1)
    assert ref.abs().sum() > 0
    runs = {
        "per_step/2": rows(per_step_streams=2),
        "graph": rows("graph"),
        "fused/None": rows("fused", fused_span=None),
        "fused/auto": rows("fused", fused_span="auto"),
        "fused/7": rows("fused", fused_span=7),
        "ksteps/8": rows("ksteps"),
        "chunk-major": rows(chunk_members=1024, per_step_streams=1),
        "split": rows(split=(100, "per_step", "per_step")),
        "split/mixed": rows(split=(100, "per_step", "fused")),
    }
    if dtype == torch.float32:
        runs["unpacked/per_step"] = rows(packing=0)
        runs["unpacked/fused"] = rows("fused", packing=0)
    for name, got in runs.items():
        assert torch.equal(got, ref), name


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_observations_change_no_bit_of_the_model(obs, ens, dtype):
    p, E, N = ens
    for mode in ("per_step", "fused", "ksteps"):
        outs = []
        for o in (None, obs):
            eng = EnsembleEngine(p, N, E, observations=o, dtype=dtype, device="cuda:0")
            eng.run(mode=mode, **({"k_steps": 8} if mode == "ksteps" else {}))
            torch.cuda.synchronize()
            outs.append([getattr(eng, k).cpu() for k in ("C", "T", "R", "S")])
            eng.close()
        assert all(torch.equal(a, b) for a, b in zip(*outs)), mode


def test_fp32_chi2_against_the_fp64_oracle(obs, ens):
    """fp32 T carries at most ~1.7e-5 relative error over the run (fiveeq_member.hpp, the compensated form's note: the default
    fp32 form's worst T error against 50-digit arithmetic); take 4x that of max |T| as the per-step bound dT.  A residual
    r_t = T_t - mean_ref T - o_t then errs by at most 2 dT, so |d chi2| <= sum_t p_t (2 |r_t| 2 dT + (2 dT)^2)."""
    from oracle import c_oracle
    p, E, N = ens
    eng = EnsembleEngine(p, N, E, observations=obs, dtype=torch.float32, store_trajectory=False, device="cuda:0")
    eng.run(mode="fused")
    got = eng.chi2().cpu().numpy()
    T = c_oracle.run(E, p, N, keep=("T",))["T"]
    want = constrain.chi2_from_misfit(constrain.misfit_numpy(T, obs.table), obs.P)
    tab = obs.table
    r = T - (tab[:, 2:3] * T).sum(0)[None, :] - tab[:, 0:1]
    dT = 4 * 1.7e-5 * np.abs(T).max(0)
    bound = (tab[:, 1:2] * (4 * np.abs(r) * dT + 4 * dT * dT)).sum(0)
    assert np.all(np.abs(got - want) <= bound), float(np.max(np.abs(got - want) / bound))
    eng.close()


@pytest.mark.parametrize("mode", ["per_step", "fused"])
def test_checkpoint_inside_the_window_resumes_bit_identically(obs, ens, mode):
    p, E, N = ens
    full = EnsembleEngine(p, N, E, observations=obs, device="cuda:0")
    full.run(mode=mode)
    torch.cuda.synchronize()
    a = EnsembleEngine(p, N, E, observations=obs, device="cuda:0")
    a.run(0, 200, mode=mode)                                     # the window is steps 150..319
    with pytest.raises(RuntimeError, match="window"):
        a.chi2()
    state = a.state_dict(include_outputs=False)
    assert state["obs_sha256"] == obs.sha256 and state["misfit"].shape == (3, N)
    b = EnsembleEngine(p, N, E, observations=obs, device="cuda:0")
    b.load_state_dict(state)
    b.run(state["t_next"], mode=mode)
    torch.cuda.synchronize()
    assert torch.equal(b.misfit, full.misfit) and torch.equal(b.T[200:], full.T[200:]) and torch.equal(b.chi2(), full.chi2())
    other = Observations(obs.table * np.r_[1.0, 1.0, 1.0, 0.0] + np.r_[0.01, 0.0, 0.0, 0.0])
    c = EnsembleEngine(p, N, E, observations=other, device="cuda:0")
    before = c.misfit.clone()
    with pytest.raises(ValueError, match="observation table"):
        c.load_state_dict(state)
    assert torch.equal(c.misfit, before) and c.t_next == 0
    plain = EnsembleEngine(p, N, E, device="cuda:0")
    with pytest.raises(ValueError, match="observation table"):
        plain.load_state_dict(state)
    for e in (full, a, b, c, plain):
        e.close()


def test_refusals_and_auto(obs, ens):
    p, E, N = ens
    eng = EnsembleEngine(p, N, E, observations=obs, device="cuda:0")
    with pytest.raises(ValueError, match="small"):
        eng.run(mode="small")
    assert eng.small_form() == 0
    eng.close()
    for kw in (dict(compensated=True, dtype=torch.float32), dict(hist=(-1.0, 3.0, 64))):
        with pytest.raises(ValueError, match="observations"):
            EnsembleEngine(p, N, E, observations=obs, device="cuda:0", **kw)
    with pytest.raises(ValueError, match="observations"):
        EnsembleEngine(p, N, np.full((N_STEPS, 3), 1.0) * [300.0, 800.0, 300.0], observations=obs, device="cuda:0",
                       concentration_driven=True)
    # a 10k CO2-only ensemble: launch-bound, where 'auto' would take the small-ensemble kernel without observations
    pc = prm.sample_ensemble(prm.default_params("co2"), 10_000)
    Ec = emissions.rcp_like_emissions(N_STEPS, 1)
    plain = EnsembleEngine(pc, 10_000, Ec, store_trajectory=False, device="cuda:0")
    assert plain.resolve_mode("auto")[0] == "small"
    plain.close()
    e1 = EnsembleEngine(pc, 10_000, Ec, observations=obs, store_trajectory=False, device="cuda:0")
    e1.run(mode="auto")
    assert e1.last_mode in ("ksteps", "fused")
    e2 = EnsembleEngine(pc, 10_000, Ec, observations=obs, store_trajectory=False, device="cuda:0")
    e2.run(mode="per_step")
    torch.cuda.synchronize()
    assert torch.equal(e1.misfit, e2.misfit) and torch.equal(e1.S, e2.S)
    assert e2.bytes_per_member_step("per_step") == pytest.approx(
        EnsembleEngine(pc, 10_000, Ec, store_trajectory=False, device="cuda:0").bytes_per_member_step("per_step") + 48 * 170 / 750)
    e1.close()
    e2.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_constrained_summary_is_np_percentile_of_the_accepted(obs, ens, dtype):
    p, E, N = ens
    steps = [749, 300]
    eng = EnsembleEngine(p, N, E, observations=obs, dtype=dtype, output_steps=steps, store_concentrations=False,
                         collect_stats=True, device="cuda:0")
    eng.run(mode="fused")
    chi2 = eng.chi2()
    keep = constrain.accept_threshold(chi2, float(chi2.median()))
    s = eng.gather_summary(steps, percentiles=(5.0, 50.0, 95.0), accepted=keep)
    T = eng.T.cpu().numpy()[[1, 0]]                      # rows are in step order: 300, 749
    sel = T[:, keep.cpu().numpy()].astype(np.float64)
    assert s["count"].tolist() == [float(keep.sum())] * 2
    assert np.array_equal(s["percentiles"].numpy(), np.percentile(sel, (5.0, 50.0, 95.0), axis=1).T)
    eng.close()


def test_science_on_the_fixture(obs):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_obs_synthetic as gen
    E = emissions.rcp_like_emissions(N_STEPS, 3)
    # the generating member scores like a draw of chi2 with n_obs degrees of freedom
    eng = EnsembleEngine(prm.default_params("multigas"), 1, E, observations=obs, store_trajectory=False, device="cuda:0")
    eng.run(mode="fused")
    chi2_true = float(eng.chi2()[0])
    eng.close()
    n = obs.n_obs
    assert abs(chi2_true - n) <= 5 * np.sqrt(2 * n), chi2_true
    assert gen.OBS_STEPS == n
    # the constrained 5-95 % range of final-step T is narrower than the unconstrained one
    N = 4000
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    eng = EnsembleEngine(p, N, E, observations=obs, output_steps=[N_STEPS - 1], store_concentrations=False, device="cuda:0")
    eng.run(mode="auto")
    keep = constrain.accept_rejection(eng.chi2(), constrain.ACCEPT_SEED, 0, N)
    assert 0 < int(keep.sum()) < N
    full = eng.gather_summary([N_STEPS - 1], percentiles=(5.0, 95.0))["percentiles"][0]
    con = eng.gather_summary([N_STEPS - 1], percentiles=(5.0, 95.0), accepted=keep)["percentiles"][0]
    assert float(con[1] - con[0]) < float(full[1] - full[0])
    eng.close()


@pytest.mark.parametrize("N", [10_000, 3001])
def test_co2_only_fp32_fused_forms_step_every_member(obs, N):
    """pools {4} in fp32 have no packed misfit form: the fused and K-step launches take the one-member-per-lane kernel on a
    grid sized for it — every member is stepped, and rows, state and misfit are the per-step path's bits (an even N is the
    case where the plain run packs two members per lane)."""
    p = prm.sample_ensemble(prm.default_params("co2"), N)
    E = emissions.rcp_like_emissions(N_STEPS, 1)

    def run(mode, **kw):
        eng = EnsembleEngine(p, N, E, dtype=torch.float32, observations=obs, output_steps=[100, 749], device="cuda:0", **kw)
        eng.run(mode=mode, **({"k_steps": 64} if mode == "ksteps" else {}))
        torch.cuda.synchronize()
        out = [t.cpu() for t in (eng.misfit, eng.R, eng.S, eng.C, eng.T)]
        eng.close()
        return out

    ref = run("per_step", per_step_streams=1)
    assert bool((ref[2][0] != 0).all()) and bool((ref[0][2] != 0).all())        # every member stepped and scored
    for mode, kw in (("fused", dict(fused_span=None)), ("fused", dict(fused_span="auto")), ("ksteps", {}), ("auto", {})):
        got = run(mode, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got, ref)), (mode, kw)


def test_rejection_on_an_empty_device_shard():
    chi2 = torch.empty(0, dtype=torch.float64, device="cuda:0")
    keep = constrain.accept_rejection(chi2, 5, 10, 10)
    assert keep.shape == (0,) and keep.dtype == torch.bool and keep.is_cuda


def _rccl_worker(port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist

    from fiveeqscm_amd import distributed as D
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)       # "nccl" is RCCL on ROCm
    calls = []
    real = dist.all_reduce

    def spy(*a, **k):
        calls.append(a[0].is_cuda)
        return real(*a, **k)

    try:
        n_total = 4001
        chi2 = (torch.arange(n_total, dtype=torch.float64, device=dev) % 97) * 0.37 + 150.0
        want = constrain.accept_rejection(chi2.cpu().numpy(), 11, 0, n_total)        # no collective: no process group used
        D.force_collectives(True)
        dist.all_reduce = spy
        got = constrain.accept_rejection(chi2, 11, 0, n_total)
        got_host = constrain.accept_rejection(chi2.cpu(), 11, 0, n_total)            # host scores over RCCL too
        empty = constrain.accept_rejection(chi2[:0], 11, 0, n_total)
        torch.cuda.synchronize()
        q.put({"device": np.array_equal(got.cpu().numpy(), want), "host": np.array_equal(got_host.numpy(), want),
               "empty": empty.numel() == 0 and empty.is_cuda, "calls": len(calls) == 3 and all(calls)})
    finally:
        dist.all_reduce = real
        dist.destroy_process_group()


def test_rejection_over_rccl_on_one_gpu():
    """accept_rejection's all-reduce MIN over the production backend (RCCL, one rank with force_collectives): the value
    travels as a device tensor, and the mask is the one-process mask."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(port, q))
    p.start()
    try:
        res = q.get(timeout=300)
    finally:
        p.join(timeout=120)
    assert p.exitcode == 0
    assert all(res.values()), res
