"""Resampling a weighted ensemble on the MI355X (include/fiveeq.h, "RESAMPLING"): the scan, pick and gather kernels against
the Python-integer reference (tests/resample_reference.py) at every size where they take another path, and the workflow end
to end — an engine built from EnsembleEngine.resampled(plan) continues, bit for bit, the members the plan drew.  Every
comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from fiveeqscm_amd import _capi, emissions
from fiveeqscm_amd import params as prm
from fiveeqscm_amd.constrain import W_ONE, Observations, accept_threshold, importance_weights, resample
from fiveeqscm_amd.engine import EnsembleEngine
from fiveeqscm_amd.forcing import ScenarioForcings
from resample_reference import first_output, source_list, weight_patterns

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE = _capi.WSCAN_TILE


def _p(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def _scan(w):
    """fiveeq_wscan of an int64 device tensor -> (cum int64 [n], flags int)"""
    lib = _capi.load()
    n = w.numel()
    cum = torch.full((n + 1,), -1, dtype=torch.int64, device=w.device)       # one guard word behind the scan
    flags = torch.full((1,), -1, dtype=torch.int64, device=w.device)
    work = torch.empty(int(lib.fiveeq_wscan_chunks(n)), dtype=torch.int64, device=w.device)
    _capi.check(lib, lib.fiveeq_wscan(n, _p(w), _p(work), _p(cum), _p(flags), None))
    torch.cuda.synchronize()
    assert int(cum[n]) == -1
    return cum[:n], int(flags[0])


# ---- 1. the scan ------------------------------------------------------------------------------------------------------------
# ... and, since ONE workgroup scans the tile sums in rounds of 256 tiles with a carried total, 256 and 257 tiles (the second
# round) and a million members (four rounds)
SCAN_N = sorted({1, 63, 64, 65, 255, 256, 257, 1000, 4097, 1_000_003} | {TILE * K + d for K in (1, 2, 65, 256, 257) for d in (-1, 0, 1)})


@pytest.mark.parametrize("n", SCAN_N)
def test_scan_equals_the_integer_cumulative_sum(n):
    lib = _capi.load()
    assert lib.fiveeq_wscan_chunks(TILE) == 2 and lib.fiveeq_wscan_chunks(TILE + 1) == 4      # TILE is the weights per workgroup
    rng = np.random.default_rng(n)
    w = rng.integers(0, W_ONE + 1, size=n + 1).astype(np.int64)
    w[rng.integers(0, n + 1, size=n // 3)] = 0
    w[-1] = W_ONE
    buf = torch.from_numpy(w).to(DEV)
    for lead in (0, 1):                                     # 16-byte aligned weights, and weights 8 bytes off (the narrow loads)
        cum, flags = _scan(buf[lead:lead + n])
        assert flags == 0 and torch.equal(cum.cpu(), torch.from_numpy(np.cumsum(w[lead:lead + n])))
    bad = buf[:n].clone()
    bad[n // 2] = W_ONE + 1
    assert _scan(bad)[1] == 2
    bad[n // 2] = -1                                        # as a bit pattern: far above 2^32
    assert _scan(bad)[1] == 2


# ---- 2. the pick ------------------------------------------------------------------------------------------------------------
def _pick_shards(w, M, rho, bounds):
    """every shard's src from the kernels (scan, then pick with the shard's C_lo and output range computed here in Python
    integers), as global member indices"""
    lib = _capi.load()
    W = sum(w)
    q, s = divmod(W, M)
    a, b = divmod(rho, M)
    out = []
    for lo, hi in bounds:
        C_lo, C_hi = sum(w[:lo]), sum(w[:hi])
        j0, j1 = first_output(C_lo, W, M, rho), first_output(C_hi, W, M, rho)
        assert j0 == len(out)
        if j1 == j0:
            continue
        cum, flags = _scan(torch.tensor(w[lo:hi], dtype=torch.int64, device=DEV))
        assert flags == 0
        src = torch.full((j1 - j0 + 1,), -7, dtype=torch.int32, device=DEV)
        _capi.check(lib, lib.fiveeq_resample_pick(hi - lo, _p(cum), C_lo, M, q, a, s, b, j0, j1 - j0, _p(src), None))
        torch.cuda.synchronize()
        assert int(src[-1]) == -7
        out.extend(v + lo for v in src[:-1].cpu().tolist())
    return out


@pytest.mark.parametrize("n", [37, 3000])
@pytest.mark.parametrize("pattern", ["equal", "one_member", "random_half_zero", "all_2_32", "mask"])
def test_pick_equals_the_reference(n, pattern):
    rng = np.random.default_rng(n)
    w = weight_patterns(n, rng)[pattern]
    W = sum(w)
    thirds = [(0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n)]
    for M in (1, 2, 3, n, 3 * n + 1):
        for rho in (0, W - 1, int(rng.integers(0, W))):
            want = source_list(w, M, rho)
            assert _pick_shards(w, M, rho, [(0, n)]) == want, (M, rho)
            assert _pick_shards(w, M, rho, thirds) == want, (M, rho)      # sub-ranges (j0 > 0, c_lo > 0): a simulated 3-way split


def test_pick_with_no_output_launches_nothing():
    lib = _capi.load()
    assert lib.fiveeq_resample_pick(8, None, 0, 10, 3, 0, 1, 2, 4, 0, None, None) == _capi.OK


# ---- 3. the gather ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n_rows", [1, 3, 9])
def test_gather_copies_columns_and_leaves_the_padding_alone(dtype, n_rows):
    lib = _capi.load()
    fn = lib.fiveeq_gather_rows_f64 if dtype == torch.float64 else lib.fiveeq_gather_rows_f32
    n, ld_in, n_out, ld_out = 1000, 1013, 1500, 1531
    g = torch.Generator().manual_seed(n_rows)
    rows = torch.full((n_rows, ld_in), float("nan"), dtype=dtype)
    rows[:, :n] = torch.randn(n_rows, n, generator=g, dtype=torch.float64).to(dtype)
    runs = torch.sort(torch.cat([torch.full((700,), 17), torch.randint(0, n, (n_out - 1000,), generator=g), torch.full((300,), n - 1)]))[0]
    src = runs.to(torch.int32)
    out = torch.full((n_rows + 1, ld_out), float("nan"), dtype=dtype, device=DEV)
    rows_d, src_d = rows.to(DEV), src.to(DEV)
    _capi.check(lib, fn(n_rows, n_out, ld_in, _p(rows_d), ld_out, _p(out), _p(src_d), None))
    torch.cuda.synchronize()
    out = out.cpu()
    assert torch.equal(out[:n_rows, :n_out], rows[:, runs]) and bool(torch.isnan(out[:n_rows, n_out:]).all()) and bool(torch.isnan(out[n_rows]).all())
    _capi.check(lib, fn(n_rows, 0, ld_in, None, ld_out, None, None, None))                 # n_out = 0: a no-op
    plan = resample(torch.ones(n, dtype=torch.bool, device=DEV))
    assert plan.gather(torch.zeros((2, 3, n), dtype=dtype, device=DEV)).shape == (2, 3, n)
    empty = resample(torch.ones(n, dtype=torch.bool, device=DEV))
    empty.src, empty.n_members = empty.src[:0], 0                                          # a rank that owns no output
    assert empty.gather(torch.zeros((4, n), dtype=dtype, device=DEV)).shape == (4, 0)


def test_device_resample_equals_the_host_twins():
    rng = np.random.default_rng(77)
    for n in (1, 300, 5000):
        for name, w in weight_patterns(n, rng).items():
            w = np.array(w, dtype=np.int64)
            for M, seed in ((n, None), (3 * n + 1, 4), (max(1, n // 10), "s")):
                host, dev = resample(w, M, seed=seed), resample(torch.from_numpy(w).to(DEV), M, seed=seed)
                assert dev.src.dtype == torch.int32 and dev.src.is_cuda and np.array_equal(dev.src.cpu().numpy(), host.src), (name, n, M)
                assert (dev.weight_sum, dev.offset, dev.n_out, dev.j0) == (host.weight_sum, host.offset, M, 0)
    mask = torch.from_numpy(rng.integers(0, 2, size=4097).astype(bool))
    assert torch.equal(resample(mask.to(DEV)).src.cpu().long(), torch.nonzero(mask)[:, 0])
    for bad in (torch.tensor([1, -1, 2]), torch.tensor([1, W_ONE + 1])):
        with pytest.raises(ValueError, match=r"outside \[0, 2\^32\]"):
            resample(bad.to(DEV), 3)
    with pytest.raises(ValueError, match="sum to 0"):
        resample(torch.zeros(70, dtype=torch.int64, device=DEV), 3)


# ---- 4. end to end: layout 4 + 1 + 1, N = 1000, 60 steps, history to step 40 ----------------------------------------------
N, N_STEPS, CUT, S = 1000, 60, 40, 2


@functools.lru_cache(maxsize=None)
def _world(dtype, with_forcing):
    """The history engine (observations=, run to CUT), its weights, and the FULL projections of all N members from the branch
    step: one scenario, and the scenario axis with S = 2.  Built once per (dtype, forcing) and left unchanged."""
    base = prm.default_params("multigas")
    p = prm.sample_ensemble_shard(base, N)
    tt = np.arange(N_STEPS)
    E = np.repeat(emissions.rcp_like_emissions(N_STEPS, 3)[None], S, axis=0)
    E[1, CUT:, 0] *= 1.5
    F = np.stack([0.02 * tt / N_STEPS, 0.02 * tt / N_STEPS + np.where(tt >= CUT, 0.05 * np.sin(tt / 7.0), 0.0)])
    sf = None
    if with_forcing:
        sc = prm.sample_forcing_scales(base, N, ranges=[(0.8, 1.2)] * 3 + [(0.3, 2.0), (0.5, 1.5)], seed=7)
        p["f_scale"], p["fx_scale"] = sc[:3], sc[3:]
        sf = ScenarioForcings(np.stack([-1.1 * E[:, :, 0] / E[0, :, 0].max(), np.repeat(np.where(tt % 17 == 5, -2.5, 0.0)[None], S, 0)], axis=2),
                              ("aerosol", "volcanic"))
    years = 1750.0 + tt
    at = np.arange(10, CUT)
    obs = Observations.from_years(years, years[at], 0.004 * (at - 10), 0.05, baseline=(1755, 1765))     # synthetic record
    kw = dict(dtype=dtype, device=DEV)
    hist = EnsembleEngine(p, N, E[0], F_ext=F[0], forcing=sf.scenario(0) if sf else None, observations=obs, store_trajectory=False, **kw)
    hist.run(0, CUT, mode="per_step")
    torch.cuda.synchronize()
    chi2 = hist.chi2()
    one = EnsembleEngine(p, N, E[0], F_ext=F[0], forcing=sf.scenario(0) if sf else None, R0=hist.R, S0=hist.S, **kw)
    one.run(CUT, N_STEPS, mode="per_step")
    two = EnsembleEngine(p, N, E, F_ext=F, forcing=sf, R0=hist.R, S0=hist.S, **kw)
    two.run(CUT, N_STEPS, mode="per_step")
    torch.cuda.synchronize()
    return dict(p=p, E=E, F=F, sf=sf, hist=hist, chi2=chi2, w=importance_weights(chi2), one=one, two=two, kw=kw)


def _project(wd, plan, scen):
    """the engine of the resampled members, built from hist.resampled(plan) and run from the branch step"""
    params, R0, S0 = wd["hist"].resampled(plan)
    E, F, sf = wd["E"], wd["F"], wd["sf"]
    forcing = None if sf is None else (sf if scen else sf.scenario(0))
    eng = EnsembleEngine(params, plan.n_members, E if scen else E[0], F_ext=F if scen else F[0], forcing=forcing, R0=R0, S0=S0, **wd["kw"])
    eng.run(CUT, N_STEPS, mode="per_step")
    torch.cuda.synchronize()
    return eng


@pytest.mark.parametrize("M", [257, 1500])
@pytest.mark.parametrize("scen", [False, True], ids=["one_scenario", "scenario_axis"])
@pytest.mark.parametrize("with_forcing", [False, True], ids=["plain", "forcing"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_resampled_engine_continues_the_drawn_members(dtype, with_forcing, scen, M):
    wd = _world(dtype, with_forcing)
    plan = resample(wd["w"], M, seed=3)
    assert plan.n_members == plan.n_out == M and plan.n_source == N and plan.weight_sum == int(wd["w"].sum())
    src = plan.src.long()
    assert src.cpu().tolist() == source_list(wd["w"].cpu().tolist(), M, plan.offset)
    full = wd["two" if scen else "one"]
    eng = _project(wd, plan, scen)
    assert eng.dtype == dtype and eng.n_members == M
    assert torch.equal(eng.T[..., CUT:, :], full.T[..., CUT:, :].index_select(-1, src))
    assert torch.equal(eng.C[..., CUT:, :, :], full.C[..., CUT:, :, :].index_select(-1, src))
    assert torch.equal(eng.R, full.R.index_select(-1, src)) and torch.equal(eng.S, full.S.index_select(-1, src))
    assert float(eng.T[..., -1, :].abs().min()) > 0.0
    if scen:                                                # the state of a scenario engine keeps its scenario axis
        params, R0, S0 = full.resampled(plan)
        assert R0.shape == (S, full.sum_pools, M) and torch.equal(R0, full.R.index_select(-1, src)) and torch.equal(S0, full.S.index_select(-1, src))
        assert torch.equal(params["q"], full.q.index_select(-1, src)) and params["r0"].shape == (3, M)
    eng.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_mask_compaction_gives_the_accepted_summary(dtype):
    wd = _world(dtype, True)
    keep = accept_threshold(wd["chi2"], float(wd["chi2"].median()))
    plan = resample(keep)
    assert 0 < plan.n_members == int(keep.sum()) < N and torch.equal(plan.src.long(), torch.nonzero(keep)[:, 0])
    eng = _project(wd, plan, False)
    steps, pct = [CUT, 50, N_STEPS - 1], (5.0, 50.0, 95.0)
    got, want = eng.gather_summary(steps, pct), wd["one"].gather_summary(steps, pct, accepted=keep)
    for key in ("percentiles", "min", "max", "count"):
        assert torch.equal(got[key], want[key]), key
    eng.close()


def test_resampled_refusals():
    wd = _world(torch.float64, False)
    with pytest.raises(ValueError, match="plan over this engine"):
        wd["hist"].resampled(resample(wd["w"].cpu().numpy(), 10))              # host indices
    with pytest.raises(ValueError, match="plan over this engine"):
        wd["hist"].resampled(resample(wd["w"][:500], 10))                      # another member count
    inv = EnsembleEngine(prm.default_params("multigas"), 64, np.full((20, 3), 1.0) * [300.0, 800.0, 300.0], concentration_driven=True,
                         device=DEV)
    with pytest.raises(ValueError, match="concentration-driven"):
        inv.resampled(resample(torch.ones(64, dtype=torch.bool, device=DEV)))
    inv.close()
