"""Constraining ensembles against an observed record, without a GPU: the observation table, the chi2 identity, the CSV
layout and its fixture, the host-side guards of the new C entry points, the acceptance rules at several world sizes, and the
constrained summary over gloo (NumPy restatement of the passes, as in tests/test_distributed.py)."""
import ctypes
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

from fiveeqscm_amd import _capi, constrain, scenario
from fiveeqscm_amd import params as prm
from fiveeqscm_amd.constrain import Observations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "obs_synthetic.csv")
RUN_YEARS = 1750.0 + np.arange(750)


def test_table_matches_years_and_weights():
    years = np.arange(2000.0, 2010.0)
    obs = Observations.from_years(years, [2003.0, 2001.0, 2008.0], [0.3, 0.1, 0.8], [0.1, 0.2, 0.5], baseline=(2000, 2002))
    t = obs.table
    assert t.shape == (10, 4) and not t[:, 3].any()
    assert t[1, 0] == 0.1 and t[3, 0] == 0.3 and t[8, 0] == 0.8
    assert t[1, 1] == 1.0 / (0.2 * 0.2) and t[3, 1] == 1.0 / (0.1 * 0.1) and t[8, 1] == 1.0 / (0.5 * 0.5)
    assert np.count_nonzero(t[:, 1]) == 3 and obs.n_obs == 3
    assert np.array_equal(t[:, 2], np.r_[np.full(3, 1.0 / 3.0), np.zeros(7)])
    assert obs.P == t[:, 1].sum() and obs.window == (0, 9)
    assert Observations.from_years(years, [2003.0], [0.3], 0.1, baseline=(2000, 2002)).sha256 != obs.sha256
    assert len(obs.sha256) == 64


@pytest.mark.parametrize("bad", [
    dict(T_obs=[np.nan]), dict(T_obs=[np.inf]), dict(sigma=[0.0]), dict(sigma=[-0.1]), dict(sigma=[np.nan]),
    dict(obs_years=[1999.0]), dict(obs_years=[2010.0]), dict(obs_years=[2003.5]), dict(baseline=(2050, 2060)),
    dict(baseline=(2003.2, 2003.8)), dict(obs_years=[2003.0, 2003.0], T_obs=[0.1, 0.2], sigma=[0.1, 0.1]),
])
def test_table_rejects_bad_input(bad):
    kw = dict(run_years=np.arange(2000.0, 2010.0), obs_years=[2003.0], T_obs=[0.3], sigma=[0.1], baseline=(2000, 2002))
    kw.update(bad)
    with pytest.raises(ValueError):
        Observations.from_years(**kw)


def test_chi2_identity_against_the_direct_sum():
    """chi2 = V - 2 A U + A^2 P from the accumulators (section 1 arithmetic) equals sum_t p_t (T_t - mean_ref T - o_t)^2."""
    rng = np.random.default_rng(7)
    for trial in range(20):
        n_steps, N = int(rng.integers(20, 300)), 257
        years = np.arange(n_steps, dtype=np.float64)
        k = int(rng.integers(5, n_steps))
        oy = np.sort(rng.choice(years, size=k, replace=False))
        y0 = float(rng.integers(0, n_steps // 2))
        obs = Observations.from_years(years, oy, rng.normal(0.5, 0.4, k), rng.uniform(0.05, 0.3, k),
                                      baseline=(y0, y0 + int(rng.integers(0, 40))))
        T = np.cumsum(rng.normal(0.01, 0.05, (n_steps, N)), axis=0) + rng.normal(0, 2.0)
        if trial % 2:
            T = T.astype(np.float32)
        mf = constrain.misfit_numpy(T, obs.table)
        chi2 = constrain.chi2_from_misfit(mf, obs.P)
        Tw = T.astype(np.float64)
        tab = obs.table
        ref = (Tw * tab[:, 2:3]).sum(0)
        direct = (tab[:, 1:2] * (Tw - ref[None, :] - tab[:, 0:1]) ** 2).sum(0)
        A, U, V = mf
        bound = 1e-12 * (V + 2 * np.abs(A * U) + A * A * obs.P)
        assert np.all(np.abs(chi2 - direct) <= bound), float(np.max(np.abs(chi2 - direct) / bound))


def test_misfit_numpy_skips_steps_outside_the_window():
    tab = np.zeros((4, 4))
    tab[1] = (0.5, 4.0, 1.0, 0.0)
    T = np.array([[np.nan], [1.0], [np.inf], [2.0]])                 # outside the window: never read
    mf = constrain.misfit_numpy(T, tab)
    assert mf[:, 0].tolist() == [1.0, 4.0 * 0.5, 4.0 * 0.5 * 0.5]
    split = constrain.misfit_numpy(T[2:], tab[2:], acc=constrain.misfit_numpy(T[:2], tab[:2]))
    assert np.array_equal(split, mf)


def test_observation_csv_round_trip_and_fixture(tmp_path):
    p = tmp_path / "obs.csv"
    y, T, s = np.arange(1900.0, 1910.0), np.random.default_rng(1).normal(size=10), np.full(10, 0.1)
    scenario.write_observations_csv(p, y, T, s, comment="a test record")
    y2, T2, s2 = scenario.read_observations_csv(p)
    assert np.array_equal(y, y2) and np.array_equal(T, T2) and np.array_equal(s, s2)
    bad = tmp_path / "bad.csv"
    bad.write_text("YEAR,TEMP,SIGMA\n1900,0.1,0.1\n")
    with pytest.raises(ValueError):
        scenario.read_observations_csv(bad)
    bad.write_text("YEAR,T,SIGMA\n1900,x,0.1\n")
    with pytest.raises(ValueError):
        scenario.read_observations_csv(bad)
    # the committed fixture: 170 yearly values 1900..2069 with sigma 0.1 K, baseline 1900..1950 (51 steps)
    y, T, s = scenario.read_observations_csv(FIXTURE)
    assert y.tolist() == list(np.arange(1900.0, 2070.0)) and np.all(s == 0.1) and np.isfinite(T).all()
    obs = Observations.from_years(RUN_YEARS, y, T, s, baseline=(1900, 1950))
    assert obs.n_obs == 170 and obs.window == (150, 320) and np.count_nonzero(obs.table[:, 2]) == 51
    assert abs(obs.P - 170 / 0.01) < 1e-9 and abs(T[:51].mean()) < 0.05 and T[-10:].mean() > 0.5


def test_obs_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _capi.load()
    m = prm.make_model(prm.default_params("multigas"))
    p = ctypes.c_void_p(0x1000)
    run = lambda *tail, fn=lib.fiveeq_run_obs_f64, t=(0, 4), n_steps=4, mm=m: fn(       # noqa: E731
        ctypes.byref(mm), 8, 8, p, n_steps, t[0], t[1], p, p, p, p, None, None, 0, None, *tail)
    assert run(None, p, _capi.FORM_FUSED, 0, None) == _capi.E_INVALID and b"NULL" in lib.fiveeq_last_error()
    assert run(p, None, _capi.FORM_PER_STEP, 0, None) == _capi.E_INVALID
    assert run(p, None, _capi.FORM_PER_STEP, 0, None, fn=lib.fiveeq_run_obs_f32) == _capi.E_INVALID
    assert run(ctypes.c_void_p(0x1004), p, _capi.FORM_FUSED, 0, None) == _capi.E_INVALID          # unaligned
    assert run(p, p, 7, 0, None) == _capi.E_INVALID and b"form" in lib.fiveeq_last_error()
    assert run(p, p, _capi.FORM_FUSED, -1, None) == _capi.E_INVALID
    assert run(p, p, _capi.FORM_FUSED, 0, None, t=(0, 5)) == _capi.E_INVALID                      # range outside [0, n_steps)
    assert run(p, p, _capi.FORM_PER_STEP, 0, None, t=(-1, 2)) == _capi.E_INVALID
    assert run(p, p, _capi.FORM_FUSED, 0, None, t=(2, 2)) == _capi.OK                              # empty range: nothing launched
    # a layout with kernels but no misfit form: CH4 + N2O alone (pools 1 + 1)
    m2 = prm.make_model(prm.default_params("multigas"))
    m2.gas[0] = m2.gas[1]
    m2.gas[1] = m2.gas[2]
    m2.n_gas = 2
    assert run(p, p, _capi.FORM_FUSED, 0, None, mm=m2) == _capi.E_INVALID and b"misfit" in lib.fiveeq_last_error()
    plan = ctypes.c_void_p()
    base = (ctypes.byref(m), 8, 8, p, 4, 0, 4, p, p, p, p, None, None, 0, None)
    assert lib.fiveeq_plan_create_obs_f64(*base, p, None, ctypes.byref(plan)) == _capi.E_INVALID and not plan.value
    assert lib.fiveeq_plan_create_obs_f32(*base, None, p, ctypes.byref(plan)) == _capi.E_INVALID and not plan.value
    assert lib.fiveeq_plan_create_obs_f64(ctypes.byref(m2), *base[1:], p, p, ctypes.byref(plan)) == _capi.E_INVALID
    layout = lambda *pools: lib.fiveeq_misfit_layout_supported(len(pools), (ctypes.c_int32 * len(pools))(*pools))  # noqa: E731
    assert layout(4) == 1 and layout(4, 1, 1) == 1
    assert layout(1, 1) == 0 and layout(4, 4, 4) == 0 and layout(2) == 0 and layout(4, 2, 1) == 0


def _ragged(n_total, world):
    cuts = np.sort(np.random.default_rng(world).choice(np.arange(1, n_total), size=world - 1, replace=False))
    b = np.r_[0, cuts, n_total]
    return [(int(b[r]), int(b[r + 1])) for r in range(world)]


def _accept_worker(rank, world, port, n_total, bounds, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        chi2 = _scores(n_total)
        lo, hi = bounds[rank]
        rej = constrain.accept_rejection(chi2[lo:hi].copy(), 99, lo, n_total)
        rej_t = constrain.accept_rejection(torch.from_numpy(chi2[lo:hi].copy()), 99, lo, n_total)
        thr = constrain.accept_threshold(chi2[lo:hi], 150.0)
        q.put((rank, rej, rej_t.numpy(), thr))
    finally:
        dist.destroy_process_group()


def _scores(n_total):
    chi2 = 120.0 + np.random.default_rng(3).chisquare(20, n_total) * 2.0
    chi2[17] = np.nan                                               # a failed member is rejected by both rules
    return chi2


def _spawn(target, world, *args):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port) + args + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    out = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return [v for _, *v in sorted(out, key=lambda r: r[0])]


@pytest.mark.parametrize("world", [2, 3])
def test_acceptance_masks_do_not_depend_on_the_world(world):
    n_total = 2001
    chi2 = _scores(n_total)
    rej1 = constrain.accept_rejection(chi2, 99, 0, n_total)
    thr1 = constrain.accept_threshold(chi2, 150.0)
    assert 0 < rej1.sum() < n_total and 0 < thr1.sum() < n_total and not rej1[17] and not thr1[17]
    # the global minimum is always accepted; a one-rank torch call gives the NumPy mask
    assert rej1[np.nanargmin(chi2)]
    assert np.array_equal(constrain.accept_rejection(torch.from_numpy(chi2), 99, 0, n_total).numpy(), rej1)
    assert not np.array_equal(constrain.accept_rejection(chi2, 100, 0, n_total), rej1)        # the seed keys the uniforms
    parts = _spawn(_accept_worker, world, n_total, _ragged(n_total, world))
    for k, want in ((0, rej1), (1, rej1), (2, thr1)):
        assert np.array_equal(np.concatenate([p[k] for p in parts]), want)


def _summary_worker(rank, world, port, n_total, empty_rank, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1")
    import torch.distributed as dist

    from fiveeqscm_amd.distributed import gather_summary, shard_bounds
    from tests.test_distributed import _use_oracle_passes
    _use_oracle_passes()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        full, keep = _summary_data(n_total, world, empty_rank)
        lo, hi = shard_bounds(n_total, rank, world)
        rows = torch.from_numpy(full[:, lo:hi].copy())
        mask = torch.from_numpy(keep[lo:hi].copy())
        s = gather_summary(rows[:, mask].contiguous(), percentiles=(5.0, 50.0, 95.0))
        q.put((rank, s["count"].numpy(), None if s["percentiles"] is None else s["percentiles"].numpy(), s["mean"].numpy()))
    finally:
        dist.destroy_process_group()


def _summary_data(n_total, world, empty_rank):
    from fiveeqscm_amd.distributed import shard_bounds
    rng = np.random.default_rng(11)
    full = rng.normal(1.5, 0.7, size=(3, n_total))
    keep = constrain.accept_threshold(rng.chisquare(10, n_total), 12.0)
    if empty_rank is not None:
        lo, hi = shard_bounds(n_total, empty_rank, world)
        keep[lo:hi] = False
    return full, keep


@pytest.mark.parametrize("empty_rank", [None, 0, 1])
def test_constrained_summary_over_gloo_world2(empty_rank):
    """The summary of the accepted members over two ranks: np.percentile of the accepted subset bit for bit — also when
    one rank (the root or the other) holds no accepted member at all."""
    n_total = 3001
    full, keep = _summary_data(n_total, 2, empty_rank)
    parts = _spawn(_summary_worker, 2, n_total, empty_rank)
    want = np.percentile(full[:, keep], (5.0, 50.0, 95.0), axis=1).T
    assert all(p[0].tolist() == [float(keep.sum())] * 3 for p in parts)
    assert np.array_equal(parts[0][1], want) and parts[1][1] is None
    assert np.allclose(parts[0][2], full[:, keep].mean(1), rtol=1e-13)


def test_exact_score_helper_and_its_bound_on_the_reference_arithmetic():
    """oracle/misfit_exact.py, the exact-arithmetic reference R3 of tests/test_misfit_gpu.py, without a GPU: its integer
    sums are plain Fraction arithmetic, and misfit_numpy + chi2_from_misfit (the fp64 arithmetic the kernels restate) stays
    inside its derived bound (chi2_bound; the derivation is in tests/test_misfit_gpu.py::test_r3_score) on C-oracle T —
    400 steps of 64 members of each misfit layout, on the observed fixture, a window from step 0, a one-step window, and a
    table that forces cancellation: T and o_t shifted by a common 10 K, so that V >> chi2."""
    from fractions import Fraction

    from fiveeqscm_amd import emissions
    from oracle import c_oracle
    from oracle import misfit_exact as mx
    n_steps, N = 400, 64
    years = 1750.0 + np.arange(n_steps)
    rng = np.random.default_rng(5)
    y, To, s = scenario.read_observations_csv(FIXTURE)
    for kind, G in (("co2", 1), ("multigas", 3)):
        p = prm.sample_ensemble(prm.default_params(kind), N)
        T = c_oracle.run(emissions.rcp_like_emissions(n_steps, G), p, N, keep=("T",))["T"]
        oy = np.arange(1750.0, 2150.0, 3.0)
        cases = {
            "fixture": (T, Observations.from_years(years, y, To, s, baseline=(1900, 1950))),
            "from_step_0": (T, Observations.from_years(years, oy, rng.normal(0.5, 0.5, oy.size), rng.uniform(0.05, 0.3, oy.size),
                                                       baseline=(1750, 1760))),
            "one_step": (T, Observations.from_years(years, [2000.0], [0.7], [0.1], baseline=(2000, 2000))),
        }
        Ts = T + 10.0                                              # a common 10 K offset on T ...
        steps = np.arange(150, 320)
        ref = Ts[150:201, 0].mean()
        o = Ts[steps, 0] - ref + 10.0 + rng.normal(0.0, 0.01, steps.size)      # ... and on o_t: d = T - o ~ mean_ref T
        cases["cancel"] = (Ts, Observations.from_years(years, years[steps], o - 10.0, 0.1, baseline=(1900, 1950)))
        for name, (TT, obs) in cases.items():
            mis = constrain.misfit_numpy(TT, obs.table)
            chi2 = constrain.chi2_from_misfit(mis, obs.P)
            if name == "cancel":
                assert np.all(mis[2] > 100 * chi2), float((mis[2] / chi2).min())          # V >> chi2
            for m in range(N):
                exact, bound = mx.chi2_bound(TT[:, m], obs.table, mis[:, m], obs.P)
                assert abs(Fraction(float(chi2[m])) - exact) <= bound, (kind, name, m)          # the derived bound
        # the integer sums are Fraction arithmetic
        tab = cases["fixture"][1].table
        live = np.nonzero(tab[:, 1] + tab[:, 2])[0]
        for m in (0, N - 1):
            F = [Fraction(float(v)) for v in T[live, m]]
            A = sum(Fraction(float(tab[t, 2])) * f for t, f in zip(live, F))
            want = sum(Fraction(float(tab[t, 1])) * (f - A - Fraction(float(tab[t, 0]))) ** 2 for t, f in zip(live, F))
            assert mx.chi2_exact(T[:, m], tab) == want
