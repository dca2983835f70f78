#!/usr/bin/env python3
"""Constrain a parameter ensemble on the historical record, then project the accepted members under several emission
scenarios at once, and write per-scenario 5/50/95 % of warming as CSV.

1. A single-scenario engine with observations= runs the history (to the end of the observation window of the committed
   synthetic record tests/golden/obs_synthetic.csv).
2. Members are accepted by rejection sampling on their chi2.
3. Branch: an engine with the scenario axis over the whole timeline starts from the history engine's state at the branch
   step and runs the rest.  Its drive tables cover every step from 0, so the cumulative-emission column is exact.
4. The summary over the accepted members of each scenario goes to one long-format CSV (SCENARIO, YEAR, ...).

The scenarios are synthetic: rcp_like_emissions with future CO2 scaled low / mid / high after the branch year.  Needs an
MI355X.

--forcing adds forcing uncertainty: every member scales the gas forcings and two external categories (an aerosol forcing
proportional to the CO2 emissions, volcanic spikes) by its own factors.  The history runs with forcing= + observations=, so the
misfit constrains the aerosol scale; the projection is a scenario engine with forcing=ScenarioForcings — one aerosol table per
scenario, following that scenario's emissions — and the SAME scale rows.

--weights keeps EVERY member instead: each is weighted by its likelihood (constrain.importance_weights, integer weights) and the
summaries are the exact weighted percentiles of gather_summary(weights=); the effective sample size is printed beside the number
rejection sampling would have accepted.

--resample M shrinks the ensemble before it is projected (include/fiveeq.h, "RESAMPLING"): after the history the members
are resampled into M equal-weight ones — by their importance weights with --weights, else from the accepted members (each
drawn floor or ceil of M / accepted times) — and only
those are branched into the scenarios (EnsembleEngine.resampled) and summarised, with the plain unweighted gather_summary.

--drivers prints, per scenario and for the last stored T row and the peak, the parameters ranked by the share of the spread
they explain (EnsembleEngine.drivers: eta2, the first-order sensitivity index, with the correlation) — once over all projected
members and once under the posterior the run uses (weights, accepted, or the resampled members, which are their own posterior).

--metrics LEVELS --smooth W judges the warming levels and the peak on the running mean over W stored rows
(EnsembleEngine.running_mean, dated at the window's centre) instead of on single rows — what a warming level means once
members carry internal variability.

--carbon prints, per scenario at the last stored step, the percentiles of the CO2 airborne fraction and of the CH4 lifetime
scaling alpha (EnsembleEngine.carbon_rows on one-row blocks of the stored rows; weighted where weights are in use).

--sea-level prints, per scenario, the percentiles of the global-mean sea-level rise since the branch year at the last step and
of the first year it reaches 0.5 m (EnsembleEngine.sea_level_rows into trajectory_metrics with a level in metres).  Sea-level
rise integrates every year, so a second projection stores consecutive steps.  Its four components' priors are ILLUSTRATIVE,
NOT A CALIBRATION.

    python example/scenario_projections.py [--members N] [--out FILE] [--forcing] [--weights] [--resample M] [--drivers]
                                           [--metrics LEVELS [--smooth W]] [--carbon] [--sea-level]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fiveeqscm_amd import constrain, emissions, params, scenario  # noqa: E402
from fiveeqscm_amd.engine import EnsembleEngine  # noqa: E402
from fiveeqscm_amd.forcing import ScenarioForcings  # noqa: E402

SCENARIOS = {"low": 0.3, "mid": 1.0, "high": 1.6}          # future CO2 emissions as a multiple of the baseline path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=100_000)
    ap.add_argument("--out", default="scenario_projections.csv")
    ap.add_argument("--forcing", action="store_true", help="per-member forcing scales, per-scenario aerosol tables")
    ap.add_argument("--weights", action="store_true", help="importance-weight every member instead of rejection sampling")
    ap.add_argument("--resample", type=int, default=0, metavar="M", help="project only M resampled equal-weight members")
    ap.add_argument("--metrics", default="", metavar="LEVELS", help="comma-separated warming levels (K): also print, per scenario, "
                    "peak warming, P(exceed level) and the crossing year, from one pass over the stored rows")
    ap.add_argument("--smooth", type=int, default=0, metavar="W", help="with --metrics: judge the levels and the peak on the running mean "
                    "over W stored rows (dated at the window's centre) instead of on single rows")
    ap.add_argument("--forcing-rows", action="store_true", help="also print, per scenario, the percentiles of the forcing F and the "
                    "energy imbalance N at the last summary year (diagnosed from the stored rows: the projection then stores C too)")
    ap.add_argument("--carbon", action="store_true", help="also print, per scenario, the percentiles of the CO2 airborne fraction and "
                    "of the CH4 lifetime scaling alpha at the last summary year (diagnosed from the stored rows: the projection then "
                    "stores C too)")
    ap.add_argument("--drivers", action="store_true", help="rank the parameters by the share of the spread of T they explain")
    ap.add_argument("--sea-level", action="store_true", help="also print, per scenario, the percentiles of the sea-level rise at the last "
                    "step and of the year it first reaches 0.5 m (component priors illustrative, not a calibration)")
    a = ap.parse_args()
    n_steps, N = 750, a.members
    run_years = 1750.0 + np.arange(n_steps)
    years, T_obs, sigma = scenario.read_observations_csv(os.path.join(ROOT, "tests", "golden", "obs_synthetic.csv"))
    obs = constrain.Observations.from_years(run_years, years, T_obs, sigma, baseline=(1900, 1950))
    p = params.sample_ensemble_shard(params.default_params("multigas"), N, 0, N, device="cuda:0")
    E = emissions.rcp_like_emissions(n_steps, 3)
    t_branch = int(obs.window[1])                             # the first step after the last observed year
    E_s = np.repeat(E[None], len(SCENARIOS), axis=0)
    for s, f in enumerate(SCENARIOS.values()):
        E_s[s, t_branch:, 0] *= f
    sf = None
    if a.forcing:                                             # the scenarios share the tables of the history, like its emissions
        sc = params.sample_forcing_scales(3, N, 0, N, [(0.9, 1.1)] * 3 + [(0.3, 2.0), (0.5, 1.5)], device="cuda:0")
        p["f_scale"], p["fx_scale"] = sc[:3], sc[3:]
        volcanic = np.where(np.arange(n_steps) % 37 == 5, -2.5, 0.0) * (np.arange(n_steps) < t_branch)
        sf = ScenarioForcings([np.stack([-0.9 * E_s[s, :, 0] / E[:, 0].max(), volcanic], 1) for s in range(len(SCENARIOS))],
                              ("aerosol", "volcanic"))

    hist = EnsembleEngine(p, N, E, observations=obs, forcing=sf.scenario(0) if sf else None, store_trajectory=False,
                          device="cuda:0")
    hist.run(0, t_branch, mode="auto")
    keep = constrain.accept_rejection(hist.chi2(), constrain.ACCEPT_SEED, 0, N)
    how = dict(weights=constrain.importance_weights(hist.chi2())) if a.weights else dict(accepted=keep)

    out_steps = [t for t in range(t_branch, n_steps, 10)] + [n_steps - 1]
    torch.cuda.synchronize()
    p_proj, n_proj, R0, S0 = p, N, hist.R, hist.S
    if a.resample:                                            # a dense equal-weight posterior: only it is stepped from here on
        plan = constrain.resample(how["weights"], a.resample, seed=constrain.ACCEPT_SEED) if a.weights \
            else constrain.resample(keep, a.resample, seed=constrain.ACCEPT_SEED)
        (p_proj, R0, S0), n_proj, how = hist.resampled(plan), plan.n_members, {}
        print(f"resampled {N} members into {n_proj} equal-weight ones ({int(torch.unique(plan.src).numel())} distinct sources)")
    proj = EnsembleEngine(p_proj, n_proj, E_s, R0=R0, S0=S0, output_steps=out_steps, store_concentrations=a.forcing_rows or a.carbon,
                          scenario_names=list(SCENARIOS), forcing=sf, device="cuda:0")
    proj.run(t_branch, n_steps, mode="auto")
    pct = (5.0, 50.0, 95.0)
    sums = [proj.gather_summary(out_steps, percentiles=pct, scenario=s, **how) for s in range(proj.n_scenarios)]
    scenario.write_scenario_summary_csv(a.out, proj.scenario_names, run_years[out_steps], sums, pct)
    if sf is not None:
        aer = p_proj["fx_scale"][0] if a.resample else p["fx_scale"][0][how["weights"] > 0 if a.weights else keep]
        print(f"aerosol scale: prior 0.3 .. 2.0, {'resampled' if a.resample else 'weighted' if a.weights else 'accepted'} members {float(aer.min()):.2f} .. {float(aer.max()):.2f} "
              f"(mean {float(aer.mean()):.2f})")
    used = f"{int(keep.sum())} accepted"
    if a.weights and not a.resample:
        used = f"{int(sums[0]['count'][0])} weighted, ess {sums[0]['ess']:.1f} (rejection sampling: {int(keep.sum())} accepted)"
    print(f"{N} members, {used} on {obs.n_obs} observed years; branch at {int(run_years[t_branch])}; "
          f"projection mode {proj.last_mode}; summary -> {a.out}")
    for name, sm in zip(proj.scenario_names, sums):
        q = sm["percentiles"][-1].tolist()
        print(f"  {name:5s} T({int(run_years[-1])}) 5/50/95 %: {q[0]:.3f} / {q[1]:.3f} / {q[2]:.3f} K")
    if a.metrics:
        from fiveeqscm_amd import metrics
        from fiveeqscm_amd.distributed import gather_summary, gather_weighted_summary
        levels = tuple(float(v) for v in a.metrics.split(","))
        what, when = "peak warming", "first stored year at or above"
        if a.smooth:                                            # the W-row running mean of the evenly stored rows, dated at its centre
            sm = proj.running_mean(a.smooth, rows=slice(0, len(range(t_branch, n_steps, 10))))
            m = metrics.trajectory_metrics(sm.rows, sm.steps, levels=levels)
            what, when = f"peak of the {a.smooth}-row mean", f"centre year of the first {a.smooth}-row mean at or above"
        else:
            m = proj.trajectory_metrics(levels=levels)          # all scenarios in one launch, stored steps only
        w = how.get("weights")
        for s, name in enumerate(proj.scenario_names):
            peak = m.peak[s].reshape(1, -1)
            if w is not None:
                q = gather_weighted_summary(peak, w, pct)["percentiles"][0].tolist()
            else:
                q = gather_summary(peak[:, how["accepted"]].contiguous() if "accepted" in how else peak, pct)["percentiles"][0].tolist()
            print(f"  {name:5s} {what} 5/50/95 %: {q[0]:.3f} / {q[1]:.3f} / {q[2]:.3f} K")
            first = m.first[s] if "accepted" not in how else m.first[s][:, how["accepted"]]
            for l, (crossed, total) in enumerate(metrics.exceedance(first, weights=w)):
                line = f"        P(T >= {levels[l]:g} K) = {crossed / total:.4f}"
                if crossed:
                    c = metrics.crossing_summary(first[l], run_years, pct, weights=w)["percentiles"][0].tolist()
                    line += f"; {when}, among those that cross, 5/50/95 %: {c[0]:.0f} / {c[1]:.0f} / {c[2]:.0f}"
                print(line)
    if a.forcing_rows:
        from fiveeqscm_amd.distributed import gather_summary, gather_weighted_summary
        res = proj.forcing_rows(want=("F", "N"))                # every scenario; F and N need no consecutive steps
        w = how.get("weights")
        for s, name in enumerate(proj.scenario_names):
            for what, rows, unit in (("F", res.F[s], "W m-2"), ("N", res.N[s], "W m-2")):
                row = rows[-1:].contiguous()
                if w is not None:
                    q = gather_weighted_summary(row, w, pct)["percentiles"][0].tolist()
                else:
                    q = gather_summary(row[:, how["accepted"]].contiguous() if "accepted" in how else row, pct)["percentiles"][0].tolist()
                print(f"  {name:5s} {what}({int(run_years[-1])}) 5/50/95 %: {q[0]:.3f} / {q[1]:.3f} / {q[2]:.3f} {unit}")
    if a.carbon:
        from fiveeqscm_amd.distributed import gather_summary, gather_weighted_summary
        last = slice(proj.n_rows - 1, proj.n_rows)              # one-row blocks of the last stored step; nothing is carried
        af = proj.carbon_rows(want=("fraction",), gases=(0,), rows=last).fraction
        al = proj.carbon_rows(want=("alpha",), gases=(1,), rows=last).alpha
        w = how.get("weights")
        for s, name in enumerate(proj.scenario_names):
            for what, rows in (("CO2 airborne fraction", af[s, :, 0]), ("CH4 alpha", al[s, :, 0])):
                row = rows.contiguous()
                if w is not None:
                    q = gather_weighted_summary(row, w, pct)["percentiles"][0].tolist()
                else:
                    q = gather_summary(row[:, how["accepted"]].contiguous() if "accepted" in how else row, pct)["percentiles"][0].tolist()
                print(f"  {name:5s} {what}({int(run_years[-1])}) 5/50/95 %: {q[0]:.4f} / {q[1]:.4f} / {q[2]:.4f}")
    if a.drivers:
        names = proj.parameter_rows()[0]
        peak = proj.trajectory_metrics().peak
        cases = [("all members", {})] + ([("posterior", how)] if how else [])
        for s, name in enumerate(proj.scenario_names):
            y = torch.stack([proj.T[s, -1].to(torch.float64), peak[s]])
            for label, kw in cases:
                d = proj.drivers(y, **kw)
                print(f"  {name:5s} drivers, {label} (ess {d.moments.ess:.0f}, eta2 of an unrelated parameter {d.noise_floor:.4f}):")
                for k, what in enumerate((f"T({int(run_years[-1])})", "peak")):
                    top = torch.argsort(d.eta2[:, k].nan_to_num(-1.0), descending=True)[:5].tolist()
                    print(f"        {what:8s} " + ", ".join(f"{names[i]} {float(d.eta2[i, k]):.3f} (r {float(d.moments.corr[i, k]):+.2f})" for i in top))
    if a.sea_level:
        from fiveeqscm_amd import metrics
        from fiveeqscm_amd.distributed import gather_summary, gather_weighted_summary
        from fiveeqscm_amd.sea_level import SeaLevelComponents
        # Sea-level rise integrates every year's warming, so it needs the stored rows of CONSECUTIVE steps: a second projection
        # from the same branch state stores every step (the summary engine above stores every tenth).
        # The component priors below are ILLUSTRATIVE, NOT A CALIBRATION: round numbers of the right order of magnitude, drawn
        # independently per member, so that the example has a spread to print.  The levels are rises since the branch year.
        sea = EnsembleEngine(p_proj, n_proj, E_s, R0=R0, S0=S0, output_steps=list(range(t_branch, n_steps)), store_concentrations=False,
                             scenario_names=list(SCENARIOS), forcing=sf, device="cuda:0")
        sea.run(t_branch, n_steps, mode="auto")
        rng = np.random.default_rng(2016)
        u = lambda lo, hi: rng.uniform(lo, hi, n_proj)                                   # noqa: E731
        comp = SeaLevelComponents(
            ("expansion", "glaciers", "greenland", "antarctica"), ("relax", "relax", "rate", "rate"),
            tau=np.stack([u(150.0, 500.0), u(100.0, 300.0), np.ones(n_proj), np.ones(n_proj)]),              # years
            a=np.stack([u(0.2, 0.6), u(0.15, 0.35), u(0.0004, 0.0016), u(0.0002, 0.0020)]),                  # m / K; m / yr / K
            b=np.stack([np.zeros(n_proj), np.zeros(n_proj), u(0.0, 0.0004), u(0.0, 0.0006)]),
            T0=np.stack([u(0.6, 1.0), u(0.4, 0.9), u(0.5, 1.0), u(0.7, 1.2)]),                               # K: in balance near today
            cap=np.stack([np.full(n_proj, np.inf), u(0.30, 0.41), np.full(n_proj, np.inf), np.full(n_proj, np.inf)]))
        sl = sea.sea_level_rows(comp)                              # all scenarios in one launch: total [S, n_rows, N] fp64
        m = metrics.trajectory_metrics(sl.total, sl.steps, levels=(0.5,))
        w = how.get("weights")
        print(f"  sea-level rise since {int(run_years[t_branch])} (illustrative component priors, not a calibration):")
        for s, name in enumerate(sea.scenario_names):
            row = sl.total[s, -1:].contiguous()
            if w is not None:
                q = gather_weighted_summary(row, w, pct)["percentiles"][0].tolist()
            else:
                q = gather_summary(row[:, how["accepted"]].contiguous() if "accepted" in how else row, pct)["percentiles"][0].tolist()
            print(f"  {name:5s} rise({int(run_years[-1])}) 5/50/95 %: {q[0]:.3f} / {q[1]:.3f} / {q[2]:.3f} m")
            first = m.first[s] if "accepted" not in how else m.first[s][:, how["accepted"]]
            (crossed, total), = metrics.exceedance(first, weights=w)
            line = f"        P(rise >= 0.5 m) = {crossed / total:.4f}"
            if crossed:
                c = metrics.crossing_summary(first[0], run_years, pct, weights=w)["percentiles"][0].tolist()
                line += f"; first year at or above, among those that cross, 5/50/95 %: {c[0]:.0f} / {c[1]:.0f} / {c[2]:.0f}"
            print(line)
        sea.close()
    hist.close()
    proj.close()


if __name__ == "__main__":
    main()
