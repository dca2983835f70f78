#!/usr/bin/env python3
"""Constrain a Latin-hypercube ensemble against an observed record and report constrained and unconstrained percentiles.

The record is the synthetic one committed for the tests (tests/golden/obs_synthetic.csv, made by
tests/golden/make_obs_synthetic.py: one known member plus 0.1 K noise over 1900..2069).  Needs an MI355X.

    python example/constrained_ensemble.py [--members N] [--dtype f64|f32] [--forcing] [--co2-record] [--concentration-driven]
                                           [--co2-emission-driven] [--variability SIGMA PHI] [--minor-gases]
                                           [--aerosols]

--forcing adds forcing uncertainty (EnsembleEngine(forcing=), fiveeqscm_amd/forcing.py): an aerosol-like cooling scaled per
member, and the accepted range of ECS with a shared and with a sampled scale.
--co2-record also makes a CO2 record the same way (one known member's stored concentration plus 1 ppm noise over the same
years), scores the stored T and C rows against both records (EnsembleEngine.score) and prints the posterior spread of the
carbon-cycle parameter r0 of CO2 with and without the CO2 record.
--concentration-driven runs the calibration the other way round (ConcentrationDrivenEngine): the history 1750..2019 is driven by
"observed" concentrations, every member carries its own aerosol scale and is scored against the warming record in-loop; the
weighted ensemble then branches into an emission-driven projection to 2499 through R0 / S0.
--co2-emission-driven (with --concentration-driven) keeps CO2 emission-driven in that history (MixedDriveEngine with
concentration_gases=(1, 2)): CH4 and N2O still follow the "observed" concentrations, CO2 takes the scenario's emissions, so each
member's carbon-cycle parameters show in its CO2 concentration and through it in the warming it is scored on, instead of only
in diagnosed CO2 emissions; the spread of CO2 at the cut is printed, and the projection continues the scenario's own
cumulative CO2 emissions (the mean diagnosed cumE is used for CH4 and N2O only).
--variability SIGMA PHI gives every member its own AR(1) forcing noise (standard deviation SIGMA W m-2, lag-1 autocorrelation
PHI; forcing.ar1_noise_rows, EnsembleEngine(member_forcing=)), constrains with the in-loop misfit and prints the accepted
fraction and the 5-95 % range of the final T with and without the variability.
--minor-gases adds two SYNTHETIC constant-lifetime species (made-up lifetimes, efficiencies and emissions: no literature values)
whose lifetime and radiative efficiency every member scales by its own factors, sampled on the same shard-computable design
(minor_gases.minor_gas_rows, EnsembleEngine(member_forcing=)); with --variability their forcing is added onto the noise rows
(into=), otherwise it runs alone.
--aerosols replaces the scaled aerosol series of --forcing by aerosol forcing computed from emissions with each member's own
shape parameters, aerosol-radiation coefficients and present-day ERFaci (aerosols.aerosol_rows, aci_scale_for_target,
EnsembleEngine(member_forcing=)) and prints the accepted range of ECS beside that of the --forcing run.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=100_000)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--forcing", action="store_true",
                    help="also sample an aerosol scale per member and print the accepted range of ECS with and without it")
    ap.add_argument("--co2-record", action="store_true",
                    help="also score the stored CO2 rows against a synthetic CO2 record and print what it does to r0 of CO2")
    ap.add_argument("--concentration-driven", action="store_true",
                    help="also constrain a concentration-driven history with an aerosol scale per member and branch into a projection")
    ap.add_argument("--co2-emission-driven", action="store_true",
                    help="with --concentration-driven: keep CO2 emission-driven in the history (CH4 and N2O prescribed)")
    ap.add_argument("--variability", nargs=2, type=float, metavar=("SIGMA", "PHI"),
                    help="also give every member AR(1) forcing noise (W m-2, lag-1 autocorrelation) and constrain with it")
    ap.add_argument("--minor-gases", action="store_true",
                    help="also give every member two synthetic minor gases with its own lifetime and efficiency scales")
    ap.add_argument("--aerosols", action="store_true",
                    help="also compute every member's aerosol forcing from synthetic SO2 / BC+OC emissions and compare with --forcing")
    a = ap.parse_args()
    n_steps, N = 750, a.members
    run_years = 1750.0 + np.arange(n_steps)
    years, T_obs, sigma = scenario.read_observations_csv(os.path.join(ROOT, "tests", "golden", "obs_synthetic.csv"))
    obs = constrain.Observations.from_years(run_years, years, T_obs, sigma, baseline=(1900, 1950))
    dtype = torch.float64 if a.dtype == "f64" else torch.float32
    p = params.sample_ensemble_shard(params.default_params("multigas"), N, 0, N, device="cuda:0", dtype=dtype)
    last = n_steps - 1
    eng = EnsembleEngine(p, N, emissions.rcp_like_emissions(n_steps, 3), dtype=dtype, observations=obs,
                         output_steps=[last], store_concentrations=False, device="cuda:0")
    eng.run(mode="auto")
    chi2 = eng.chi2()
    keep = constrain.accept_rejection(chi2, constrain.ACCEPT_SEED, 0, N)
    pct = (5.0, 50.0, 95.0)
    prior = eng.gather_summary([last], percentiles=pct)
    post = eng.gather_summary([last], percentiles=pct, accepted=keep)
    print(f"{N} members ({a.dtype}, mode {eng.last_mode}), {obs.n_obs} observed years; chi2 min {float(chi2.min()):.1f}, "
          f"median {float(chi2.median()):.1f}; accepted {int(post['count'][0])}")
    for label, s in (("unconstrained", prior), ("constrained", post)):
        q = s["percentiles"][0].tolist()
        print(f"  T({int(run_years[last])}) {label:13s} 5/50/95 %: {q[0]:.3f} / {q[1]:.3f} / {q[2]:.3f} K")
    eng.close()
    if a.forcing or a.aerosols:
        forcing_uncertainty(p, N, n_steps, dtype, obs)
    if a.aerosols:
        aerosol_emissions(p, N, n_steps, dtype, obs)
    if a.co2_record:
        co2_record(p, N, n_steps, dtype, obs, run_years, years)
    if a.co2_emission_driven and not a.concentration_driven:
        ap.error("--co2-emission-driven is an option of --concentration-driven")
    if a.concentration_driven:
        concentration_driven_history(p, N, n_steps, dtype, run_years, years, T_obs, sigma, co2_emission_driven=a.co2_emission_driven)
    if a.variability or a.minor_gases:
        internal_variability(p, N, n_steps, dtype, obs, run_years, *(a.variability or (None, None)), minor=a.minor_gases)


def co2_record(p, N, n_steps, dtype, obs, run_years, years, truth=12345, sigma_ppm=1.0):
    """--co2-record: the run stores the rows of the observed years; member `truth`'s CO2 plus noise is the record.  T barely
    constrains the carbon cycle, the observed concentration does: the weighted spread of r0 of CO2 narrows once its chi2 is
    added to that of T."""
    steps = np.searchsorted(run_years, years)
    stored = sorted(set(int(t) for t in steps) | set(int(t) for t in obs.live_steps))
    eng = EnsembleEngine(p, N, emissions.rcp_like_emissions(n_steps, 3), dtype=dtype, output_steps=stored, device="cuda:0")
    eng.run(mode="auto")
    row_of = {t: r for r, t in enumerate(eng.out_steps.tolist())}
    truth %= N
    series = eng.C[[row_of[int(t)] for t in steps], 0, truth].double().cpu().numpy()
    noisy = series + np.random.default_rng(2017).normal(0.0, sigma_ppm, series.size)
    co2 = constrain.Observations.absolute(run_years, years, noisy, sigma_ppm)
    s = eng.score({"T": obs, 0: co2})
    r0 = p["r0"][0].double()
    order = torch.argsort(r0)
    print(f"scored {s.n_obs['T']} T and {s.n_obs[0]} CO2 observations from the stored rows (mode {eng.last_mode}); r0 of CO2 of the "
          f"known member: {float(r0[truth]):.2f}")
    for label, chi2 in (("T record only", s.chi2["T"]), ("T and CO2 records", s.total)):
        w = constrain.importance_weights(chi2)[order].double()
        cdf = torch.cumsum(w, 0) / w.sum()
        lo, mid, hi = (float(r0[order][int(torch.searchsorted(cdf, torch.tensor(q, dtype=cdf.dtype, device=cdf.device)))]) for q in (0.05, 0.5, 0.95))
        print(f"  r0[CO2] {label:18s} 5/50/95 %: {lo:.2f} / {mid:.2f} / {hi:.2f}   (90 % width {hi - lo:.2f})")
    eng.close()


def concentration_driven_history(p, N, n_steps, dtype, run_years, years, T_obs, sigma, cut=270, co2_emission_driven=False):
    """--concentration-driven: the concentrations of the default member's forward run stand in for the observed record up to
    2019 (step `cut`).  History: every member reaches exactly those concentrations (its own emissions are diagnosed), scales the
    aerosol-like cooling by its own factor and accumulates its misfit against the warming observed up to 2019.  Projection: a
    forward forcing= engine with the same scale rows starts from the history's pools and boxes (R0 / S0) at step `cut`; its
    drive table continues the cumulative emissions from the ensemble mean of the history's diagnosed cumE (the first `cut` rows
    of its emissions hold that mean rate; they are not run).  co2_emission_driven: the history is a MixedDriveEngine with CH4 and
    N2O prescribed and CO2 from the scenario's emissions, whose rows the projection keeps."""
    from fiveeqscm_amd.engine import ConcentrationDrivenEngine, MixedDriveEngine
    from fiveeqscm_amd.forcing import ExternalForcings
    E = emissions.rcp_like_emissions(n_steps, 3)
    base = params.default_params("multigas")
    one = EnsembleEngine(base, 1, E, device="cuda:0")
    one.run(mode="fused")
    conc = one.C[:cut, :, 0].cpu().numpy()
    one.close()
    aerosol = -0.9 * E[:, 0] / E[:, 0].max()
    scales = params.sample_forcing_scales(3, N, ranges=[(1.0, 1.0)] * 3 + [(0.3, 2.0)], device="cuda:0")
    ps = dict(p, fx_scale=scales[3:].to(dtype))
    seen = years < run_years[cut]
    obs = constrain.Observations.from_years(run_years[:cut], years[seen], T_obs[seen], np.broadcast_to(sigma, years.shape)[seen],
                                            baseline=(1900, 1950))
    kw = dict(dtype=dtype, forcing=ExternalForcings(aerosol[:cut], ("aerosol",)), observations=obs, device="cuda:0")
    if co2_emission_driven:
        hist = MixedDriveEngine(ps, N, E[:cut], conc, (1, 2), output_steps=[cut - 1], **kw)
    else:
        hist = ConcentrationDrivenEngine(ps, N, conc, store_trajectory=False, **kw)
    hist.run()
    chi2 = hist.chi2()
    w = constrain.importance_weights(chi2)
    ess = float(w.double().sum() ** 2 / (w.double() ** 2).sum())
    print(f"concentration-driven history to {int(run_years[cut - 1])}: {obs.n_obs} observed years, chi2 min {float(chi2.min()):.1f}, "
          f"effective sample size {ess:.0f} of {N}")
    E_proj = E.copy()
    E_proj[:cut] = hist.cumE.double().mean(1).cpu().numpy()[None, :] / cut          # the drive's cumulative emissions at the cut
    if co2_emission_driven:
        co2 = hist.X[0, 0].double()
        print(f"  CO2 emission-driven: CO2({int(run_years[cut - 1])}) spans {float(co2.min()):.1f} .. {float(co2.max()):.1f} ppm over the "
              f"members (prescribed: {conc[cut - 1, 0]:.1f})")
        E_proj[:cut, 0] = E[:cut, 0]                                                # CO2 went by the scenario: its own cumulative sum
    last = n_steps - 1
    proj = EnsembleEngine(ps, N, E_proj, dtype=dtype, forcing=ExternalForcings(aerosol, ("aerosol",)), R0=hist.R, S0=hist.S,
                          output_steps=[last], store_concentrations=False, device="cuda:0")
    proj.run(cut, n_steps, mode="fused")
    pct = (5.0, 50.0, 95.0)
    for label, s in (("unweighted", proj.gather_summary([last], percentiles=pct)),
                     ("weighted", proj.gather_summary([last], percentiles=pct, weights=w))):
        q = s["percentiles"][0].tolist()
        print(f"  T({int(run_years[last])}) {label:11s} 5/50/95 %: {q[0]:.3f} / {q[1]:.3f} / {q[2]:.3f} K")
    hist.close()
    proj.close()


def synthetic_minor_gases(N, n_steps, dtype, into=None):
    """--minor-gases: two synthetic species (lifetimes 14 and 230 yr, emissions ramping up from 1950 and levelling off; the
    numbers are illustrations, not data) with a per-member lifetime scale in 0.8..1.2 and efficiency scale in 0.7..1.3 — two
    more dimensions of the design, after the forcing scales' — as member_forcing rows, added onto `into` when given."""
    from fiveeqscm_amd.minor_gases import minor_gas_rows
    t = np.arange(n_steps, dtype=np.float64)
    ramp = np.clip((t - 200.0) / 120.0, 0.0, 1.0)
    E = np.stack([40.0 * ramp, 3.0 * ramp ** 2], 1)                       # kt / yr
    scales = params.sample_forcing_scales(3, N, ranges=[(1.0, 1.0)] * 4 + [(0.8, 1.2), (0.7, 1.3)])[4:]
    tau = np.array([14.0, 230.0])[:, None] * scales[0][None, :]
    eff = np.array([0.16e-3, 0.57e-3])[:, None] * scales[1][None, :]      # W m-2 per ppt
    out = minor_gas_rows(E, tau, [0.06, 0.04], eff, N, into=into, device="cuda:0", dtype=dtype)
    print(f"minor gases: {out.species} synthetic species, lifetime x0.8..1.2 and efficiency x0.7..1.3 per member; forcing in "
          f"{int(1750 + n_steps - 1)}: {float(out.rows[-1].min()):.3f} .. {float(out.rows[-1].max()):.3f} W m-2"
          + (" (on top of the noise rows)" if into is not None else ""))
    return out.rows


def internal_variability(p, N, n_steps, dtype, obs, run_years, sigma_f, phi, minor=False):
    """--variability: the observed record contains year-to-year noise a deterministic member cannot produce, so the chi2
    charges every member for it and the posterior comes out too narrow.  With a stochastic forcing realisation per member
    (rows [n_steps, N]: n_steps N w bytes on the device, 3 GB for 1M fp32 members over 750 steps) the members carry such noise
    themselves."""
    from fiveeqscm_amd.forcing import ar1_noise_rows
    E = emissions.rcp_like_emissions(n_steps, 3)
    last = n_steps - 1
    rows = None
    if sigma_f is not None:
        rows = ar1_noise_rows(N, n_steps, sigma_f, phi, device="cuda:0", dtype=dtype)
        print(f"internal variability: AR(1) forcing noise, sigma {sigma_f} W m-2, phi {phi} ({rows.numel() * rows.element_size() / 1e6:.0f} MB of rows)")
    if minor:
        rows = synthetic_minor_gases(N, n_steps, dtype, into=rows)
    for label, mf in (("without", None), ("with", rows)):
        eng = EnsembleEngine(p, N, E, dtype=dtype, observations=obs, member_forcing=mf, output_steps=[last],
                             store_concentrations=False, device="cuda:0")
        eng.run(mode="auto")
        keep = constrain.accept_rejection(eng.chi2(), constrain.ACCEPT_SEED, 0, N)
        n_keep = int(keep.sum())
        if n_keep:
            q = eng.gather_summary([last], percentiles=(5.0, 95.0), accepted=keep)["percentiles"][0].tolist()
        else:
            q = [float("nan")] * 2
        print(f"  {label:7s} member forcing (mode {eng.last_mode}): accepted {n_keep} of {N} ({n_keep / N:.4f}); "
              f"T({int(run_years[last])}) 5-95 %: {q[0]:.3f} .. {q[1]:.3f} K")
        eng.close()


def aerosol_emissions(p, N, n_steps, dtype, obs):
    """--aerosols: aerosol forcing from emissions, its time shape the member's own.  A SYNTHETIC SO2 / BC+OC history (the
    numbers are illustrations, not data: SO2 rising from 1850, peaking in 1980 and halving by 2050; BC+OC rising later and
    levelling off) over a pre-industrial reference.  Every member draws, on dimensions of the design after those of
    --forcing and --minor-gases, its shape parameters s_SO2 and s_BCOC, its two aerosol-radiation coefficients and a present-day
    (2005..2014) ERFaci in -1.6..-0.2 W m-2, which aerosols.aci_scale_for_target turns into its beta.  A small s saturates
    early — most of such a member's cooling was in place long before the emissions peaked, and when BC+OC warms it its
    strongest cooling falls in another year — which no scale of a shared series can express."""
    from fiveeqscm_amd.aerosols import aci_scale_for_target, aerosol_rows
    t = np.arange(n_steps, dtype=np.float64)                             # step 0 is 1750
    so2 = 2.0 + 120.0 * np.clip((t - 100.0) / 130.0, 0.0, 1.0) ** 2 - 60.0 * np.clip((t - 230.0) / 70.0, 0.0, 1.0)    # Tg / yr
    bcoc = 5.0 + 35.0 * np.clip((t - 150.0) / 150.0, 0.0, 1.0)
    E_aer, base = np.stack([so2, bcoc], 1), np.array([2.0, 5.0])
    u = params.sample_forcing_scales(3, N, ranges=[(1.0, 1.0)] * 6 + [(20.0, 400.0), (10.0, 200.0), (-4.0e-3, -1.0e-3),
                                                                        (-2.0e-3, 4.0e-3), (-1.6, -0.2)])[6:]
    shape, ari, target = u[0:2], u[2:4], u[4]
    beta = aci_scale_for_target(E_aer, base, shape, target, (255, 265), N, device="cuda:0", dtype=dtype)
    rows = aerosol_rows(E_aer, base, ari, shape, beta, N, device="cuda:0", dtype=dtype).rows
    peak = 1750 + rows.argmin(0)
    print(f"aerosols from emissions: s_SO2 20..400, s_BCOC 10..200, present-day ERFaci -1.6..-0.2 W m-2 -> beta "
          f"{float(beta.min()):.2f} .. {float(beta.max()):.2f} W m-2; strongest cooling {float(rows.min()):.2f} W m-2, "
          f"its year {int(peak.min())} .. {int(peak.max())} over the members")
    E = emissions.rcp_like_emissions(n_steps, 3)
    eng = EnsembleEngine(p, N, E, dtype=dtype, observations=obs, member_forcing=rows, store_trajectory=False, device="cuda:0")
    eng.run(mode="auto")
    keep = constrain.accept_rejection(eng.chi2(), constrain.ACCEPT_SEED, 0, N)
    kept = p["ECS"][keep]
    lo, hi = (float(torch.quantile(kept, q)) for q in (0.05, 0.95)) if kept.numel() else (float("nan"),) * 2
    print(f"  from emissions (mode {eng.last_mode}) accepted {int(keep.sum()):7d}  ECS {lo:.2f} .. {hi:.2f} K   "
          "(against the fx_scale run above: one series, stretched)")
    eng.close()


def forcing_uncertainty(p, N, n_steps, dtype, obs):
    """--forcing: the same design with an aerosol-like cooling that every member scales by its own factor in 0.3..2.0 (one more
    dimension of the hypercube).  A member with high sensitivity and strong cooling fits the record as well as one with low
    sensitivity and weak cooling, so the accepted range of ECS is wider than with a forcing every member shares."""
    from fiveeqscm_amd.forcing import ExternalForcings
    E = emissions.rcp_like_emissions(n_steps, 3)
    aerosol = ExternalForcings(-0.9 * E[:, 0] / E[:, 0].max(), ("aerosol",))
    scales = params.sample_forcing_scales(3, N, ranges=[(1.0, 1.0)] * 3 + [(0.3, 2.0)], device="cuda:0")
    ecs = p["ECS"]
    print("accepted range of ECS (5 / 95 % of the accepted members), aerosol scale shared (1.0) against sampled (0.3..2.0):")
    for label, fx_scale in (("shared", np.ones(1)), ("sampled", scales[3:].to(dtype))):
        eng = EnsembleEngine(dict(p, fx_scale=fx_scale), N, E, dtype=dtype, observations=obs, forcing=aerosol,
                             store_trajectory=False, device="cuda:0")
        eng.run(mode="auto")
        keep = constrain.accept_rejection(eng.chi2(), constrain.ACCEPT_SEED, 0, N)
        kept = ecs[keep]
        lo, hi = (float(torch.quantile(kept, q)) for q in (0.05, 0.95)) if kept.numel() else (float("nan"),) * 2
        print(f"  {label:8s} accepted {int(keep.sum()):7d}  ECS {lo:.2f} .. {hi:.2f} K")
        eng.close()


if __name__ == "__main__":
    main()
