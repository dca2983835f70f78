#!/usr/bin/env python3
"""Constrain a Latin-hypercube ensemble against an observed record and report constrained and unconstrained percentiles.

The record is the synthetic one committed for the tests (tests/golden/obs_synthetic.csv, made by
tests/golden/make_obs_synthetic.py: one known member plus 0.1 K noise over 1900..2069).  Needs an MI355X.

    python example/constrained_ensemble.py [--members N] [--dtype f64|f32]
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


if __name__ == "__main__":
    main()
