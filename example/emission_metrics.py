#!/usr/bin/env python3
"""Emission metrics with the ensemble's uncertainty: GWP and GTP of CH4 and N2O against CO2 at 20, 100 and 500 years.

One scenario engine runs a constant-concentration background (no emissions: every gas stays at its pre-industrial
concentration, the warming at 0) and the same background with a pulse of CO2, of CH4 and of N2O in year 0 — four scenarios, the
same members.  EnsembleEngine.pulse_response then forms, per member, the differences of forcing, warming and concentration
between each pulse scenario and the background and sums them to the horizons: one streaming HIP pass over the stored rows
(include/fiveeq.h, "PULSE RESPONSE").  The ratios per kilogram go through gather_summary for their percentiles.

--weights weights every member by a likelihood instead (here: a synthetic one on the member's ECS, 3 +- 0.75 K) and prints
the exact weighted percentiles of gather_weighted_summary.

    python example/emission_metrics.py [--members N] [--weights]

Needs an MI355X.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fiveeqscm_amd import constrain, params, pulse  # noqa: E402
from fiveeqscm_amd.distributed import gather_summary, gather_weighted_summary  # noqa: E402
from fiveeqscm_amd.engine import EnsembleEngine  # noqa: E402

GASES = ("CO2", "CH4", "N2O")
# small pulses (the metrics are derivatives): 1 GtC, 10 Mt CH4, 1 Mt N2O-N; and what one emission unit of each weighs in kg
SIZES = (1.0, 10.0, 1.0)
MASS_KG = (44.009 / 12.011 * 1e12, 1e9, 44.013 / 28.014 * 1e9)
HORIZONS = (20, 100, 500)
PCT = (5.0, 50.0, 95.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=10_000)
    ap.add_argument("--weights", action="store_true", help="importance-weight the members by a synthetic likelihood on ECS")
    args = ap.parse_args()
    N = args.members
    base = params.default_params("multigas")
    p = params.sample_ensemble_shard(base, N)
    n_steps = HORIZONS[-1]
    exp = pulse.pulse_experiment(np.zeros((n_steps, 3)), 0, list(enumerate(SIZES)), n_steps)
    t0 = time.perf_counter()
    eng = EnsembleEngine(p, N, exp.emissions, device="cuda:0", scenario_names=exp.scenario_names, output_steps=exp.output_steps)
    eng.run()
    res = eng.pulse_response(exp, HORIZONS)
    gwp, gtp = res.gwp(0, mass_kg=MASS_KG), res.gtp(0, mass_kg=MASS_KG)
    torch.cuda.synchronize()
    print(f"{N} members x {1 + len(SIZES)} scenarios x {n_steps} years, run and pulse response: {time.perf_counter() - t0:.2f} s")
    weights = None
    if args.weights:
        ecs = eng.parameter_rows(["ECS"])[1][0]
        weights = constrain.importance_weights(((ecs - 3.0) / 0.75) ** 2)

    def summary(row):
        if weights is None:
            return gather_summary(row.contiguous(), PCT)["percentiles"][0].tolist()
        return gather_weighted_summary(row.contiguous(), weights, PCT)["percentiles"][0].tolist()

    agwp = res.agwp()
    for h, years in enumerate(HORIZONS):
        lo, mid, hi = summary(agwp[0, h:h + 1])
        print(f"AGWP-{years} of CO2: {mid:.4g} [{lo:.4g}, {hi:.4g}] W yr m-2 per GtC")
    print(f"{'':10s}" + "".join(f"{f'{name}-{years}':>34s}" for name in ("GWP", "GTP") for years in HORIZONS))
    for g in (1, 2):
        cells = []
        for x in (gwp, gtp):
            for h in range(len(HORIZONS)):
                lo, mid, hi = summary(x[g, h:h + 1])
                cells.append(f"{mid:10.4g} [{lo:9.4g}, {hi:9.4g}]")
        print(f"{GASES[g]:10s}" + "".join(f"{c:>34s}" for c in cells))
    print("(per kilogram, against CO2; median [5 %, 95 %] over the " + ("weighted " if args.weights else "") + "ensemble)")


if __name__ == "__main__":
    main()
