"""Generates tests/golden/obs_synthetic.csv: a synthetic observed-temperature record for the constrained-ensemble tests and
example (no real record ships with the project).

The "truth" is one known member — the centre of the default three-gas set, params.default_params("multigas") — driven by
emissions.rcp_like_emissions(750, 3) through the C oracle.  Step t of the run is year 1750 + t.  The record covers the 170
steps 150..319 (years 1900..2069); T is the member's anomaly against its own mean over the first 51 of them (1900..1950, the
baseline period), plus Gaussian noise of sigma = 0.1 K drawn with a fixed seed.

    python tests/golden/make_obs_synthetic.py      # rewrites obs_synthetic.csv next to this file
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

N_STEPS = 750
YEAR0 = 1750                      # year of step 0
OBS_FIRST, OBS_STEPS = 150, 170   # observed steps 150..319
BASELINE_STEPS = 51               # the first 51 observed steps are the reference period
SIGMA = 0.1
SEED = 20261016


def truth():
    """(run_years [750], T [750]) of the generating member."""
    from fiveeqscm_amd import emissions, params
    from oracle import c_oracle
    E = emissions.rcp_like_emissions(N_STEPS, 3)
    T = c_oracle.run(E, params.default_params("multigas"), 1, keep=("T",))["T"][:, 0]
    return YEAR0 + np.arange(N_STEPS, dtype=np.float64), T


def main():
    from fiveeqscm_amd import scenario
    years, T = truth()
    sl = slice(OBS_FIRST, OBS_FIRST + OBS_STEPS)
    anomaly = T[sl] - T[OBS_FIRST:OBS_FIRST + BASELINE_STEPS].mean()
    noise = np.random.default_rng(SEED).normal(0.0, SIGMA, OBS_STEPS)
    scenario.write_observations_csv(
        os.path.join(HERE, "obs_synthetic.csv"), years[sl], anomaly + noise, SIGMA,
        comment=f"synthetic record: default multigas centre member, rcp_like_emissions({N_STEPS}, 3), year = {YEAR0} + step;\n"
                f"anomaly against {int(years[OBS_FIRST])}..{int(years[OBS_FIRST + BASELINE_STEPS - 1])}, "
                f"noise N(0, {SIGMA}) seed {SEED} (tests/golden/make_obs_synthetic.py)")


if __name__ == "__main__":
    main()
