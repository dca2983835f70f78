#!/usr/bin/env python3
"""A/B of the per-member forcing scales (forcing=) against the same run without them, in ONE process, alternating the two.

    python tools/forcing_ab.py [--repeats R] [--quick]

Legs (750 steps, three external forcing categories, every scale row sampled):
  config 3 shape: 1M members x 3 gases fp64 (pools 4 + 1 + 1), every C / T row stored, mode per_step and mode fused;
  the same per_step leg with observations= on both sides (the 170-step window of tests/golden/obs_synthetic.csv);
  config 5 shard: 12.5M members x 3 gases fp32, mode fused, no stored rows.
Prints one line per leg: median wall time per run with and without, the ratio, and for per_step the ratio
bytes_per_member_step predicts ((248 + 8 (G + K)) / 248 = 1.19 for config 3)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fiveeqscm_amd import emissions, scenario  # noqa: E402
from fiveeqscm_amd import params as prm  # noqa: E402
from fiveeqscm_amd.constrain import Observations  # noqa: E402
from fiveeqscm_amd.engine import EnsembleEngine  # noqa: E402
from fiveeqscm_amd.forcing import ExternalForcings  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="small members, for a dry run of the script")
    a = ap.parse_args()
    n_steps, G, K = 750, 3, 3
    y, T, s = scenario.read_observations_csv(os.path.join(ROOT, "tests", "golden", "obs_synthetic.csv"))
    obs = Observations.from_years(1750.0 + np.arange(n_steps), y, T, s, baseline=(1900, 1950))
    E = emissions.rcp_like_emissions(n_steps, G)
    tt = np.arange(n_steps)
    fx = ExternalForcings(np.stack([-1.1 * E[:, 0] / E[:, 0].max(), np.where(tt % 37 == 5, -2.5, 0.0),
                                    0.1 * np.sin(2 * np.pi * tt / 11.0)], 1), ("aerosol", "volcanic", "solar"))
    legs = [("config3 1M fp64", 1_000_000, torch.float64, "per_step", True, None),
            ("config3 1M fp64", 1_000_000, torch.float64, "fused", True, None),
            ("config3 1M fp64 + obs", 1_000_000, torch.float64, "per_step", True, obs),
            ("config5 12.5M fp32", 12_500_000, torch.float32, "fused", False, None)]
    print(f"# {torch.cuda.get_device_name(0)}; {n_steps} steps, {K} categories, G + K = {G + K} scale rows; "
          f"median of {a.repeats} alternating runs each")
    base = prm.default_params("multigas")
    for name, N, dt, mode, store, o in legs:
        if a.quick:
            N = 20_000
        p = prm.sample_ensemble_shard(base, N, 0, N, device="cuda:0", dtype=dt)
        sc = prm.sample_forcing_scales(base, N, ranges=[(0.8, 1.2)] * G + [(0.3, 2.0), (0.5, 1.5), (0.5, 1.5)], device="cuda:0")
        pf = dict(p, f_scale=sc[:G].to(dt), fx_scale=sc[G:].to(dt))
        engs = {k: EnsembleEngine(pp, N, E, dtype=dt, store_trajectory=store, observations=o, forcing=f, device="cuda:0")
                for k, pp, f in (("plain", p, None), ("forcing", pf, fx))}
        times = {k: [] for k in engs}
        for k, e in engs.items():                                 # warm-up: first launches, graph-free
            e.run(mode=mode)
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for k, e in engs.items():
                e.reset_state()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.run(mode=mode)
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
        med = {k: float(np.median(v)) for k, v in times.items()}
        ratio = med["forcing"] / med["plain"]
        line = (f"{name:22s} {mode:9s} plain {med['plain'] * 1e3:9.2f} ms  forcing {med['forcing'] * 1e3:9.2f} ms  "
                f"ratio {ratio:.4f}  (runs plain {[round(v * 1e3, 2) for v in times['plain']]}, "
                f"forcing {[round(v * 1e3, 2) for v in times['forcing']]})")
        if mode == "per_step":
            pred = engs["forcing"].bytes_per_member_step("per_step") / engs["plain"].bytes_per_member_step("per_step")
            line += f"  bytes_per_member_step predicts {pred:.4f}"
        print(line, flush=True)
        for e in engs.values():
            e.close()
        del engs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
