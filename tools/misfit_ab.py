#!/usr/bin/env python3
"""A/B of the in-loop misfit (observations=) against the same run without it, in ONE process, alternating the two.

    python tools/misfit_ab.py [--repeats R] [--quick]

Legs (a 750-step run with the 170-step window of tests/golden/obs_synthetic.csv, no stored rows):
  config 3 shape: 1M members x 3 gases fp64, mode per_step and mode fused;
  config 5 shard: 12.5M members x 3 gases fp32, mode fused;
  CO2-only (pools {4}) 12.5M members fp32, mode fused — with observations= this layout runs one member per lane, where the
  plain run packs two (fiveeq_capi.hip, misfit_packed_fused), so the ratio includes the unpacked kernel.
Prints one line per leg: median wall time per run with and without, the ratio, and for per_step the ratio
bytes_per_member_step predicts."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="small members, for a dry run of the script")
    a = ap.parse_args()
    n_steps = 750
    y, T, s = scenario.read_observations_csv(os.path.join(ROOT, "tests", "golden", "obs_synthetic.csv"))
    obs = Observations.from_years(1750.0 + np.arange(n_steps), y, T, s, baseline=(1900, 1950))
    legs = [("config3 1M fp64", 1_000_000, torch.float64, "per_step", "multigas"),
            ("config3 1M fp64", 1_000_000, torch.float64, "fused", "multigas"),
            ("config5 12.5M fp32", 12_500_000, torch.float32, "fused", "multigas"),
            ("co2-only 12.5M fp32", 12_500_000, torch.float32, "fused", "co2")]
    print(f"# {torch.cuda.get_device_name(0)}; {n_steps} steps, observation window {obs.window} ({obs.n_obs} observed); "
          f"median of {a.repeats} alternating runs each; no stored rows")
    for name, N, dt, mode, kind in legs:
        if a.quick:
            N = 20_000
        base = prm.default_params(kind)
        E = emissions.rcp_like_emissions(n_steps, 3 if kind == "multigas" else 1)
        p = prm.sample_ensemble_shard(base, N, 0, N, device="cuda:0", dtype=dt)
        engs = {k: EnsembleEngine(p, N, E, dtype=dt, store_trajectory=False, observations=o, device="cuda:0")
                for k, o in (("plain", None), ("misfit", obs))}
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
        ratio = med["misfit"] / med["plain"]
        line = (f"{name:20s} {mode:9s} plain {med['plain'] * 1e3:9.2f} ms  misfit {med['misfit'] * 1e3:9.2f} ms  "
                f"ratio {ratio:.4f}  (runs plain {[round(v * 1e3, 2) for v in times['plain']]}, "
                f"misfit {[round(v * 1e3, 2) for v in times['misfit']]})")
        if mode == "per_step":
            pred = engs["misfit"].bytes_per_member_step("per_step") / engs["plain"].bytes_per_member_step("per_step")
            line += f"  bytes_per_member_step predicts {pred:.4f}"
        print(line, flush=True)
        for e in engs.values():
            e.close()
        del engs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
