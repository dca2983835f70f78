#!/usr/bin/env python3
"""A/B of the scenario axis against single-scenario engines, in ONE process, alternating the legs.

    python tools/scenario_ab.py [--repeats R] [--quick]

Legs (three gases, fp64, 750 steps, no stored rows):
  bandwidth-bound, mode per_step: 1M parameter members x S = 4 scenarios against ONE single-scenario engine of 4M members
      (the same state bytes); reported per member-scenario-step next to the ratio bytes_per_member_step predicts;
  launch-bound, mode auto: 10k members x S = 8 against eight single-scenario engines of 10k members, each in its own 'auto'
      mode, run back to back.
Prints one line per leg: median wall time per run of each side, the ratio, the modes 'auto' resolved to."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fiveeqscm_amd import emissions  # noqa: E402
from fiveeqscm_amd import params as prm  # noqa: E402
from fiveeqscm_amd.engine import EnsembleEngine  # noqa: E402


def scenarios(n_steps, S, t_branch=250):
    base = emissions.rcp_like_emissions(n_steps, 3)
    E = np.repeat(base[None], S, axis=0)
    for s in range(S):
        E[s, t_branch:, 0] *= 0.5 + s / max(S - 1, 1)          # future CO2 low ... high
    return E


def timed(fn, repeats, sides):
    times = {k: [] for k in sides}
    for _ in range(repeats):
        for k in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(k)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="small members, for a dry run of the script")
    a = ap.parse_args()
    n_steps = 750
    base = prm.default_params("multigas")
    print(f"# {torch.cuda.get_device_name(0)}; {n_steps} steps, three gases, fp64, no stored rows; median of {a.repeats} "
          "alternating runs each")

    # -- bandwidth-bound: 1M x 4 scenarios vs 4M x 1 -------------------------------------------------------------
    N, S = (20_000, 4) if a.quick else (1_000_000, 4)
    E = scenarios(n_steps, S)
    p1 = prm.sample_ensemble_shard(base, N, 0, N, device="cuda:0")
    p4 = prm.sample_ensemble_shard(base, S * N, 0, S * N, device="cuda:0")
    engs = {"scen": EnsembleEngine(p1, N, E, store_trajectory=False, device="cuda:0"),
            "single": EnsembleEngine(p4, S * N, E[0], store_trajectory=False, device="cuda:0")}
    for e in engs.values():
        e.run(mode="per_step")

    def run_bw(k):
        engs[k].reset_state()
        engs[k].run(mode="per_step")

    t = timed(run_bw, a.repeats, engs)
    med = {k: float(np.median(v)) for k, v in t.items()}
    per = {k: med[k] / (S * N * n_steps) for k in med}                 # per member-scenario-step (4M either way)
    pred = engs["scen"].bytes_per_member_step("per_step") / engs["single"].bytes_per_member_step("per_step")
    print(f"bandwidth per_step  {N} x S={S} {med['scen'] * 1e3:9.2f} ms ({per['scen'] * 1e12:7.2f} ps per member-scenario-step)"
          f"  vs {S * N} x 1 {med['single'] * 1e3:9.2f} ms ({per['single'] * 1e12:7.2f} ps)  ratio {med['scen'] / med['single']:.4f}"
          f"  bytes_per_member_step predicts {pred:.4f}  chunks {len(engs['scen']._chunks())} / {len(engs['single']._chunks())}"
          f"  streams {engs['scen'].per_step_streams} / {engs['single'].per_step_streams}"
          f"  (runs scen {[round(v * 1e3, 2) for v in t['scen']]}, single {[round(v * 1e3, 2) for v in t['single']]})",
          flush=True)
    for e in engs.values():
        e.close()
    del engs
    torch.cuda.empty_cache()

    # -- launch-bound: 10k x 8 scenarios in one engine vs eight engines ------------------------------------------
    N, S = 10_000, 8
    E = scenarios(n_steps, S)
    p = prm.sample_ensemble_shard(base, N, 0, N, device="cuda:0")
    scen = EnsembleEngine(p, N, E, store_trajectory=False, device="cuda:0")
    singles = [EnsembleEngine(p, N, E[s], store_trajectory=False, device="cuda:0") for s in range(S)]
    scen.run(mode="auto")
    for e in singles:
        e.run(mode="auto")

    def run_lb(k):
        for e in ([scen] if k == "scen" else singles):
            e.reset_state()
        for e in ([scen] if k == "scen" else singles):
            e.run(mode="auto")

    t = timed(run_lb, a.repeats, ("scen", "singles"))
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(f"launch-bound auto   {N} x S={S} {med['scen'] * 1e3:9.2f} ms (auto -> {scen.last_mode})  vs {S} x {N} back to back "
          f"{med['singles'] * 1e3:9.2f} ms (auto -> {singles[0].last_mode})  ratio {med['scen'] / med['singles']:.4f}"
          f"  (runs scen {[round(v * 1e3, 2) for v in t['scen']]}, singles {[round(v * 1e3, 2) for v in t['singles']]})",
          flush=True)
    for e in [scen] + singles:
        e.close()


if __name__ == "__main__":
    main()
