#!/usr/bin/env python3
"""A/B of the forcing scales under the scenario axis, in ONE process, alternating the sides, warm, the same members on
every side.

    python tools/scenario_forcing_ab.py [--repeats R] [--quick]

Sides (three gases, fp64, 750 steps, K = 2 categories, no stored rows):
  scen_forc    one scenario engine with forcing=ScenarioForcings                       (a) the new form
  singles_forc S single-scenario forcing= engines of the same members, back to back    (b) what the parent commit offers
  scen_plain / singles_plain   the same two without forcing=: the plain scenario kernel's own ratio, in the same process
Legs: 1M members x S = 4 in mode per_step and in mode fused; 10k members x S = 8 in mode auto (launch-bound).
Per leg one line with the medians, per member-scenario-step times, the ratios (a) / (b) and plain / plain, the ratio
bytes_per_member_step predicts (c), and every raw run.  The last line says whether the forcing form's ratio is no worse
than the plain form's."""
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
from fiveeqscm_amd.forcing import ScenarioForcings  # noqa: E402

SIDES = ("scen_forc", "singles_forc", "scen_plain", "singles_plain")


def inputs(n_steps, S, t_branch=250):
    """S scenarios (future CO2 low ... high), an aerosol table proportional to each scenario's CO2 emissions and volcanic
    spikes."""
    base = emissions.rcp_like_emissions(n_steps, 3)
    E = np.repeat(base[None], S, axis=0)
    for s in range(S):
        E[s, t_branch:, 0] *= 0.5 + s / max(S - 1, 1)
    tt = np.arange(n_steps)
    tabs = np.stack([np.stack([-1.1 * E[s, :, 0] / base[:, 0].max(), np.where(tt % 37 == 5, -2.5, 0.0)], 1) for s in range(S)])
    return E, ScenarioForcings(tabs, ("aerosol", "volcanic"))


def engines(p, N, E, sf):
    """{side: [engines]}: the same parameter members on every side, the scale rows on the forcing sides."""
    S = E.shape[0]
    plain = {k: v for k, v in p.items() if k not in ("f_scale", "fx_scale")}
    kw = dict(store_trajectory=False, device="cuda:0")
    return {"scen_forc": [EnsembleEngine(p, N, E, forcing=sf, **kw)],
            "singles_forc": [EnsembleEngine(p, N, E[s], forcing=sf.scenario(s), **kw) for s in range(S)],
            "scen_plain": [EnsembleEngine(plain, N, E, **kw)],
            "singles_plain": [EnsembleEngine(plain, N, E[s], **kw) for s in range(S)]}


def leg(name, engs, mode, repeats, N, S, n_steps):
    def run(side):
        for e in engs[side]:
            e.reset_state()
        for e in engs[side]:
            e.run(mode=mode)

    for side in SIDES:                                              # warm: plans, streams, the caches
        run(side)
    times = {k: [] for k in SIDES}
    for _ in range(repeats):
        for side in SIDES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(side)
            torch.cuda.synchronize()
            times[side].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) for k, v in times.items()}
    ps = {k: med[k] / (S * N * n_steps) * 1e12 for k in med}       # per member-scenario-step
    r_forc, r_plain = med["scen_forc"] / med["singles_forc"], med["scen_plain"] / med["singles_plain"]
    bm = "per_step" if mode == "auto" else mode
    pred = {k: engs["scen_" + k][0].bytes_per_member_step(bm) / engs["singles_" + k][0].bytes_per_member_step(bm)
            for k in ("forc", "plain")}
    modes = {k: engs[k][0].last_mode for k in SIDES}
    print(f"{name} {N} x S={S} mode {mode}:", flush=True)
    for k in SIDES:
        print(f"   {name}.{k:14s} median {med[k] * 1e3:9.3f} ms  {ps[k]:8.2f} ps per member-scenario-step  (-> {modes[k]})  runs ms "
              f"{[round(v * 1e3, 3) for v in times[k]]}")
    print(f"   {name}.ratio_forc  {r_forc:.4f}  (a) / (b);  bytes_per_member_step predicts {pred['forc']:.4f}  (c)")
    print(f"   {name}.ratio_plain {r_plain:.4f}  plain scenario engine / plain singles;  predicts {pred['plain']:.4f}")
    print(f"   {name}.forc_over_plain {r_forc / r_plain:.4f}  (<= 1: the forcing form's ratio is no worse than the plain form's)",
          flush=True)
    return r_forc, r_plain


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="few members, for a dry run of the script")
    a = ap.parse_args()
    n_steps, K = 750, 2
    base = prm.default_params("multigas")
    print(f"# {torch.cuda.get_device_name(0)}; {n_steps} steps, three gases, fp64, K = {K}, no stored rows; median of "
          f"{a.repeats} alternating warm runs per side")
    out = {}
    for name, N, S, modes in (("bandwidth", 20_000 if a.quick else 1_000_000, 4, ("per_step", "fused")),
                              ("launch_bound", 10_000, 8, ("auto",))):
        E, sf = inputs(n_steps, S)
        p = prm.sample_ensemble_shard(base, N, 0, N, device="cuda:0")
        sc = prm.sample_forcing_scales(base, N, 0, N, [(0.8, 1.2)] * 3 + [(0.3, 2.0), (0.5, 1.5)], device="cuda:0")
        p["f_scale"], p["fx_scale"] = sc[:3], sc[3:]
        engs = engines(p, N, E, sf)
        for mode in modes:
            out[f"{name}_{mode}"] = leg(f"{name}_{mode}", engs, mode, a.repeats, N, S, n_steps)
        for es in engs.values():
            for e in es:
                e.close()
        del engs
        torch.cuda.empty_cache()
    worse = [k for k, (rf, rp) in out.items() if rf > rp]
    print("expectation (the forcing form's ratio to (b) is no worse than the plain scenario form's ratio): "
          + ("CONFIRMED in every leg" if not worse else f"REFUTED in {worse}"))


if __name__ == "__main__":
    main()
