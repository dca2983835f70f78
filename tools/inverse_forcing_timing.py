#!/usr/bin/env python3
"""Cost of the concentration-driven forms with forcing scales and / or the in-loop misfit against the plain inverse run
(profiles/r24/NOTES.md): the same ensemble, the same 250-step target series, one time-fused launch per run.

    python tools/inverse_forcing_timing.py [--members 1000000] [--steps 250] [--rounds 7] [--reps 4] [--out FILE.json]

Per precision the four forms are timed in alternation (`rounds` times plain, misfit, forc, forc+misfit), each window `reps` runs
between two device events after one warm-up run of every form; the figure of a form is the median of its windows, the spread
(max - min) / median is printed beside it.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fiveeqscm_amd import constrain, params as prm                     # noqa: E402
from fiveeqscm_amd.engine import ConcentrationDrivenEngine, EnsembleEngine   # noqa: E402
from fiveeqscm_amd.forcing import ExternalForcings                     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, n = a.members, a.steps
    base = prm.default_params("multigas")                             # pools 4 + 1 + 1
    p = prm.sample_ensemble_shard(base, N)
    s = prm.sample_forcing_scales(base, N, ranges=[(0.75, 1.25)] * 3 + [(0.25, 2.0)] * 3, seed=7)
    ps = dict(p, f_scale=s[:3], fx_scale=s[3:])
    t = np.arange(n)
    C0 = np.asarray(base["PI_conc"], dtype=np.float64)
    target = C0[None, :] * (1.0 + np.array([0.5, 1.2, 0.2])[None, :] * (t[:, None] / n) ** 2)
    fx = ExternalForcings(np.stack([-0.9 * t / n, np.where(t % 37 == 5, -2.5, 0.0), 0.1 * np.sin(2 * np.pi * t / 11.0)], 1))
    at = t[t >= 100].astype(float)
    obs = constrain.Observations.from_years(t.astype(float), at, 0.004 * (at - 100.0), 0.1, (100.0, 130.0))
    result = {"members": N, "steps": n, "layout": "4+1+1", "rounds": a.rounds, "reps": a.reps, "forms": {}}
    for dtype, prec in ((torch.float64, "f64"), (torch.float32, "f32")):
        kw = dict(dtype=dtype, device="cuda:0", output_steps=[n - 1])
        engines = {
            "plain": EnsembleEngine(p, N, target, concentration_driven=True, **kw),
            "misfit": ConcentrationDrivenEngine(p, N, target, observations=obs, **kw),
            "forc": ConcentrationDrivenEngine(ps, N, target, forcing=fx, **kw),
            "forc+misfit": ConcentrationDrivenEngine(ps, N, target, forcing=fx, observations=obs, **kw),
        }
        for eng in engines.values():                                   # warm-up: every form once
            eng.run()
        torch.cuda.synchronize()
        times = {k: [] for k in engines}
        for _ in range(a.rounds):
            for name, eng in engines.items():
                eng.reset_state()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    eng.run()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / a.reps)
        med = {k: float(np.median(v)) for k, v in times.items()}
        for name, v in times.items():
            result["forms"][f"{prec} {name}"] = {"ms_per_run": med[name], "spread": float((max(v) - min(v)) / med[name]),
                                                 "ratio_to_plain": med[name] / med["plain"],
                                                 "ns_per_member_step": med[name] * 1e6 / (N * n)}
            print(f"{prec} {name:12s} {med[name]:9.3f} ms per run  spread {result['forms'][f'{prec} {name}']['spread']:.3f}  "
                  f"x plain {med[name] / med['plain']:.3f}")
        for eng in engines.values():
            eng.close()
        del engines
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
