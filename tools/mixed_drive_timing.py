#!/usr/bin/env python3
"""Cost of a mixed-drive step (mask 0b110: CO2 emission-driven, CH4 and N2O concentration-driven) against its two parents, the
plain inverse run (fiveeq_run_inverse_*) and the plain time-fused forward run (fiveeq_run_fused_*), profiles/r26/NOTES.md: the
same 4 + 1 + 1 ensemble, the same series, one time-fused launch per run, one stored row.

    python tools/mixed_drive_timing.py [--members 1000000] [--steps 750] [--rounds 7] [--reps 2] [--out FILE.json]

Per precision the three forms are timed in alternation (`rounds` times inverse, mixed, forward), each window `reps` runs between
two device events after one warm-up run of every form; the figure of a form is the median of its windows, the spread
(max - min) / median is printed beside it.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fiveeqscm_amd import emissions, params as prm                    # noqa: E402
from fiveeqscm_amd.engine import EnsembleEngine, MixedDriveEngine     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=750)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, n = a.members, a.steps
    base = prm.default_params("multigas")                             # pools 4 + 1 + 1
    p = prm.sample_ensemble_shard(base, N)
    t = np.arange(n)
    C0 = np.asarray(base["PI_conc"], dtype=np.float64)
    target = C0[None, :] * (1.0 + np.array([0.5, 1.2, 0.2])[None, :] * (t[:, None] / n) ** 2)
    E = emissions.rcp_like_emissions(n, 3)
    result = {"members": N, "steps": n, "layout": "4+1+1", "mask": "0b110", "rounds": a.rounds, "reps": a.reps, "forms": {}}
    for dtype, prec in ((torch.float64, "f64"), (torch.float32, "f32")):
        kw = dict(dtype=dtype, device="cuda:0", output_steps=[n - 1], fused_span=None)
        engines = {
            "inverse": (EnsembleEngine(p, N, target, concentration_driven=True, **kw), {}),
            "mixed 0b110": (MixedDriveEngine(p, N, E, target, (1, 2), **kw), {}),
            "forward fused": (EnsembleEngine(p, N, E, **kw), {"mode": "fused"}),
        }
        for eng, run_kw in engines.values():                           # warm-up: every form once
            eng.run(**run_kw)
        torch.cuda.synchronize()
        times = {k: [] for k in engines}
        for _ in range(a.rounds):
            for name, (eng, run_kw) in engines.items():
                eng.reset_state()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    eng.run(**run_kw)
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / a.reps)
        med = {k: float(np.median(v)) for k, v in times.items()}
        for name, v in times.items():
            entry = {"ms_per_run": med[name], "us_per_step": med[name] * 1e3 / n, "spread": float((max(v) - min(v)) / med[name]),
                     "ratio_to_inverse": med[name] / med["inverse"]}
            result["forms"][f"{prec} {name}"] = entry
            print(f"{prec} {name:14s} {med[name]:9.3f} ms per run  {entry['us_per_step']:7.3f} us per step  spread "
                  f"{entry['spread']:.3f}  x inverse {entry['ratio_to_inverse']:.3f}")
        for eng, _ in engines.values():
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
