#!/usr/bin/env python3
"""Time the pulse-response pass (EnsembleEngine.pulse_response: one HIP kernel over the stored rows) against the composition
the package offered before it: 1 + P calls of forcing_rows(want=("F",)), the torch subtractions, cumsum over the rows and the
picks of the horizon rows.  Both give I_F, I_T, I_C, dT, dC [P, H, N] from the same stored rows of one scenario engine.

Device events around each call, `--warmup` untimed calls of each path, then the two paths alternating, the median of
`--repeats` each.  The default size (1M fp64 members x 3
gases x 100 rows x 3 pulses: 12.8 GB of rows) streams from HBM in every call; `--members 8192` (105 MB of rows) shows the same
two paths on rows that stay in the 256 MiB Infinity Cache between calls.  Prints one line per path and the ratio; --out
appends them to a file.  Needs an MI355X.

    python tools/pulse_response_timing.py [--members N] [--rows K] [--dtype f64|f32] [--warmup W] [--repeats R] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fiveeqscm_amd import emissions, params, pulse  # noqa: E402
from fiveeqscm_amd.engine import EnsembleEngine  # noqa: E402

SIZES = (100.0, 3000.0, 800.0)


def composition(eng, table, horizons):
    """The outputs of pulse_response from the passes of the parent commit."""
    F = [eng.forcing_rows(want=("F",), scenario=s).F.double() for s in range(eng.n_scenarios)]
    pick = torch.tensor([h - 1 for h in horizons], device=eng.device)
    out = []
    for s, g, _ in table:
        dF, dT, dC = F[s] - F[0], eng.T[s].double() - eng.T[0].double(), eng.C[s, :, g].double() - eng.C[0, :, g].double()
        out.append(torch.stack([dF.cumsum(0)[pick], dT.cumsum(0)[pick], dC.cumsum(0)[pick], dT[pick], dC[pick]]))
    return torch.stack(out, 1)


def timed(fns, warmup, repeats):
    """(median, min, max) ms of every function of `fns`, their calls alternating so that both see the same machine."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    ms = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=1_000_000)
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--dtype", choices=("f64", "f32"), default="f64")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, K = args.members, args.rows
    dtype = torch.float64 if args.dtype == "f64" else torch.float32
    w = 8 if args.dtype == "f64" else 4
    p = params.sample_ensemble_shard(params.default_params("multigas"), N)
    exp = pulse.pulse_experiment(emissions.rcp_like_emissions(K + 5, 3), 5, list(enumerate(SIZES)), K)
    eng = EnsembleEngine(p, N, exp.emissions, dtype=dtype, device="cuda:0", scenario_names=exp.scenario_names,
                         output_steps=exp.output_steps)
    eng.run(mode="per_step")
    torch.cuda.synchronize()
    horizons = tuple(sorted({max(1, K // 5), K}))
    table = [(1 + i, g, size) for i, (g, size) in enumerate(exp.pulses)]
    res = eng.pulse_response(exp, horizons)
    new = torch.stack([res.I_F, res.I_T, res.I_C, res.dT, res.dC])
    old = composition(eng, table, horizons)
    rel = float(((new - old).abs() / old.abs().clamp_min(1e-300)).max())
    t_new, t_old = timed((lambda: eng.pulse_response(exp, horizons), lambda: composition(eng, table, horizons)), args.warmup, args.repeats)
    row_bytes = (1 + len(table)) * (3 + 1) * w * N * K
    lines = [
        f"pulse response timing: {N} {args.dtype} members x 3 gases x {K} rows x {len(table)} pulses; stored rows {row_bytes / 1e9:.3f} GB "
        f"({'streamed from HBM in every call' if row_bytes > 256 * 2**20 else 'resident in the Infinity Cache after the warm-up'}); "
        f"warm-up {args.warmup}, median of {args.repeats} (min, max)",
        f"  pulse_response (one pass)        {t_new[0]:9.3f} ms ({t_new[1]:.3f}, {t_new[2]:.3f})  {row_bytes / t_new[0] / 1e9:.3f} TB/s of the rows it reads",
        f"  composition (forcing_rows+torch) {t_old[0]:9.3f} ms ({t_old[1]:.3f}, {t_old[2]:.3f})",
        f"  ratio composition / pass         {t_old[0] / t_new[0]:9.2f}",
        f"  worst relative difference of the two results {rel:.3e} (0: the same bits)",
    ]
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
