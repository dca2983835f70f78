#!/usr/bin/env python3
"""Warm time of the WEIGHTED end-of-run summary (distributed.gather_weighted_summary) against the unweighted one
(gather_summary) on the same rows, one GPU, and the device time of each weighted pass (HIP events around the C-ABI calls).

    python tools/weighted_summary_timing.py [--members N] [--rows K] [--dtype f64|f32] [--zero-fraction F]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fiveeqscm_amd import distributed as D  # noqa: E402
from fiveeqscm_amd.constrain import W_ONE  # noqa: E402


def warm_ms(fn, repeats=5):
    fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


class TimedLib:
    """The library with a pair of HIP events around every pass: name -> list of device milliseconds."""

    def __init__(self, lib):
        self.lib, self.ms, self.pending = lib, {}, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith(("fiveeq_wrow_moments_f", "fiveeq_whist", "fiveeq_wselect")):
            return fn

        def timed(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*a)
            e1.record()
            self.pending.append((name, e0, e1))
            return rc
        return timed

    def collect(self):
        torch.cuda.synchronize()
        for name, e0, e1 in self.pending:
            self.ms.setdefault(name, []).append(e0.elapsed_time(e1))
        self.pending = []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=1_000_000)
    ap.add_argument("--rows", type=int, default=3)
    ap.add_argument("--dtype", choices=("f64", "f32"), default="f64")
    ap.add_argument("--zero-fraction", type=float, default=0.5, help="share of members of weight 0")
    a = ap.parse_args()
    dt = torch.float64 if a.dtype == "f64" else torch.float32
    g = torch.Generator(device="cuda:0").manual_seed(1)
    x = torch.randn((a.rows, a.members), device="cuda:0", dtype=dt, generator=g) * 0.7 + 2.0
    rng = np.random.default_rng(2)
    w = rng.integers(1, W_ONE + 1, size=a.members, dtype=np.int64)
    w[rng.uniform(size=a.members) < a.zero_fraction] = 0
    wd = torch.from_numpy(w).to("cuda:0")
    pct = (5.0, 50.0, 95.0)
    plain = warm_ms(lambda: D.gather_summary(x, pct))
    weighted = warm_ms(lambda: D.gather_weighted_summary(x, wd, pct))
    print(f"{a.members} members x {a.rows} rows {a.dtype}, {a.zero_fraction:.2f} of the weights zero, percentiles {pct}")
    print(f"  gather_summary (unweighted, warm)          {plain:8.3f} ms")
    print(f"  gather_weighted_summary (warm)             {weighted:8.3f} ms   ratio {weighted / plain:.2f}")
    real = D._lib_and_stream
    lib, capi, ct, st = real(x)
    timed = TimedLib(lib)
    D._lib_and_stream = lambda rows: (timed, capi, ct, st)
    try:
        for _ in range(5):
            s = D.gather_weighted_summary(x, wd, pct)
            timed.collect()
    finally:
        D._lib_and_stream = real
    for name, ms in timed.ms.items():
        print(f"  {name:32s} {min(ms) * 1e3:8.1f} us (device, best of {len(ms)})")
    print(f"  ess {s['ess']:.1f} of {int(s['count'][0])} weighted members; median {s['percentiles'][0, 1]:.6f}")


if __name__ == "__main__":
    main()
