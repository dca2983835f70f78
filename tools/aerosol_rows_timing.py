"""Cost of the aerosol forcing rows (fiveeq_aerosol_rows_*) on the MI355X beside the other two generators of member_forcing rows
on the same rows: the AR(1) noise pass (fiveeq_noise_rows_*) and the minor-gas pass (fiveeq_minor_rows_*, the same number of
species).  Events on the stream, warm-up, the median of repeats and their spread; the passes alternate.  --out FILE also writes
the result as JSON (kept as profiles/r30/aerosol_rows_timing.json).

    python tools/aerosol_rows_timing.py [--members N] [--rows K] [--out FILE]

Each case times the writing call (accumulate = 0, every species in the cloud term), the accumulating call (accumulate = 1: one
more read of the rows), and the writing call without a cloud term (aci_mask = 0: no logarithm) — the last two tell the store
traffic from the logarithm.  The traffic model: n_rows n w bytes written, the same again read by an accumulating call, plus
(2 K + 1) n w bytes of parameters (the emission table is left out of it).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fiveeqscm_amd import _capi  # noqa: E402


def timed(fn, warm=2, reps=9):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    ts = np.array(ts)
    return float(np.median(ts)), float((ts.max() - ts.min()) / np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=1_000_000)
    ap.add_argument("--rows", type=int, default=750)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    N, n_rows = a.members, a.rows
    lib = _capi.load()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())              # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    result = {"device": torch.cuda.get_device_name(0), "members": N, "rows": n_rows, "cases": []}
    g = torch.Generator(device="cuda").manual_seed(1)
    K_max = 8
    E = torch.rand((n_rows, K_max), generator=g, device="cuda", dtype=torch.float64) * 50.0 + 0.5
    base = (ctypes.c_double * K_max)(*([0.25] * K_max))
    c = (ctypes.c_double * K_max)(*([0.1] * K_max))
    for dtype, w, sfx in ((torch.float64, 8, "f64"), (torch.float32, 4, "f32")):
        rows = torch.zeros((n_rows, N), dtype=dtype, device="cuda")
        ari = (-torch.rand((K_max, N), generator=g, device="cuda", dtype=torch.float32) * 0.01).to(dtype)
        shape = (torch.rand((K_max, N), generator=g, device="cuda", dtype=torch.float32) * 100.0 + 5.0).to(dtype)
        beta = (torch.rand(N, generator=g, device="cuda", dtype=torch.float32) + 0.3).to(dtype)
        tau = (torch.rand((K_max, N), generator=g, device="cuda", dtype=torch.float32) * 200.0 + 1.0).to(dtype)
        eff = (torch.rand((K_max, N), generator=g, device="cuda", dtype=torch.float32) * 0.5).to(dtype)
        R = torch.zeros((K_max, N), dtype=torch.float64, device="cuda")
        phi = torch.full((N,), 0.6, dtype=dtype, device="cuda")
        s = torch.full((N,), 0.4, dtype=dtype, device="cuda")
        xi = torch.zeros(N, dtype=torch.float64, device="cuda")
        aer, minor_fn, noise_fn = (getattr(lib, f"fiveeq_{name}_rows_{sfx}") for name in ("aerosol", "minor", "noise"))
        noise = lambda: _capi.check(lib, noise_fn(1, 0, N, N, 0, n_rows, ptr(phi), ptr(s), ptr(xi), ptr(rows), stream))   # noqa: E731
        for K in (3, 8):
            table = E[:, :K].contiguous()

            def aerosol(mask, acc):
                return lambda: _capi.check(lib, aer(K, mask, N, N, n_rows, ctypes.cast(base, ctypes.c_void_p), ptr(table), ptr(ari),
                                                    ptr(shape), ptr(beta), ptr(rows), acc, stream))
            minor = lambda: _capi.check(lib, minor_fn(K, N, N, n_rows, 1.0, ctypes.cast(c, ctypes.c_void_p), ptr(table), ptr(tau),   # noqa: E731
                                                      ptr(eff), ptr(R), ptr(rows), 0, stream))
            passes = {"aerosol": aerosol((1 << K) - 1, 0), "aerosol_accumulate": aerosol((1 << K) - 1, 1),
                      "aerosol_no_cloud": aerosol(0, 0), "noise": noise, "minor": minor}
            times = {name: [] for name in passes}
            for _ in range(3):                                 # alternate: three windows of each
                R.zero_()
                rows.zero_()
                for name, fn in passes.items():
                    times[name].append(timed(fn))
            ms = {name: min(v)[0] * 1e3 for name, v in times.items()}
            spread = {name: max(sp for _, sp in v) for name, v in times.items()}
            model = n_rows * N * w + (2 * K + 1) * N * w
            case = {"pass": "aerosol_rows", "dtype": "fp64" if w == 8 else "fp32", "species": K, "model_bytes": model, "ms": ms,
                    "spread": spread, "model_tb_per_s": model / ms["aerosol"] / 1e9,
                    "accumulate_model_tb_per_s": (model + n_rows * N * w) / ms["aerosol_accumulate"] / 1e9,
                    "ratio_to_noise": ms["aerosol"] / ms["noise"], "ratio_to_minor": ms["aerosol"] / ms["minor"],
                    "accumulate_ratio_to_write": ms["aerosol_accumulate"] / ms["aerosol"],
                    "no_cloud_ratio_to_write": ms["aerosol_no_cloud"] / ms["aerosol"],
                    "ns_per_member_row": ms["aerosol"] * 1e6 / (n_rows * N)}
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
        del rows, ari, shape, beta, tau, eff, R
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
