"""Cost of the minor-gas forcing rows (fiveeq_minor_rows_*) on the MI355X beside the AR(1) noise pass (fiveeq_noise_rows_*) on the
same rows, and against a traffic model.  Events on the stream, warm-up, the median of repeats and their spread; the two passes
alternate.  --out FILE also writes the result as JSON (kept as profiles/r29/minor_rows_timing.json).

    python tools/minor_rows_timing.py [--members N] [--rows K] [--out FILE]

K species go in consecutive groups of 8, as minor_gases.minor_gas_rows calls them: the first group writes the rows, the later
ones add onto them.  The traffic model: n_rows n w bytes written per group, the same again read by every accumulating group,
plus 2 K n w bytes of parameters (the fp64 state R, 16 K n bytes, and the emission table are left out of it).
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

GROUP = 8


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
    K_max = 40
    E = torch.rand((n_rows, K_max), generator=g, device="cuda", dtype=torch.float64) + 0.5
    c = (ctypes.c_double * K_max)(*([0.1] * K_max))
    for dtype, w, sfx in ((torch.float64, 8, "f64"), (torch.float32, 4, "f32")):
        rows = torch.empty((n_rows, N), dtype=dtype, device="cuda")
        tau = (torch.rand((K_max, N), generator=g, device="cuda", dtype=torch.float32) * 200.0 + 1.0).to(dtype)
        eff = (torch.rand((K_max, N), generator=g, device="cuda", dtype=torch.float32) * 0.5).to(dtype)
        R = torch.zeros((K_max, N), dtype=torch.float64, device="cuda")
        phi = torch.full((N,), 0.6, dtype=dtype, device="cuda")
        s = torch.full((N,), 0.4, dtype=dtype, device="cuda")
        xi = torch.zeros(N, dtype=torch.float64, device="cuda")
        minor, noise_fn = getattr(lib, "fiveeq_minor_rows_" + sfx), getattr(lib, "fiveeq_noise_rows_" + sfx)
        noise = lambda: _capi.check(lib, noise_fn(1, 0, N, N, 0, n_rows, ptr(phi), ptr(s), ptr(xi), ptr(rows), stream))   # noqa: E731
        for K in (8, 40):
            groups = [(k0, min(k0 + GROUP, K)) for k0 in range(0, K, GROUP)]
            tables = [E[:, k0:k1].contiguous() for k0, k1 in groups]

            def call():
                for i, (k0, k1) in enumerate(groups):
                    c_g = ctypes.cast(ctypes.byref(c, 8 * k0), ctypes.c_void_p)
                    _capi.check(lib, minor(k1 - k0, N, N, n_rows, 1.0, c_g, ptr(tables[i]), ptr(tau[k0:k1]), ptr(eff[k0:k1]),
                                           ptr(R[k0:k1]), ptr(rows), int(i > 0), stream))
            model = n_rows * N * w * (2 * len(groups) - 1) + 2 * K * N * w
            t_pass, t_noise = [], []
            for _ in range(3):                                 # alternate: three windows of each
                R.zero_()
                t_pass.append(timed(call))
                t_noise.append(timed(noise))
            ms, spread = min(t_pass)[0] * 1e3, max(v for _, v in t_pass)
            ms_noise, spread_noise = min(t_noise)[0] * 1e3, max(v for _, v in t_noise)
            case = {"pass": "minor_rows", "dtype": "fp64" if w == 8 else "fp32", "species": K, "calls": len(groups), "model_bytes": model,
                    "ms": ms, "spread": spread, "model_tb_per_s": model / ms / 1e9, "noise_ms": ms_noise, "noise_spread": spread_noise,
                    "noise_tb_per_s": n_rows * N * w / ms_noise / 1e9, "ratio_to_noise": ms / ms_noise,
                    "ns_per_member_row_species": ms * 1e6 / (n_rows * N * K)}
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
        del rows, tau, eff, R
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
