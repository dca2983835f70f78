"""Cost of the running-mean and trend passes on the MI355X against the library's own plain copy moving the same bytes (the rows
read once plus the outputs written).  Events on the stream, warm-up, the median of repeats and their spread; the passes and the
copy alternate.  --out FILE also writes the result as JSON (kept as profiles/r27/smooth_timing.json).

    python tools/smooth_timing.py [--members N] [--rows K] [--out FILE]
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
    ap.add_argument("--rows", type=int, default=251)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    N, K = a.members, a.rows
    lib = _capi.load()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())              # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    result = {"device": torch.cuda.get_device_name(0), "members": N, "rows": K, "cases": []}
    # the copy's buffers: sized per case to the bytes the pass moves (read + written), half each way
    pool = torch.ones((K * N * 8 + 8 * N * 8) // 8 + 16, dtype=torch.float64, device="cuda")
    pool_dst = torch.empty_like(pool)
    steps = torch.arange(K, dtype=torch.int32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    for dtype, w in ((torch.float64, 8), (torch.float32, 4)):
        T = (torch.rand((K, N), generator=g, device="cuda", dtype=torch.float32) * 3.0).to(dtype)
        cases = [("running_mean", window) for window in (5, 20, 32)] + [("window_trends", 4)]
        for what, arg in cases:
            if what == "running_mean":
                n_out = K - arg + 1
                out = torch.empty((n_out, N), dtype=torch.float64, device="cuda")
                fn = lib.fiveeq_running_mean_f64 if w == 8 else lib.fiveeq_running_mean_f32
                call = lambda: _capi.check(lib, fn(1, K, N, N, ptr(T), K * N, arg, 0, None, 0, ptr(out), n_out * N, stream))   # noqa: E731
                moved = K * N * w + n_out * N * 8
            else:
                wn = (ctypes.c_int32 * 8)(0, K, K // 4, K // 2, K // 2, K, 10, 50)
                out = torch.empty((2 * arg, N), dtype=torch.float64, device="cuda")
                fn = lib.fiveeq_window_trends_f64 if w == 8 else lib.fiveeq_window_trends_f32
                call = lambda: _capi.check(lib, fn(1, K, N, N, ptr(T), K * N, ptr(steps), arg, ctypes.cast(wn, ctypes.c_void_p), ptr(out), 1,   # noqa: E731
                                                   stream))
                moved = K * N * w + 2 * arg * N * 8
            n_copy = moved // 32 * 2                           # fp64 elements each way (even): the same bytes in all
            copy = lambda: _capi.check(lib, lib.fiveeq_stream_copy_wide_f64(n_copy, ptr(pool), ptr(pool_dst), stream))   # noqa: E731
            t_pass, t_copy = [], []
            for _ in range(3):                                 # alternate: three windows of each
                t_pass.append(timed(call))
                t_copy.append(timed(copy))
            ms, spread = min(t_pass)[0] * 1e3, max(s for _, s in t_pass)
            ms_copy, spread_copy = min(t_copy)[0] * 1e3, max(s for _, s in t_copy)
            case = {"pass": what, "dtype": "fp64" if w == 8 else "fp32", "window_or_windows": arg, "bytes": moved, "ms": ms, "spread": spread,
                    "tb_per_s": moved / ms / 1e9, "copy_ms": ms_copy, "copy_spread": spread_copy, "copy_tb_per_s": 2 * n_copy * 8 / ms_copy / 1e9,
                    "ratio_to_copy": ms_copy / ms}
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
            del out
        del T
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
