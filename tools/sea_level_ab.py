"""Cost of the sea-level rows (fiveeq_sea_level_rows_*) on the MI355X beside the project's stream-copy yardstick measured in the
same session.  Events on the stream, warm-up, the median of repeats and their spread; the pass and the copy alternate.
--out FILE also writes the result as JSON (kept as profiles/r31/sea_level_ab.json).

    python tools/sea_level_ab.py [--members N] [--rows K] [--components J] [--out FILE]

Algorithmic bytes of a pass: the T rows in (n_rows n w) plus total out (n_rows n 8) plus, where asked for, the component rows
(n_rows n J 8); the parameters and the state (8 (6 J + 1) n) are left out.  The yardstick: fiveeq_stream_copy_f64 (8 bytes per
lane, the access shape of this pass) over a buffer of the T rows' size, 16 bytes moved per element; fiveeq_stream_copy_nt_f64
(the fastest plain copy of the box) is reported beside it.
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
    ap.add_argument("--components", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    N, n_rows, J = a.members, a.rows, a.components
    lib = _capi.load()
    ptr = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())                 # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    result = {"device": torch.cuda.get_device_name(0), "members": N, "rows": n_rows, "components": J, "cases": []}
    g = torch.Generator(device="cuda").manual_seed(1)
    par = torch.empty((5, J, N), dtype=torch.float64, device="cuda")
    par[0] = torch.rand((J, N), generator=g, device="cuda", dtype=torch.float64) * 300.0 + 2.0
    par[1] = torch.rand((J, N), generator=g, device="cuda", dtype=torch.float64) * 0.4
    par[2] = torch.rand((J, N), generator=g, device="cuda", dtype=torch.float64) * 0.05
    par[3] = 0.0
    par[4] = float("inf")
    par[4, 0] = 0.5                                              # one component with a cap that binds for some members
    S = torch.zeros((J, N), dtype=torch.float64, device="cuda")
    total = torch.empty((n_rows, N), dtype=torch.float64, device="cuda")
    comps = torch.empty((n_rows, J, N), dtype=torch.float64, device="cuda")
    T64 = torch.rand((n_rows, N), generator=g, device="cuda", dtype=torch.float64) * 3.0
    n_copy = n_rows * N - (n_rows * N) % 1024
    copy = lambda: _capi.check(lib, lib.fiveeq_stream_copy_f64(n_copy, ptr(T64), ptr(total), stream))        # noqa: E731
    copy_nt = lambda: _capi.check(lib, lib.fiveeq_stream_copy_nt_f64(n_copy, ptr(T64), ptr(total), stream))  # noqa: E731
    rate_mask = 0b10 if J > 1 else 0
    for dtype, w, sfx in ((torch.float64, 8, "f64"), (torch.float32, 4, "f32")):
        T = T64 if w == 8 else T64.to(dtype)
        fn = getattr(lib, "fiveeq_sea_level_rows_" + sfx)
        for with_comps in (False, True):
            def call():
                _capi.check(lib, fn(1, J, rate_mask, N, N, n_rows, 1.0, ptr(T), N, n_rows * N, ptr(par), None, N, N, None, ptr(S),
                                    ptr(total), ptr(comps) if with_comps else None, N, stream))
            model = n_rows * N * (w + 8 + (8 * J if with_comps else 0))
            t_pass, t_copy, t_nt = [], [], []
            for _ in range(3):                                   # alternate: three windows of each
                S.zero_()
                t_pass.append(timed(call))
                t_copy.append(timed(copy))
                t_nt.append(timed(copy_nt))
            ms, spread = min(t_pass)[0] * 1e3, max(v for _, v in t_pass)
            ms_copy, ms_nt = min(t_copy)[0] * 1e3, min(t_nt)[0] * 1e3
            tb, tb_copy, tb_nt = model / ms / 1e9, 16 * n_copy / ms_copy / 1e9, 16 * n_copy / ms_nt / 1e9
            case = {"pass": "sea_level_rows", "T_rows": "fp64" if w == 8 else "fp32", "component_rows": with_comps, "model_bytes": model,
                    "ms": ms, "spread": spread, "model_tb_per_s": tb, "copy_ms": ms_copy, "copy_tb_per_s": tb_copy,
                    "copy_spread": max(v for _, v in t_copy), "copy_nt_tb_per_s": tb_nt, "fraction_of_copy": tb / tb_copy,
                    "fraction_of_copy_nt": tb / tb_nt}
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
