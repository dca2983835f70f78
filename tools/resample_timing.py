#!/usr/bin/env python3
"""Cost of resampling on the MI355X: scan + pick + gather of 19 fp64 rows through the HIP kernels (fiveeq_wscan,
fiveeq_resample_pick, fiveeq_gather_rows_f64), beside the same work composed from torch.cumsum, torch.searchsorted and
index_select on the same card.  Warm, event-timed repeats, the two sides ALTERNATING call by call; both write into buffers
allocated before the timed window (torch through out=; only the temporaries of its position arithmetic are allocated inside);
the two results are compared bit for bit before anything is timed.

    python tools/resample_timing.py [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fiveeqscm_amd import _capi  # noqa: E402
from fiveeqscm_amd.constrain import W_ONE, resample_plan  # noqa: E402

N_ROWS, WARM, REPS = 19, 5, 30


def timed(*fns):
    """per function: median and spread (min, max) of REPS event-timed calls after WARM warm ones, in microseconds; several
    functions are called in turn, one call each per round"""
    for _ in range(WARM):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(REPS):
        for fn, t in zip(fns, ts):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b) * 1e3)
    out = [(statistics.median(t), min(t), max(t)) for t in ts]
    return out[0] if len(fns) == 1 else out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    lib = _capi.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    lines = [f"# resampling cost, {torch.cuda.get_device_name(0)}; {N_ROWS} fp64 rows; median (min .. max) of {REPS} event-timed "
             f"calls after {WARM} warm ones, microseconds",
             "# hip = fiveeq_wscan + fiveeq_resample_pick + fiveeq_gather_rows_f64; torch = cumsum + position arithmetic + "
             "searchsorted(right=True) + index_select"]
    lines.append("# hip and torch alternate call by call; the parts of each side alternate with their counterparts")
    for N in (1_000_000, 12_500_000):
        g = torch.Generator(device=dev).manual_seed(N)
        w = torch.randint(0, W_ONE + 1, (N,), generator=g, device=dev, dtype=torch.int64)
        w[torch.rand(N, generator=g, device=dev) < 0.5] = 0                       # half the members weigh nothing
        rows = torch.randn((N_ROWS, N), generator=g, device=dev, dtype=torch.float64)
        cum = torch.empty(N, dtype=torch.int64, device=dev)
        flags = torch.empty(1, dtype=torch.int64, device=dev)
        work = torch.empty(int(lib.fiveeq_wscan_chunks(N)), dtype=torch.int64, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        scan = lambda: _capi.check(lib, lib.fiveeq_wscan(N, p(w), p(work), p(cum), p(flags), st))      # noqa: E731
        scan()
        W = int(cum[-1])
        assert int(flags[0]) == 0 and W == int(w.sum())
        for M in (N // 10, N):
            plan = resample_plan([W], 0, M, W // 3)
            q, a_, s, b = plan["q"], plan["a"], plan["s"], plan["b"]
            src = torch.empty(M, dtype=torch.int32, device=dev)
            out = torch.empty((N_ROWS, M), dtype=torch.float64, device=dev)
            pick = lambda: _capi.check(lib, lib.fiveeq_resample_pick(N, p(cum), 0, M, q, a_, s, b, 0, M, p(src), st))     # noqa: E731
            gather = lambda: _capi.check(lib, lib.fiveeq_gather_rows_f64(N_ROWS, M, N, p(rows), M, p(out), p(src), st))     # noqa: E731

            def hip():
                scan()
                pick()
                gather()

            j = torch.arange(M, device=dev, dtype=torch.int64)
            t_cum, t_src, t_out = torch.empty_like(cum), torch.empty(M, dtype=torch.int64, device=dev), torch.empty_like(out)
            t_scan = lambda: torch.cumsum(w, 0, out=t_cum)      # noqa: E731
            t_pick = lambda: torch.searchsorted(t_cum, j * q + a_ + torch.div(j * s + b, M, rounding_mode="floor"), right=True,     # noqa: E731
                                                out=t_src)
            t_gather = lambda: torch.index_select(rows, 1, t_src, out=t_out)      # noqa: E731

            def torch_parts():
                t_scan()
                t_pick()
                t_gather()

            hip()
            torch_parts()
            torch.cuda.synchronize()
            assert torch.equal(t_cum, cum) and torch.equal(t_src.to(torch.int32), src) and torch.equal(t_out, out)
            fmt = lambda t: f"{t[0]:9.1f} ({t[1]:.1f} .. {t[2]:.1f})"      # noqa: E731
            t_hip, t_torch = timed(hip, torch_parts)
            (h1, g1), (h2, g2), (h3, g3) = timed(scan, t_scan), timed(pick, t_pick), timed(gather, t_gather)
            lines.append(f"N = {N:>10,}  M = {M:>10,}   hip {fmt(t_hip)}   torch {fmt(t_torch)}   hip / torch = {t_hip[0] / t_torch[0]:.2f}")
            lines.append(f"    parts, hip:   scan {fmt(h1)}   pick {fmt(h2)}   gather {fmt(h3)}")
            lines.append(f"    parts, torch: cumsum {fmt(g1)}   positions + searchsorted {fmt(g2)}   index_select {fmt(g3)}")
            del t_cum, t_src, t_out
            print("\n".join(lines[-3:]), flush=True)
        del w, rows, cum
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
