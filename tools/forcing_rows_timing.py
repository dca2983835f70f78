"""Cost of the forcing-rows pass (fiveeq_forcing_rows_*) on the MI355X: 1M members of the 4 + 1 + 1 layout, the 750 stored rows of
BASELINE configs[2] processed in row blocks (the outputs of one block fit beside the trajectories), want = ("F",) — the
row-parallel grid — and want = ("F", "N", "H") — a lane carries its members through the rows, the heat carried from block to
block — in fp64 and fp32; against the box's non-temporal copy (fiveeq_stream_copy_nt_f64) over the same number of bytes from the
same process.  Events on the stream, warm-up, the median of 21 sweeps over all 750 rows.  --out STEM writes STEM.txt (the
lines) and STEM.json (the figures DESIGN.md cites): kept as profiles/r17/forcing_rows.*; the ISA facts of the .txt are added
from tools/kernel_isa_stats.py."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fiveeqscm_amd import _capi, params  # noqa: E402
from tools.score_timing import copy_time, timed  # noqa: E402

OUT, FIG = [], {}
N, K, BLOCK, G = 1_000_000, 750, 50, 3


def say(line=""):
    print(line, flush=True)
    OUT.append(line)


def case(name, dtype):
    w = 8 if dtype == torch.float64 else 4
    base = params.default_params("multigas")
    model = params.make_model(base, 1.0)
    C0 = torch.tensor(np.asarray(base["PI_conc"], dtype=np.float64), device="cuda").reshape(1, G, 1)
    g = torch.Generator(device="cuda").manual_seed(1)
    C = torch.empty((K, G, N), dtype=dtype, device="cuda")
    T = torch.empty((K, N), dtype=dtype, device="cuda")
    for k in range(0, K, BLOCK):                               # filled in blocks: no second buffer of the whole size
        C[k:k + BLOCK] = C0 * (1.0 + 1.5 * torch.rand((BLOCK, G, N), generator=g, device="cuda", dtype=torch.float32))
        T[k:k + BLOCK] = 3.0 * torch.rand((BLOCK, N), generator=g, device="cuda", dtype=torch.float32)
    q = (0.2 + 0.3 * torch.rand((2, N), generator=g, device="cuda", dtype=torch.float32)).to(dtype)
    drive = torch.zeros((K, _capi.DRIVE_STRIDE), dtype=dtype, device="cuda")
    steps = torch.arange(K, dtype=torch.int32, device="cuda")
    F, Nn = (torch.empty((BLOCK, N), dtype=dtype, device="cuda") for _ in range(2))
    H = torch.empty((BLOCK, N), dtype=torch.float64, device="cuda")
    H_io = torch.zeros((N,), dtype=torch.float64, device="cuda")
    lib = _capi.load()
    fn = lib.fiveeq_forcing_rows_f64 if w == 8 else lib.fiveeq_forcing_rows_f32
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)                     # noqa: E731
    say(f"--- {name}: {N} members x {K} stored rows in blocks of {BLOCK}, {'fp64' if w == 8 else 'fp32'}, pools 4 + 1 + 1 "
        f"({(C.numel() + T.numel()) * w / 1e9:.1f} GB stored)")
    fig = {}
    for label, full in (("F", False), ("F_N_H", True)):
        def sweep():
            for k in range(0, K, BLOCK):
                _capi.check(lib, fn(ctypes.byref(model), BLOCK, N, N, ptr(C, k * G * N * w), G * N, N, ptr(T, k * N * w), N,
                                    ptr(steps, 4 * k), ptr(drive), K, ptr(q), None, 0, None, ptr(F), None, ptr(Nn) if full else None,
                                    ptr(H) if full else None, N, ptr(H_io) if full else None, None, None, stream))
        per_row = w * (G + (1 if full else 0)) + w * (2 if full else 1) + (8 if full else 0)
        nbytes = per_row * N * K + (16 * N * (K // BLOCK) if full else 0)
        med, lo, hi = timed(sweep)
        cmed, clo, chi, cbytes = copy_time(nbytes)
        fig[label] = {"ms": med * 1e3, "min_ms": lo * 1e3, "max_ms": hi * 1e3, "bytes": nbytes, "bytes_per_member_row": per_row,
                      "GBps": nbytes / med / 1e9, "copy_ms": cmed * 1e3, "copy_GBps": cbytes / cmed / 1e9,
                      "ratio_to_copy": (nbytes / med) / (cbytes / cmed)}
        say(f"want = {label.replace('_', ', ')}: median {med * 1e3:.3f} ms per sweep of {K} rows (min {lo * 1e3:.3f}, max {hi * 1e3:.3f}); "
            f"{per_row} B per member-row, {nbytes / 1e9:.2f} GB -> {nbytes / med / 1e9:.0f} GB/s; fiveeq_stream_copy_nt_f64 over "
            f"{cbytes / 1e9:.2f} GB: median {cmed * 1e3:.3f} ms (min {clo * 1e3:.3f}, max {chi * 1e3:.3f}) -> {cbytes / cmed / 1e9:.0f} GB/s; "
            f"ratio {fig[label]['ratio_to_copy']:.2f}")
    FIG[name] = fig
    del C, T


def main():
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    say("bytes per member-row = w (G + [T read]) + w (outputs of the rows' type) + 8 [H]  (DESIGN.md 3.17)")
    case("f64", torch.float64)
    case("f32", torch.float32)
    if "--out" in sys.argv[1:]:
        stem = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(stem) or ".", exist_ok=True)
        with open(stem + ".txt", "w") as fh:
            fh.write("\n".join(OUT) + "\n")
        with open(stem + ".json", "w") as fh:
            json.dump(FIG, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
