"""Cost of the carbon-rows pass (fiveeq_carbon_rows_*) on the MI355X: 1M members of the 4 + 1 + 1 layout, 250 stored rows
processed in row blocks (the outputs of one block fit beside the trajectories), in fp64 and fp32:
    fraction          the airborne fraction of CO2 alone — the row-parallel grid, one row read and one written
    fraction_alpha    fraction and alpha of all three gases — the row-parallel grid, the T row and the r rows read too
    sink_uptake       sink and uptake of all three gases — a lane carries G_a of its members through the rows, from block to block
against fiveeq_stream_copy_wide_f64 over THE SAME BYTES (half read, half written) from the same process.  Events on the stream,
warm-up, the median of 21 sweeps over all rows.  --out STEM writes STEM.txt (the lines) and STEM.json (the figures
profiles/r28/NOTES.md cites)."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fiveeqscm_amd import _capi, params  # noqa: E402
from tools.score_timing import timed  # noqa: E402

OUT, FIG = [], {}
N, K, BLOCK, G = 1_000_000, 250, 50, 3
CASES = {"fraction": (0b001, ("fraction",)), "fraction_alpha": (0b111, ("fraction", "alpha")), "sink_uptake": (0b111, ("uptake", "sink"))}
ORDER = ("airborne", "cumE", "uptake", "fraction", "iirf", "alpha", "sink")


def say(line=""):
    print(line, flush=True)
    OUT.append(line)


def copy_time(n_bytes):
    """fiveeq_stream_copy_wide_f64 moving n_bytes in all (half read, half written)."""
    lib = _capi.load()
    n = max(1024, n_bytes // 16 // 1024 * 1024)
    src = torch.ones(n, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    med, lo, hi = timed(lambda: _capi.check(lib, lib.fiveeq_stream_copy_wide_f64(n, ctypes.c_void_p(src.data_ptr()),
                                                                                 ctypes.c_void_p(dst.data_ptr()), st)))
    del src, dst
    return med, lo, hi, 16 * n


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
    p = params.sample_ensemble_shard(base, N, 0, N, device="cuda")
    r = torch.stack([p[key][gas].to(dtype) for gas in range(G) for key in ("r0", "rC", "rT")]).contiguous()
    drive = torch.ones((K, _capi.DRIVE_STRIDE), dtype=dtype, device="cuda")
    cum = torch.cumsum(torch.ones((K, _capi.MAX_GAS), dtype=dtype, device="cuda"), 0).contiguous()
    steps = torch.arange(K, dtype=torch.int32, device="cuda")
    outs = [torch.empty((BLOCK, G, N), dtype=dtype, device="cuda") for _ in range(2)]
    ga_io = torch.zeros((G, N), dtype=dtype, device="cuda")
    lib = _capi.load()
    fn = lib.fiveeq_carbon_rows_f64 if w == 8 else lib.fiveeq_carbon_rows_f32
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)                     # noqa: E731
    say(f"--- {name}: {N} members x {K} stored rows in blocks of {BLOCK}, {'fp64' if w == 8 else 'fp32'}, pools 4 + 1 + 1 "
        f"({(C.numel() + T.numel()) * w / 1e9:.1f} GB stored)")
    fig = {}
    for label, (gas_mask, want) in CASES.items():
        n_sel = bin(gas_mask).count("1")
        alpha, seq = "alpha" in want, "sink" in want
        slots = [ptr(outs[want.index(o)]) if o in want else None for o in ORDER]

        def sweep():
            for k in range(0, K, BLOCK):
                _capi.check(lib, fn(ctypes.byref(model), BLOCK, N, N, ptr(C, k * G * N * w), G * N, N, ptr(T, k * N * w) if alpha else None,
                                    N, ptr(steps, 4 * k), ptr(drive), ptr(cum), K, ptr(r) if alpha else None, 0, gas_mask, *slots, N,
                                    None, ptr(ga_io) if seq else None, stream))
        per_row = w * (n_sel + (1 if alpha else 0)) + w * n_sel * len(want)
        per_block = w * N * ((3 * n_sel if alpha else 0) + (2 * n_sel if seq else 0))
        nbytes = per_row * N * K + per_block * (K // BLOCK)
        med, lo, hi = timed(sweep)
        cmed, clo, chi, cbytes = copy_time(nbytes)
        fig[label] = {"ms": med * 1e3, "min_ms": lo * 1e3, "max_ms": hi * 1e3, "bytes": nbytes, "bytes_per_member_row": per_row,
                      "GBps": nbytes / med / 1e9, "copy_ms": cmed * 1e3, "copy_GBps": cbytes / cmed / 1e9,
                      "ratio_to_copy": (nbytes / med) / (cbytes / cmed)}
        say(f"want = {', '.join(want)} of {n_sel} gas(es): median {med * 1e3:.3f} ms per sweep of {K} rows (min {lo * 1e3:.3f}, max "
            f"{hi * 1e3:.3f}); {per_row} B per member-row, {nbytes / 1e9:.2f} GB -> {nbytes / med / 1e9:.0f} GB/s; "
            f"fiveeq_stream_copy_wide_f64 over {cbytes / 1e9:.2f} GB: median {cmed * 1e3:.3f} ms (min {clo * 1e3:.3f}, max {chi * 1e3:.3f}) "
            f"-> {cbytes / cmed / 1e9:.0f} GB/s; ratio {fig[label]['ratio_to_copy']:.2f}")
    FIG[name] = fig
    del C, T


def main():
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    say("bytes per member-row = w (selected gases + [T read]) + w (selected gases x outputs); per block and member the r rows "
        "(alpha) and G_a in and out (sink)")
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
