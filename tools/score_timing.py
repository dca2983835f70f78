"""Cost of scoring stored rows (fiveeq_score_rows_*) on the MI355X: kernel time against the algorithmic bytes
w N (live row-quantities) + 48 N n_q, the box's non-temporal copy over the same byte count from the same process, the torch
expression of the same operations a user writes without the pass, and an all-rows-live run beside the 170-of-750 one.
Events on the stream, warm-up, the median of 21.  --out STEM writes STEM.txt (the lines) and STEM.json (the figures DESIGN.md
cites): kept as profiles/r15/score_rows.*"""
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fiveeqscm_amd import _capi  # noqa: E402
from fiveeqscm_amd.constrain import Observations, score_rows  # noqa: E402

OUT, FIG = [], {}
N, K, LIVE0, LIVE1 = 1_000_000, 750, 100, 270                 # members, stored rows, the record's live steps [100, 270)


def say(line=""):
    print(line, flush=True)
    OUT.append(line)


def timed(fn, warm=3, reps=21):
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
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def copy_time(n_bytes):
    """fiveeq_stream_copy_nt_f64 moving n_bytes in all (half read, half written)."""
    lib = _capi.load()
    n = max(1024, n_bytes // 16 // 1024 * 1024)
    src = torch.ones(n, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    med, lo, hi = timed(lambda: _capi.check(lib, lib.fiveeq_stream_copy_nt_f64(n, ctypes.c_void_p(src.data_ptr()),
                                                                               ctypes.c_void_p(dst.data_ptr()), st)))
    del src, dst
    return med, lo, hi, 16 * n


def table(live):
    t = np.zeros((K, 4))
    idx = np.arange(*live)
    t[idx, 0], t[idx, 1] = 1.0 + 0.002 * (idx - live[0]), 1.0 / 0.1 ** 2
    t[live[0]:live[0] + 50, 2] = 1.0 / 50
    return Observations(t)


def case(name, dtype, Q):
    w = 8 if dtype == torch.float64 else 4
    g = torch.Generator(device="cuda").manual_seed(1)
    shape = (K, N) if Q == 1 else (K, Q, N)
    rows = torch.empty(shape, dtype=dtype, device="cuda")
    for k in range(0, K, 50):                                  # filled in blocks: no second buffer of the whole size
        rows[k:k + 50] = torch.rand(rows[k:k + 50].shape, generator=g, device="cuda", dtype=torch.float32) * 3.0
    steps = np.arange(K)
    lib = _capi.load()
    fn = lib.fiveeq_score_rows_f64 if w == 8 else lib.fiveeq_score_rows_f32
    st32 = torch.from_numpy(steps.astype(np.int32)).cuda()
    misfit = torch.zeros((Q, 3, N), dtype=torch.float64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                  # noqa: E731
    say(f"--- {name}: {N} members x {K} stored rows, {'fp64' if w == 8 else 'fp32'}, n_q = {Q} ({rows.numel() * w / 1e9:.1f} GB stored)")
    fig = {}
    for label, live in (("live170", (LIVE0, LIVE1)), ("live750", (0, K))):
        rec = table(live)
        obs = torch.from_numpy(np.stack([rec.table] * Q)).cuda()          # (stack copies)
        n_live = len(rec.live_steps)
        nbytes = w * N * n_live * Q + 48 * N * Q
        call = lambda: _capi.check(lib, fn(Q, K, N, ptr(rows), Q * N, N, ptr(st32), ptr(obs), K, ptr(misfit), N, stream))   # noqa: E731
        med, lo, hi = timed(call)
        cmed, clo, chi, cbytes = copy_time(nbytes)
        fig[label] = {"live_rows": n_live, "ms": med * 1e3, "min_ms": lo * 1e3, "max_ms": hi * 1e3, "bytes": nbytes, "GBps": nbytes / med / 1e9,
                      "copy_ms": cmed * 1e3, "copy_GBps": cbytes / cmed / 1e9, "ratio_to_copy": (nbytes / med) / (cbytes / cmed)}
        say(f"fiveeq_score_rows_* alone, {n_live} live of {K} rows: median {med * 1e3:.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f}); "
            f"algorithmic bytes {nbytes / 1e9:.3f} GB -> {nbytes / med / 1e9:.0f} GB/s; fiveeq_stream_copy_nt_f64 over {cbytes / 1e9:.3f} GB: "
            f"median {cmed * 1e3:.3f} ms (min {clo * 1e3:.3f}, max {chi * 1e3:.3f}) -> {cbytes / cmed / 1e9:.0f} GB/s; "
            f"ratio {fig[label]['ratio_to_copy']:.2f}")
    fig["live750_over_live170"] = fig["live750"]["ms"] / fig["live170"]["ms"]
    say(f"all rows live / 170 live: {fig['live750_over_live170']:.2f} x the time for {K / (LIVE1 - LIVE0):.2f} x the rows "
        f"({(w * K + 48) / (w * (LIVE1 - LIVE0) + 48):.2f} x the bytes)")
    # what a user writes without the pass: the same five operations, every live row at once, torch's reductions
    rec = table((LIVE0, LIVE1))
    tab = torch.from_numpy(rec.table[LIVE0:LIVE1].copy()).cuda()
    o, p, b = (tab[:, c].reshape((-1,) + (1,) * (len(shape) - 1)) for c in range(3))

    def eager():
        Tw = rows[LIVE0:LIVE1].double()
        d = Tw - o
        pd = p * d
        return torch.stack([(b * Tw).sum(0), pd.sum(0), (pd * d).sum(0)], dim=-2)

    emed, elo, ehi = timed(eager, warm=2, reps=21)
    got = score_rows(rows, steps, rec if Q == 1 else [rec] * Q)
    same = bool(torch.equal(eager().reshape(got.shape), got))
    fig["eager_ms"], fig["eager_over_pass"], fig["eager_same_bits"] = emed * 1e3, emed * 1e3 / fig["live170"]["ms"], same
    say(f"torch eager (slice, widen, d = T - o, pd = p d, three sums over the rows): median {emed * 1e3:.3f} ms (min {elo * 1e3:.3f}, "
        f"max {ehi * 1e3:.3f}) -> {fig['eager_over_pass']:.1f} x the pass; same bits as the pass (= the in-loop misfit): {same}")
    FIG[name] = fig
    del rows


def main():
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    say("algorithmic bytes = w N (live row-quantities) + 48 N n_q (DESIGN.md 3.15)")
    case("f64_T", torch.float64, 1)
    case("f64_C3", torch.float64, 3)
    case("f32_T", torch.float32, 1)
    case("f32_C3", torch.float32, 3)
    if "--out" in sys.argv[1:]:
        stem = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(stem) or ".", exist_ok=True)
        with open(stem + ".txt", "w") as fh:
            fh.write("\n".join(OUT) + "\n")
        with open(stem + ".json", "w") as fh:
            json.dump(FIG, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
