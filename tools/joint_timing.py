"""Cost of the two JOINT STATISTICS passes on the MI355X: 1M members, 20 x rows by 8 y rows, 16 bins, fp64 and fp32.  Per pass
the kernel time (events on the stream, warm-up, repeats, the spread), the algorithmic bytes — every row read once per row tile
that needs it, plus the weights once per tile — and the ratio to fiveeq_stream_copy_f64 moving the same bytes on the same card.
--out FILE also writes the lines to FILE (kept as profiles/r14/joint_timing.txt)."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fiveeqscm_amd import _capi  # noqa: E402

OUT = []


def say(line=""):
    print(line, flush=True)
    OUT.append(line)


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
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def copy_time(lib, n_bytes):
    """fiveeq_stream_copy_f64 over n_bytes of traffic (half read, half written)"""
    n = max(1024, int(n_bytes) // 16)
    src = torch.ones(n, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return timed(lambda: _capi.check(lib, lib.fiveeq_stream_copy_f64(n, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), st)))


def case(N, Kx, Ky, B, dtype):
    lib = _capi.load()
    t = [lib.fiveeq_joint_tile(k) for k in range(8)]
    el = 8 if dtype == torch.float64 else 4
    sfx = "f64" if el == 8 else "f32"
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((Kx, N), generator=g, device="cuda", dtype=torch.float32).to(dtype)
    y = (torch.randn((Ky, Kx), generator=g, device="cuda", dtype=torch.float32).to(dtype) @ x) / Kx ** 0.5
    w = torch.randint(0, 1 << 32, (N,), generator=g, device="cuda", dtype=torch.int64)
    piv = torch.cat([x.double().mean(1), y.double().mean(1)])
    edges = torch.quantile(x[:, ::64].double(), torch.arange(1, B, device="cuda", dtype=torch.float64) / B, dim=1).T.contiguous()
    R = Kx + Ky
    chunks = int(lib.fiveeq_joint_chunks(N))
    work = torch.empty(chunks * max(int(lib.fiveeq_joint_moments_words(Kx, Ky)), int(lib.fiveeq_cond_sums_words(Kx, Ky, B))),
                       dtype=torch.float64, device="cuda")
    oa = torch.empty(Kx * Ky + 3 * R + 4, dtype=torch.float64, device="cuda")
    ob = torch.empty(Kx * B * (Ky + 1) + Kx, dtype=torch.float64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda a, k=0: ctypes.c_void_p(a.data_ptr() + 8 * k)      # noqa: E731
    mom = lambda: _capi.check(lib, getattr(lib, f"fiveeq_joint_moments_{sfx}")(      # noqa: E731
        N, Kx, N, p(x), Ky, N, p(y), p(w), p(piv), p(work), p(oa), p(oa, Kx * Ky), p(oa, Kx * Ky + 2 * R), p(oa, Kx * Ky + 2 * R + 4), st))
    cond = lambda: _capi.check(lib, getattr(lib, f"fiveeq_cond_sums_{sfx}")(      # noqa: E731
        N, Kx, N, p(x), Ky, N, p(y), p(w), B, p(edges), p(piv, Kx), p(work), p(ob), p(ob, Kx * B * Ky), p(ob, Kx * B * (Ky + 1)), st))
    say(f"--- {N} members, {Kx} x rows by {Ky} y rows, {B} bins, {'fp64' if el == 8 else 'fp32'} "
        f"({R * N * el / 1e6:.0f} MB of rows + {N * 8 / 1e6:.0f} MB of weights read once)")
    up = lambda a, b: -(-a // b)      # noqa: E731
    # (a): tile (tx, ty) reads its TX x rows and TY y rows (an edge tile its last row again) and the weights
    tiles_a = up(Kx, t[0]) * up(Ky, t[1])
    bytes_a = tiles_a * ((t[0] + t[1]) * N * el + N * 8)
    # (b): a workgroup column (x row, bin group, y tile) reads the x row, TY y rows and the weights
    tiles_b = Kx * up(B, t[5]) * up(Ky, t[6])
    bytes_b = tiles_b * ((1 + t[6]) * N * el + N * 8)
    once = R * N * el + N * 8
    for name, fn, nbytes, tiles in (("fiveeq_joint_moments", mom, bytes_a, tiles_a), ("fiveeq_cond_sums", cond, bytes_b, tiles_b)):
        med, lo, hi = timed(fn)
        cmed, _, _ = copy_time(lib, nbytes)
        say(f"{name}_{sfx}: median {med * 1e3:.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f}; spread {(hi - lo) / med * 100:.1f} %); "
            f"{tiles} row tiles, algorithmic bytes {nbytes / 1e6:.0f} MB = {nbytes / once:.2f} x the rows and weights read once "
            f"-> {nbytes / med / 1e12:.3f} TB/s; fiveeq_stream_copy_f64 of the same bytes: {cmed * 1e3:.3f} ms -> ratio {med / cmed:.2f}")


def main():
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; tile {[_capi.load().fiveeq_joint_tile(k) for k in range(8)]}")
    for dtype in (torch.float64, torch.float32):
        case(1_000_000, 20, 8, 16, dtype)
    if "--out" in sys.argv[1:]:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
