"""Cost of the trajectory-metrics pass on the MI355X: kernel time and read bandwidth, the box's wide copy rate from the same
process, and the torch formulation a user writes today.  Events on the stream, warm-up, repeats, the spread.
--out FILE also writes the lines to FILE (kept as profiles/r13/traj_metrics.txt)."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fiveeqscm_amd import _capi  # noqa: E402
from fiveeqscm_amd.metrics import trajectory_metrics  # noqa: E402

OUT = []


def say(line=""):
    print(line, flush=True)
    OUT.append(line)


def timed(fn, warm=2, reps=7):
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


def copy_rate():
    lib = _capi.load()
    n = 1 << 28                                                # 2 GiB each way
    src = torch.ones(n, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    med, lo, hi = timed(lambda: _capi.check(lib, lib.fiveeq_stream_copy_wide_f64(n, ctypes.c_void_p(src.data_ptr()),
                                                                                 ctypes.c_void_p(dst.data_ptr()), st)))
    say(f"fiveeq_stream_copy_wide_f64, {n} fp64 ({n * 8 / 2**30:.0f} GiB read + as much written): median {med * 1e3:.3f} ms "
        f"(min {lo * 1e3:.3f}, max {hi * 1e3:.3f}) -> {2 * n * 8 / med / 1e12:.3f} TB/s both directions, "
        f"{n * 8 / med / 1e12:.3f} TB/s one direction's share")
    del src, dst


def case(N, K, dtype, levels, windows):
    w = 8 if dtype == torch.float64 else 4
    g = torch.Generator(device="cuda").manual_seed(1)
    T = (torch.rand((K, N), generator=g, device="cuda", dtype=torch.float32) * 3.0).to(dtype)
    T += torch.linspace(0, 1, K, device="cuda", dtype=dtype).reshape(-1, 1)
    steps = np.arange(K) * 1 + 100
    say(f"--- {N} members x {K} stored rows, {'fp64' if w == 8 else 'fp32'} ({N * K * w / 1e9:.2f} GB of rows), "
        f"L = {len(levels)}, W = {len(windows)}")
    med, lo, hi = timed(lambda: trajectory_metrics(T, steps, levels, windows))
    say(f"trajectory_metrics (one call, with its state allocation and the steps upload): median {med * 1e3:.3f} ms "
        f"(min {lo * 1e3:.3f}, max {hi * 1e3:.3f}) -> rows read at {N * K * w / med / 1e12:.3f} TB/s "
        f"(spread {(hi - lo) / med * 100:.1f} %)")
    # the kernel alone: the C entry point on preallocated state blocks and a steps table already on the device
    lib = _capi.load()
    L, W = len(levels), len(windows)
    fmet = torch.empty((1 + W, N), dtype=torch.float64, device="cuda")
    imet = torch.empty((2 + 2 * L, N), dtype=torch.int32, device="cuda")
    st32 = torch.from_numpy(steps.astype(np.int32)).cuda()
    c_lv = (ctypes.c_double * L)(*levels)
    c_wn = (ctypes.c_int32 * (2 * W))(*[v for ab in windows for v in ab])
    fn = lib.fiveeq_traj_metrics_f64 if w == 8 else lib.fiveeq_traj_metrics_f32
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                  # noqa: E731
    call = lambda: _capi.check(lib, fn(1, K, N, N, ptr(T), K * N, ptr(st32), L, ctypes.cast(c_lv, ctypes.c_void_p), W,   # noqa: E731
                                       ctypes.cast(c_wn, ctypes.c_void_p), ptr(fmet), ptr(imet), 1, stream))
    state_bytes = N * (8 * (1 + W) + 4 * (2 + 2 * L))
    for reps in (1, 20):                                       # one launch per timed window, and 20 back to back
        med, lo, hi = timed(lambda: [call() for _ in range(reps)], warm=2, reps=9)
        med, lo, hi = med / reps, lo / reps, hi / reps
        say(f"fiveeq_traj_metrics_* alone, {reps} launch(es) per window: median {med * 1e3:.3f} ms per launch (min {lo * 1e3:.3f}, "
            f"max {hi * 1e3:.3f}; spread {(hi - lo) / med * 100:.1f} %) -> rows read at {N * K * w / med / 1e12:.3f} TB/s; with the "
            f"{state_bytes / 1e6:.0f} MB of state written: {(N * K * w + state_bytes) / med / 1e12:.3f} TB/s")
    a, b = windows[0]
    ia, ib = int(np.searchsorted(steps, a)), int(np.searchsorted(steps, b))

    def torch_way():
        pk = T.max(0)
        firsts = [(T >= lv).int().argmax(0) for lv in levels]
        mean = T[ia:ib].mean(0)
        return pk, firsts, mean

    med2, lo2, hi2 = timed(torch_way, warm=1, reps=5)
    say(f"torch formulation (T.max(0), (T >= level).int().argmax(0) per level, slice mean): median {med2 * 1e3:.3f} ms "
        f"(min {lo2 * 1e3:.3f}, max {hi2 * 1e3:.3f}) -> {med2 / med:.2f} x the metrics pass")
    m = trajectory_metrics(T, steps, levels, windows)
    pk, firsts, _ = torch_way()
    same_peak = bool(torch.equal(m.peak, pk.values.double()))
    say(f"same peak as torch: {same_peak}")
    del T


def main():
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    copy_rate()
    case(1_000_000, 750, torch.float64, (1.5, 2.0), ((600, 700),))
    case(12_500_000, 64, torch.float32, (1.5, 2.0), ((130, 150),))
    copy_rate()
    if "--out" in sys.argv[1:]:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
