"""Running means and linear trends of stored rows, per member — the two noise-robust reductions of a trajectory.  With internal
variability on (member_forcing=ar1_noise_rows(...)) a member's stored T rows are noisy year to year: a warming level is then
the first 20-year MEAN at or above the level, dated at the window's midpoint, not the first warm year, and a warming rate is a
least-squares slope over a period, not a difference of two rows.

    sm = running_mean(eng.T, eng.out_steps, 20)                       # or eng.running_mean(20)
    m = trajectory_metrics(sm.rows, sm.steps, levels=(1.5, 2.0))      # m.first: the crossing of the 20-row mean
    tr = window_trends(eng.T, eng.out_steps, ((130, 171),), dt=1.0)   # tr.slope[0]: K per year over steps 130..170

Two streaming HIP passes (include/fiveeq.h, "RUNNING MEANS AND TRENDS"; csrc/fiveeq_smooth.hpp).  Every running mean is summed
afresh from its own `window` rows in ascending order and divided once — no sliding update — and the trend sums are fp64 sums
in row order, so the bits do not depend on the launch shape, on how the rows are split into calls (`state=`) or on how the
members are split into shards.  Device rows only: there is no CPU path (_smooth_host.py is the NumPy twin the CPU tests put
behind the same switch).
"""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _rowargs
from .metrics import _rows_in_place, _spec

ALIGNS = ("centre", "trailing")


def _lib_and_stream(rows):
    """(library, _capi, stream, device guard) for rows on a GPU.  (_smooth_host.host_passes() replaces this function and the
    next.)"""
    from . import _capi
    lib = _capi.load()
    return lib, _capi, ctypes.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream), torch.cuda.device(rows.device)


def _passes_apply(rows):
    return rows.is_cuda and rows.dtype in (torch.float32, torch.float64)


def _device_rows(rows, what):
    if not isinstance(rows, torch.Tensor) or rows.dim() not in (2, 3):
        raise ValueError("rows: want a tensor [n_rows, N] or [S, n_rows, N]")
    if not _passes_apply(rows):
        raise TypeError(f"rows must be fp32 / fp64 rows on a GPU (got {rows.dtype} on {rows.device}): {what} run through the "
                        "HIP kernel and have no CPU fallback")
    x = rows if rows.dim() == 3 else rows.unsqueeze(0)
    if x.shape[2] < 1:
        raise ValueError("rows: no members")
    return x


@dataclass
class SmoothedRows:
    """The result of running_mean.  rows: fp64 [n_out, N] ([S, n_out, N] with a scenario axis) on the input's device, n_out =
    max(0, rows seen - window + 1) minus what earlier calls of the state returned; steps: the model step each output is dated
    at — "trailing": the window's last step, "centre": its step number window // 2 (the first year of the second decade for
    window = 20).  tail: a clone of the last min(window - 1, rows seen) input rows in their dtype, and seen_steps: every step
    folded so far — what a `state=` call continues from."""
    rows: torch.Tensor
    steps: np.ndarray             # int64 [n_out]
    window: int
    align: str
    tail: torch.Tensor
    seen_steps: np.ndarray        # int64


def _even_steps(st, before):
    """ValueError unless `before` (the steps an earlier call folded) followed by `st` is evenly spaced."""
    seq = np.concatenate([before, st])
    if seq.size > 2 and np.any(np.diff(seq) != seq[1] - seq[0]):
        raise ValueError("steps: want evenly spaced model steps" + (", continuing the state's spacing from its last step" if before.size else "")
                         + ": a mean over unevenly stored rows is not a mean over time")
    return seq


def running_mean(rows, steps, window, align="centre", state=None):
    """The running mean over `window` consecutive rows, per member.  rows [n_rows, N] or [S, n_rows, N] (fp32 / fp64 ON THE
    GPU; a column-sliced view of a buffer less than twice as wide is read in place, a narrower slice is copied); steps
    [n_rows]: the model step each row holds, strictly increasing and EVENLY spaced (ValueError otherwise); 1 <= window <= 32.
    Output k is ((x[k] + x[k+1]) + ...) + x[k+window-1], one rounded fp64 add per row in ascending order, divided once by
    window.  Returns SmoothedRows; its rows and steps go into trajectory_metrics, score_rows, gather_summary and drivers like
    stored rows.  state: the result of an earlier call over the rows directly before these (same window, align, members and
    dtype, the next evenly spaced step, else ValueError) — the outputs of the calls, concatenated, are bit for bit those of
    one call over all the rows.  Runs on the current stream."""
    from ._capi import MAX_SMOOTH_WINDOW
    x = _device_rows(rows, "the running means")
    scen = rows.dim() == 3
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or not 1 <= int(window) <= MAX_SMOOTH_WINDOW:
        raise ValueError(f"window: want an integer 1..{MAX_SMOOTH_WINDOW}, got {window!r}")
    window = int(window)
    if align not in ALIGNS:
        raise ValueError(f"align: want one of {ALIGNS}, got {align!r}")
    S, K, N = x.shape
    st = _rowargs.model_steps(steps, K, non_negative=True)
    dev = rows.device
    if state is not None:
        if not isinstance(state, SmoothedRows) or state.window != window or state.align != align:
            raise ValueError("state: window and align must equal those of the call that made it")
        want = (S, state.tail.shape[-2], N) if scen else (state.tail.shape[-2], N)
        if tuple(state.tail.shape) != want or state.tail.device != dev or state.tail.dtype != rows.dtype:
            raise ValueError(f"state: made for other rows ({tuple(state.tail.shape)} {state.tail.dtype} on {state.tail.device})")
        if K and state.seen_steps.size and st[0] <= state.seen_steps[-1]:
            raise ValueError(f"steps: the first new step {int(st[0])} does not lie after the state's last step {int(state.seen_steps[-1])}")
    seen = _even_steps(st, state.seen_steps if state is not None else np.zeros(0, dtype=np.int64))
    old_tail = None if state is None else (state.tail if scen else state.tail.unsqueeze(0))
    n_tail = 0 if old_tail is None else int(old_tail.shape[1])
    n_out = max(0, n_tail + K - window + 1)
    x, ld, scen_stride = _rows_in_place(x)
    out = torch.empty((S, n_out, ld), dtype=torch.float64, device=dev)
    tail = None
    if n_tail:                                                 # ONE ld for rows, tail and out in the C ABI
        tail = old_tail.contiguous() if ld == N else torch.empty((S, n_tail, ld), dtype=rows.dtype, device=dev)
        if ld != N:
            tail[:, :, :N] = old_tail
    if n_out:
        lib, capi, stream, guard = _lib_and_stream(rows)
        ptr = _rowargs.ptr
        _rowargs.call(lib, capi, "fiveeq_running_mean", rows.dtype, dev, S, K, N, ld, ptr(x) if K else None, scen_stride, window, n_tail,
                      ptr(tail), n_tail * ld, ptr(out), n_out * ld, stream=stream, guard=guard)
    keep = min(window - 1, n_tail + K)
    both = x[:, :, :N] if old_tail is None else torch.cat([old_tail, x[:, :, :N]], dim=1)
    new_tail = both[:, both.shape[1] - keep:].clone()
    x_steps = seen[seen.size - (n_tail + K):]
    shift = window - 1 if align == "trailing" else window // 2
    drop = (lambda t: t) if scen else (lambda t: t[0])
    return SmoothedRows(rows=drop(out[:, :, :N]), steps=x_steps[shift:shift + n_out].copy(), window=window, align=align,
                        tail=drop(new_tail), seen_steps=seen)


@dataclass
class WindowTrends:
    """The result of window_trends: fp64 tensors [W, N] ([S, W, N] with a scenario axis) on the rows' device.  sx / stx: the
    sums of T and of (t - a) T over the stored steps inside each window; count: those steps' number per window; mean = sx /
    count; slope: the least-squares trend per year, NaN for a window with fewer than 2 stored steps.  steps: every step
    folded so far."""
    sx: torch.Tensor
    stx: torch.Tensor
    count: tuple
    mean: torch.Tensor
    slope: torch.Tensor
    steps: np.ndarray
    windows: tuple
    dt: float


def trend_moments(steps, windows):
    """Per window [a, b) the exact integers (n, su, suu) = (count, sum u, sum u^2), u = t - a over the `steps` inside."""
    out = []
    for a, b in windows:
        u = [int(t) - a for t in steps if a <= int(t) < b]
        out.append((len(u), sum(u), sum(v * v for v in u)))
    return out


def window_trends(rows, steps, windows, dt=1.0, state=None):
    """Least-squares linear trends of the rows over step windows, per member.  rows [n_rows, N] or [S, n_rows, N] (fp32 / fp64
    ON THE GPU); steps [n_rows]: the model step each row holds, strictly increasing (they need not be evenly spaced: the fit
    uses each row's own step); windows: up to 4 step ranges [a, b); dt: years per model step.  One HIP pass forms sx and stx
    (one rounded fp64 add per row, in row order); the slope is then formed on the device in fp64 as
    ((n stx - su sx) / (n suu - su su)) / dt with n, su, suu exact integers of the stored steps inside the window (ValueError
    for suu >= 2^53).  Returns WindowTrends.  state: the result of an earlier call over earlier rows of the same members (same
    windows and dt, first new step after the last old one, else ValueError); the result is, bit for bit, that of one call over
    all the rows.  Runs on the current stream."""
    x = _device_rows(rows, "the trend sums")
    scen = rows.dim() == 3
    _, wn = _spec((), windows)
    dt = float(dt)
    if not dt > 0.0 or dt == float("inf"):
        raise ValueError(f"dt: want a positive number of years per step, got {dt}")
    S, K, N = x.shape
    st = _rowargs.model_steps(steps, K, non_negative=True)
    W = len(wn)
    dev = rows.device
    if state is not None:
        if not isinstance(state, WindowTrends) or state.windows != wn or state.dt != dt:
            raise ValueError("state: windows and dt must equal those of the call that made it")
        if tuple(state.sx.shape) != ((S, W, N) if scen else (W, N)) or state.sx.device != dev:
            raise ValueError(f"state: made for other rows ({tuple(state.sx.shape)} on {state.sx.device})")
        if K and state.steps.size and st[0] <= state.steps[-1]:
            raise ValueError(f"steps: the first new step {int(st[0])} does not lie after the state's last step {int(state.steps[-1])}")
    all_steps = st if state is None else np.concatenate([state.steps, st])
    moments = trend_moments(all_steps, wn)
    if any(suu >= 2 ** 53 for _, _, suu in moments):
        raise ValueError("windows: the sum of squared step offsets reaches 2^53 — not exact in fp64")
    x, ld, scen_stride = _rows_in_place(x)
    tsum = torch.empty((S, 2 * W, ld), dtype=torch.float64, device=dev)
    if state is not None and W:
        lead = (lambda t: t) if scen else (lambda t: t.unsqueeze(0))
        tsum[:, 0::2, :N], tsum[:, 1::2, :N] = lead(state.sx), lead(state.stx)
    if W:
        lib, capi, stream, guard = _lib_and_stream(rows)
        st32 = _rowargs.steps_i32(st, dev)
        c_wn = (ctypes.c_int32 * (2 * W))(*[v for ab in wn for v in ab])
        ptr = _rowargs.ptr
        _rowargs.call(lib, capi, "fiveeq_window_trends", rows.dtype, dev, S, K, N, ld, ptr(x) if K else None, scen_stride,
                      ptr(st32) if K else None, W, ctypes.cast(c_wn, ctypes.c_void_p), ptr(tsum), 1 if state is None else 0,
                      stream=stream, guard=guard)
    drop = (lambda t: t) if scen else (lambda t: t[0])
    sx, stx = drop(tsum[:, 0::2, :N]), drop(tsum[:, 1::2, :N])
    col = lambda i: torch.tensor([float(m[i]) for m in moments], dtype=torch.float64, device=dev).reshape(-1, 1)   # noqa: E731
    n, su, suu = col(0), col(1), col(2)
    slope = ((n * stx - su * sx) / (n * suu - su * su)) / dt
    slope = torch.where(n < 2.0, torch.full_like(slope, float("nan")), slope)
    return WindowTrends(sx=sx, stx=stx, count=tuple(m[0] for m in moments), mean=sx / n, slope=slope, steps=all_steps, windows=wn, dt=dt)
