"""Per-member trajectory metrics of stored T rows — what an overshoot scenario is judged by: how high each member peaks and
when, when it first crosses a warming level and for how many stored steps it stays at or above it, means over step windows
(2081-2100), and with what (posterior-weighted) probability a level is exceeded.

    m = trajectory_metrics(eng.T, eng.out_steps, levels=(1.5, 2.0), windows=((231, 251),))    # or eng.trajectory_metrics(...)
    crossed, total = exceedance(m.first)[0]                                                   # exact integers over all ranks
    s = crossing_summary(m.first[0], years, (5, 50, 95))                                      # conditional on crossing

One streaming HIP pass over the rows (include/fiveeq.h, "TRAJECTORY METRICS"; csrc/fiveeq_metrics.hpp) folds all metrics at
once; every result is an integer or an fp64 sum in row order, so the bits do not depend on the launch shape, on how the rows
are split into calls (`state=`) or on how the members are split into shards.  Device rows only: there is no CPU path
(_metrics_host.py is the NumPy twin the CPU tests put behind the same switch).
"""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _rowargs


def _lib_and_stream(rows):
    """(library, _capi, stream, device guard) for rows on a GPU.  (_metrics_host.host_passes() replaces this function and the
    next.)"""
    from . import _capi
    lib = _capi.load()
    return lib, _capi, ctypes.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream), torch.cuda.device(rows.device)


def _passes_apply(rows):
    return rows.is_cuda and rows.dtype in (torch.float32, torch.float64)


@dataclass
class TrajectoryMetrics:
    """The result of trajectory_metrics: tensors on the rows' device, [N] per member ([S, N] with a scenario axis; level and
    window axes come before N).  t_peak / first hold model steps (entries of `steps`), -1 for "never" (an all-NaN member has
    no peak; a member that never reaches a level has no first).  window_mean is wsum over the number of stored steps inside the
    window — NaN for a window that holds none."""
    peak: torch.Tensor            # fp64
    t_peak: torch.Tensor          # int32
    first: torch.Tensor           # int32 [L, N]
    n_above: torch.Tensor         # int32 [L, N]
    n_nan: torch.Tensor           # int32
    wsum: torch.Tensor            # fp64 [W, N]
    window_mean: torch.Tensor     # fp64 [W, N]
    steps: np.ndarray             # int64: every step folded so far
    levels: tuple
    windows: tuple


def _spec(levels, windows):
    from . import _capi
    lv = tuple(float(v) for v in levels)
    wn = tuple((int(a), int(b)) for a, b in windows)
    if len(lv) > _capi.MAX_LEVELS:
        raise ValueError(f"levels: {len(lv)} given, at most {_capi.MAX_LEVELS}")
    if len(wn) > _capi.MAX_WINDOWS:
        raise ValueError(f"windows: {len(wn)} given, at most {_capi.MAX_WINDOWS}")
    if any(v != v for v in lv):
        raise ValueError("levels: NaN")
    if any(a < 0 or a > b or b >= 2 ** 31 for a, b in wn):
        raise ValueError(f"windows: want step ranges [a, b) with 0 <= a <= b, got {wn}")
    return lv, wn


def _rows_in_place(x):
    """x [S, K, N] -> (x or its contiguous copy, ld, scen_stride).  The C ABI has ONE ld for the rows and the state blocks, so
    a narrow slice of a wide buffer (ld >= 2 N) is copied: read in place it would cost (3 + W + 2 L) state rows of ld words
    each, most of them padding.  The scenario axis is this pass's own: scenario blocks at least K ld apart."""
    S, K, N = x.shape
    ld = int(x.stride(1)) if K > 1 else N
    x, (ld,) = _rowargs.walk_in_place(x, N, first=1, copy=ld >= 2 * N or (S > 1 and K > 0 and x.stride(0) < K * ld))
    return x, ld, (int(x.stride(0)) if S > 1 and K > 0 else K * ld)


def trajectory_metrics(rows, steps, levels=(), windows=(), state=None):
    """rows [n_rows, N] or [S, n_rows, N] (fp32 / fp64 ON THE GPU; a column-sliced view of a buffer less than twice as wide is read in place, a narrower slice is copied),
    steps [n_rows]: the model step each row holds, strictly increasing.  levels: up to 8 values; windows: up to 4 step ranges
    [a, b).  Returns TrajectoryMetrics.  state: the result of an earlier call over earlier rows of the same members — the
    call continues it (same levels and windows, first new step after the last old one, else ValueError) and the result is, bit
    for bit, that of one call over all the rows.  Runs on the current stream."""
    if not isinstance(rows, torch.Tensor) or rows.dim() not in (2, 3):
        raise ValueError("rows: want a tensor [n_rows, N] or [S, n_rows, N]")
    if not _passes_apply(rows):
        raise TypeError(f"rows must be fp32 / fp64 rows on a GPU (got {rows.dtype} on {rows.device}): the metrics run through the "
                        "HIP kernel and have no CPU fallback")
    lv, wn = _spec(levels, windows)
    scen = rows.dim() == 3
    x = rows if scen else rows.unsqueeze(0)
    S, K, N = x.shape
    if N < 1:
        raise ValueError("rows: no members")
    st = _rowargs.model_steps(steps, K, non_negative=True)
    if state is not None:
        if not isinstance(state, TrajectoryMetrics) or state.levels != lv or state.windows != wn:
            raise ValueError("state: levels and windows must equal those of the call that made it")
        if tuple(state.peak.shape) != ((S, N) if scen else (N,)) or state.peak.device != rows.device:
            raise ValueError(f"state: made for other rows ({tuple(state.peak.shape)} on {state.peak.device})")
        if K and state.steps.size and st[0] <= state.steps[-1]:
            raise ValueError(f"steps: the first new step {int(st[0])} does not lie after the state's last step {int(state.steps[-1])}")
    x, ld, scen_stride = _rows_in_place(x)
    L, W = len(lv), len(wn)
    dev = rows.device
    fmet = torch.empty((S, 1 + W, ld), dtype=torch.float64, device=dev)
    imet = torch.empty((S, 2 + 2 * L, ld), dtype=torch.int32, device=dev)
    if state is not None:
        lead = (lambda t: t) if scen else (lambda t: t.unsqueeze(0))
        fmet[:, 0, :N], imet[:, 0, :N], imet[:, 1, :N] = lead(state.peak), lead(state.t_peak), lead(state.n_nan)
        if W:
            fmet[:, 1:, :N] = lead(state.wsum)
        if L:
            imet[:, 2:2 + L, :N], imet[:, 2 + L:, :N] = lead(state.first), lead(state.n_above)
    lib, capi, stream, guard = _lib_and_stream(rows)
    st32 = _rowargs.steps_i32(st, dev)
    c_lv = (ctypes.c_double * max(L, 1))(*lv)
    c_wn = (ctypes.c_int32 * max(2 * W, 1))(*[v for ab in wn for v in ab])
    ptr = _rowargs.ptr
    _rowargs.call(lib, capi, "fiveeq_traj_metrics", rows.dtype, dev, S, K, N, ld, ptr(x) if K else None, scen_stride,
                  ptr(st32) if K else None, L, ctypes.cast(c_lv, ctypes.c_void_p), W, ctypes.cast(c_wn, ctypes.c_void_p), ptr(fmet),
                  ptr(imet), 1 if state is None else 0, stream=stream, guard=guard)
    all_steps = st if state is None else np.concatenate([state.steps, st])
    counts = torch.tensor([int(np.count_nonzero((all_steps >= a) & (all_steps < b))) for a, b in wn], dtype=torch.float64, device=dev)
    drop = (lambda t: t) if scen else (lambda t: t[0])
    wsum = drop(fmet[:, 1:, :N])
    return TrajectoryMetrics(peak=drop(fmet[:, 0, :N]), t_peak=drop(imet[:, 0, :N]), first=drop(imet[:, 2:2 + L, :N]),
                             n_above=drop(imet[:, 2 + L:, :N]), n_nan=drop(imet[:, 1, :N]), wsum=wsum,
                             window_mean=wsum / counts.reshape(-1, 1), steps=all_steps, levels=lv, windows=wn)


def exceedance(first, weights=None, group=None):
    """first [L, n_local] int32 (TrajectoryMetrics.first of this rank's members).  Per level (crossed, total) as Python
    integers over ALL ranks of `group`: the number of members that reach the level among all members — or, with `weights`
    (int64 [n_local], 0..2^32 each: the contract of gather_summary(weights=)), the integer weight of those that do in the
    total weight.  Integer sums all-reduced as int64: P(exceed) = crossed / total is the same rational for every world size."""
    from .distributed import _all_reduce, _dist
    if first.dim() != 2:
        raise ValueError("first: want [L, n_local]")
    L, n = first.shape
    crossed = first >= 0
    if weights is None:
        acc = torch.cat([crossed.sum(dim=1, dtype=torch.int64), torch.tensor([n], dtype=torch.int64, device=first.device)])
    else:
        _rowargs.int_weights(weights, n, first.device, check_range=True)
        acc = torch.cat([(crossed.to(torch.int64) * weights.unsqueeze(0)).sum(dim=1), weights.sum().reshape(1)])
    dist, _, _, exchange = _dist(group)
    if exchange:
        _all_reduce(dist, group, acc, dist.ReduceOp.SUM)
    vals = [int(v) for v in acc.cpu().tolist()]
    return [(vals[l], vals[L]) for l in range(L)]


def crossing_summary(first_row, years, percentiles=(5.0, 50.0, 95.0), weights=None, accepted=None, dst=0, group=None):
    """Percentiles of the crossing YEAR of one level — CONDITIONAL ON CROSSING: over the members that reach the level only (how
    many do: exceedance()).  first_row [n_local] int32 = TrajectoryMetrics.first[l]; years: year of every model step
    (years[t], a sequence).  Collective over `group`.  Unweighted, the crossers (of `accepted`, a boolean mask, if given) are
    compacted and summarised by distributed.gather_summary; weighted, every member goes to gather_weighted_summary with
    weights * crossed — a weight of 0 drops a member.  Never-crossers are thus never encoded as a year (an infinite year
    would turn the interpolation into NaN and degenerate the histogram range).
    Returns the summary dict of the function used, plus 'crossed' (members, or integer weight, over all ranks); when nobody
    crosses, count is 0 and the percentiles (on rank `dst`) are NaN."""
    from .distributed import _dist, _all_reduce, gather_summary, gather_weighted_summary
    if first_row.dim() != 1:
        raise ValueError("first_row: want [n_local]")
    if weights is not None and accepted is not None:
        raise ValueError("crossing_summary: weights= and accepted= exclude each other (a weight of 0 drops a member)")
    dev = first_row.device
    yr = torch.as_tensor(np.asarray(years, dtype=np.float64), device=dev)
    crossed = first_row >= 0
    if accepted is not None:
        mask = _rowargs.bool_mask(accepted, crossed.shape[0], dev)
        crossed = crossed & mask
    if first_row.numel() and int(first_row.max()) >= yr.numel():
        raise ValueError("years: shorter than the steps in first_row")
    year_of = yr[first_row.clamp_min(0).long()] if first_row.numel() else yr[:0]
    if weights is None:
        w_eff = crossed.to(torch.int64)
    else:
        _rowargs.int_weights(weights, crossed.shape[0], dev, check_range=False)
        w_eff = weights * crossed.to(torch.int64)
    total = w_eff.sum().reshape(1)
    dist, rank, _, exchange = _dist(group)
    if exchange:
        _all_reduce(dist, group, total, dist.ReduceOp.SUM)
    total = int(total.item())
    P = len(percentiles)
    if total == 0:            # nobody crosses (or every crosser weighs 0): nothing to rank; the keys of the summary used, host
        nan = lambda: torch.full((1,), float("nan"), dtype=torch.float64)      # noqa: E731    tensors like its own
        out = {"count": torch.zeros(1, dtype=torch.float64), "mean": nan(), "var": nan(), "min": nan(), "max": nan(),
               "percentiles": torch.full((1, P), float("nan"), dtype=torch.float64) if rank == dst else None, "crossed": 0}
        if weights is not None:
            out.update(std=nan(), weight_sum=0, ess=float("nan"), method="weighted_inverted_cdf")
        return out
    if weights is None:
        out = gather_summary(year_of[crossed].reshape(1, -1).contiguous(), percentiles, dst=dst, group=group)
    else:
        out = gather_weighted_summary(year_of.reshape(1, -1).contiguous(), w_eff, percentiles, dst=dst, group=group)
    out["crossed"] = total
    return out
