"""Multi-GPU side of the engine: member sharding and the end-of-run summary exchange.

Ensemble members never interact, so the ensemble is cut into contiguous member ranges, one per
GPU / process, and time-stepping needs NO communication.  The only exchange is after the last
step: summary statistics of T (or C) at selected output times, over ALL members —
  * moments (count, mean, variance, min, max): each rank reduces its shard, the tiny per-rank
    records are all-gathered and merged with Chan's parallel-variance formula;
  * exact percentiles — one rank: a device sort of its rows; several ranks: by SELECTION, so that the ensemble does
    not have to travel: a 4096-bin histogram per output time
    between the global min and max is all-reduced (0.1 MB per rank for three output times), the bins
    holding the wanted order statistics are located on its cumulative counts, and only the members
    inside those bins travel to the root (a few thousand values out of 10M), where they are sorted
    and read off with NumPy's default linear interpolation.  Values keep their dtype on the wire.
The summary is four HIP passes over device rows (include/fiveeq.h "END-OF-RUN SUMMARY": moments, histogram with per-row
device ranges, selection with ballot counts and LDS compaction, radix pick) with the small bookkeeping between them done
on the host in NumPy — the rows are read three times at memory speed and nothing else of their size exists.  Rows on the
host are refused: there is no CPU path (a torch-ops restatement for tests: oracle/summary_host.py).
The unweighted summary (_device_summary) and the weighted one (gather_weighted_summary) are two short drivers over the same
stages, each a function below that a CPU test can call on its own: _histogram_stage, _selection_plan (with _pack_bin_mask),
_upload_plan, _select_and_pick (with _candidates_to_root), _first_lost and _fix_up.
`torch.distributed` backend "nccl" is RCCL on ROCm; tests/test_distributed.py runs the same host logic over gloo with the
passes replaced by their NumPy restatement.  The reference has no distributed code at all.
"""
import contextlib
import ctypes
import os
from fractions import Fraction

import numpy as np
import torch

from . import _capi            # (importing it binds nothing: the library is opened by _capi.load(), in _lib_and_stream)
from ._rowargs import int_weights


def shard_bounds(n_total, rank, world):
    """Contiguous, balanced member range [lo, hi) of `rank` (sizes differ by at most one)."""
    if not 0 <= rank < world:
        raise ValueError(f"rank {rank} outside 0..{world - 1}")
    base, extra = divmod(int(n_total), int(world))
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


# First-contact hook: with a process group of ONE rank the collectives below would all be skipped ("nothing to
# exchange").  force_collectives(True) — or FIVEEQ_FORCE_COLLECTIVES=1 in the environment — makes every one of them
# execute on the group's backend anyway, so that a one-GPU box can run the exact RCCL calls the multi-GPU summary makes
# (all_gather fp64, all_reduce SUM int64 / MIN / MAX fp64, gather of a device tensor with a receive list) before the
# first multi-GPU lease does (tests/test_distributed_gpu.py::test_rccl_first_contact_on_one_gpu).
_FORCE = [os.environ.get("FIVEEQ_FORCE_COLLECTIVES", "") == "1"]


def force_collectives(on=True):
    """Run the exchange's collectives even in a one-rank group (see above).  Returns the previous setting."""
    prev, _FORCE[0] = _FORCE[0], bool(on)
    return prev


def _dist(group):
    """(dist module or None, rank, world, exchange) — `exchange` says whether the collectives run: more than one rank,
    or a one-rank group with force_collectives on."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        world = dist.get_world_size(group)
        return dist, dist.get_rank(group), world, world > 1 or _FORCE[0]
    return None, 0, 1, False


def _comm_tensor(dist, group, x):
    """Collectives run where the backend can reach: device tensors over RCCL ("nccl"), host copies
    over gloo (CPU tests, and single-GPU rehearsals of the multi-process path)."""
    if dist is not None and dist.get_backend(group) == "gloo" and x.is_cuda:
        return x.cpu()
    return x


def merge_moments(parts):
    """parts [W, K, 5] -> [K, 5]: Chan et al. pairwise merge of (count, mean, M2), min/max."""
    out = parts[0].clone()
    for w in range(1, parts.shape[0]):
        b = parts[w]
        na, nb = out[:, 0], b[:, 0]
        n = na + nb
        delta = b[:, 1] - out[:, 1]
        mean = out[:, 1] + delta * nb / n
        m2 = out[:, 2] + b[:, 2] + delta * delta * na * nb / n
        out = torch.stack([n, mean, m2, torch.minimum(out[:, 3], b[:, 3]), torch.maximum(out[:, 4], b[:, 4])], dim=1)
    return out


def linear_positions(n, percentiles):
    """NumPy's 'linear' percentile rule, operation for operation (numpy/lib/_function_base_impl.py: the 'linear' entry of
    _QuantileMethods, _get_indexes, _get_gamma): for each percentile the two order-statistic indices (i0, i1) of an n-member
    row and the weight gamma.  Returns (i0 [P] int64, i1 [P] int64, gamma [P] float64) as NumPy arrays.  With `lerp` below the
    result is np.percentile's BIT FOR BIT (fp64 rows) once the order statistics are exact."""
    q = np.true_divide(np.asarray(percentiles, dtype=np.float64), 100)
    virtual = (n - 1) * q
    prev = np.floor(virtual)
    nxt = prev + 1.0
    above, below = virtual >= n - 1, virtual < 0
    prev[above], nxt[above] = -1.0, -1.0
    prev[below], nxt[below] = 0.0, 0.0
    gamma = virtual - prev                                   # (with prev = -1 above the bounds, like NumPy: both ends are the max then)
    i0, i1 = prev.astype(np.int64) % n, nxt.astype(np.int64) % n
    return i0, i1, gamma


def lerp(a, b, t):
    """numpy's _lerp: a + (b - a) t, and b - (b - a)(1 - t) where t >= 0.5 (NumPy arrays or torch tensors, broadcasting)."""
    d = b - a
    lo = a + d * t
    hi = b - d * (1.0 - t)
    if isinstance(lo, torch.Tensor):
        return torch.where(torch.as_tensor(t >= 0.5, device=lo.device).expand_as(lo), hi, lo)
    return np.where(np.broadcast_to(t >= 0.5, lo.shape), hi, lo)


def percentiles_sorted(xs, percentiles):
    """xs [K, n] sorted along dim 1 -> [K, len(percentiles)], NumPy 'linear' definition (bit for bit in fp64)."""
    i0, i1, gamma = linear_positions(xs.shape[1], percentiles)
    a = xs[:, torch.from_numpy(i0).to(xs.device)]
    b = xs[:, torch.from_numpy(i1).to(xs.device)]
    return lerp(a, b, torch.from_numpy(gamma).to(device=xs.device, dtype=xs.dtype).reshape(1, -1))


def moments_from_sums(sums):
    """sums [n, 5] = (count, sum, sum of squares, min, max) -> dict of [n] tensors."""
    cnt, s1, s2 = sums[:, 0], sums[:, 1], sums[:, 2]
    mean = s1 / cnt
    return {"count": cnt, "mean": mean, "var": (s2 / cnt - mean * mean).clamp_min(0.0), "min": sums[:, 3],
            "max": sums[:, 4]}


def reduce_stats(sums, group=None):
    """All-reduce the per-shard (count, sum, sum^2, min, max) records of every step over the ranks
    (three tiny collectives: SUM on the first three columns, MIN, MAX) and return the ensemble
    moments on every rank.  This is all a run without stored trajectories has to exchange."""
    dist, _, _, exchange = _dist(group)
    sums = _comm_tensor(dist, group, sums).clone()
    if exchange:
        add, mn, mx = sums[:, :3].contiguous(), sums[:, 3].contiguous(), sums[:, 4].contiguous()
        dist.all_reduce(add, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(mn, op=dist.ReduceOp.MIN, group=group)
        dist.all_reduce(mx, op=dist.ReduceOp.MAX, group=group)
        sums = torch.cat([add, mn[:, None], mx[:, None]], dim=1)
    return moments_from_sums(sums)


def histogram_percentiles(hist, lo, hi, percentiles=(5.0, 50.0, 95.0), group=None):
    """hist [K, n_bins] int64: this rank's fixed-bin counts (EnsembleEngine.T_histogram) with the SAME
    lo/hi/n_bins on every rank.  One all-reduce(SUM) of K*n_bins counters (24 MB for 750 steps x 4096
    bins) replaces gathering the members; percentiles are read off the cumulative counts with linear
    interpolation inside the bin, so the error is below one bin width w = (hi - lo)/n_bins for
    values inside [lo, hi).  Returns (percentiles [K, P] fp64, total counts [K]) on every rank."""
    dist, _, _, exchange = _dist(group)
    h = _comm_tensor(dist, group, hist).clone()
    if exchange:
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=group)
    n_bins = h.shape[1]
    w = (float(hi) - float(lo)) / n_bins
    cdf = torch.cumsum(h, dim=1).to(torch.float64)
    total = cdf[:, -1]
    cols = []
    for p in percentiles:
        target = (float(p) / 100.0) * total                              # members at or below the percentile
        b = torch.searchsorted(cdf, target[:, None].contiguous()).clamp_(max=n_bins - 1)[:, 0]
        below = torch.where(b > 0, cdf.gather(1, (b - 1).clamp_(min=0)[:, None])[:, 0], torch.zeros_like(total))
        inside = h.gather(1, b[:, None])[:, 0].to(torch.float64)
        frac = torch.where(inside > 0, (target - below) / inside.clamp_min(1.0), torch.zeros_like(total))
        cols.append(float(lo) + (b.to(torch.float64) + frac.clamp(0.0, 1.0)) * w)
    return torch.stack(cols, dim=1), total


SELECT_BINS = 4096


SELECT_CAND_BYTES = 4 << 30      # device summary: rows are summarised in halves while rows x candidates-per-row exceeds this


def _need_device_rows(rows):
    if not _passes_apply(rows):
        raise TypeError(f"rows must be fp32 / fp64 rows on a GPU (got {rows.dtype} on {rows.device}): the summary runs through the "
                        "HIP passes and has no CPU fallback; oracle/summary_host.py restates it in torch ops for the tests")


def exact_percentiles(rows, percentiles, gmin, gmax, n_total, dst=0, group=None, n_bins=SELECT_BINS, stats=None):
    """Exact percentiles (NumPy 'linear' definition) of device rows [K, n_local] over all ranks by histogram selection, with
    the global extrema gmin / gmax [K] and the member count n_total over all ranks handed in (no moments pass): see
    _device_summary.  Returns [K, P] fp64 (a host tensor) on rank `dst`, None elsewhere.  `stats`, if a dict, receives
    bytes_to_root / allreduce_bytes."""
    rows = rows.contiguous()
    _need_device_rows(rows)
    if len(percentiles) < 1:
        raise ValueError("no percentiles asked for")
    _, out = _device_summary(rows, percentiles, dst, group, stats, gmin=gmin, gmax=gmax, n_total=n_total, want_moments=False,
                             n_bins=n_bins)
    return None if out is None else torch.from_numpy(out)


# ---------------------------------------------------------------------------------------------------------------------
# The summary of DEVICE rows: HIP passes + host bookkeeping.
# ---------------------------------------------------------------------------------------------------------------------
def _lib_and_stream(rows):
    """(library, _capi, ctypes, stream) for rows on a GPU.  (tests/test_distributed.py replaces this function to run the host
    side of the summary on CPU tensors against the NumPy restatement of the passes, oracle/summary_passes.py.)"""
    lib = _capi.load()
    return lib, _capi, ctypes, ctypes.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream)


def _passes_apply(rows):
    """The summary of these rows goes through the four passes of the C ABI: fp32 / fp64 rows on a GPU."""
    return rows.is_cuda and rows.dtype in (torch.float32, torch.float64)


def _on(device):
    return torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext()


def _ptr(t, off=0):
    """Tensor `t`'s address plus `off` bytes, as the C ABI takes it."""
    return ctypes.c_void_p(t.data_ptr() + off)


def _all_reduce(dist, group, x, op):
    """all-reduce of a small device (or host) tensor over the group's backend; gloo takes device tensors through the host."""
    if dist.get_backend(group) == "gloo" and x.is_cuda:
        y = x.cpu()
        dist.all_reduce(y, op=op, group=group)
        x.copy_(y)
    else:
        dist.all_reduce(x, op=op, group=group)
    return x


def _all_gather_np(dist, group, world, arr, device):
    """every rank's NumPy array `arr` (same shape and dtype everywhere) -> array [world, ...], through the group's backend
    (RCCL moves device tensors: they go through `device`, the rank's GPU)."""
    t = torch.from_numpy(np.ascontiguousarray(arr))
    if dist.get_backend(group) != "gloo":
        t = t.to(device)
    parts = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(parts, t, group=group)
    return torch.stack(parts).cpu().numpy()


_EMPTY_ROW_SUMS = (0.0, 0.0, float("inf"), float("-inf"))    # (sum, sum of squares, min, max) of a row without members


def device_row_sums(rows, out=None):
    """rows [K, n] on the GPU -> device tensor [K, 4] fp64 = (sum, sum of squares, min, max) per row: ONE pass of
    fiveeq_row_moments_* (16-byte loads, fixed summation order: the same bits every run).  min / max ignore NaNs, the sums
    propagate them.  `out`: a [K, 4] fp64 device tensor to write into."""
    lib, _capi, ctypes, st = _lib_and_stream(rows)
    K, n = rows.shape
    if n == 0:                                         # an empty shard (fewer members than ranks): the neutral record
        if out is None:
            out = torch.empty((K, 4), dtype=torch.float64, device=rows.device)
        out.copy_(torch.tensor(_EMPTY_ROW_SUMS, dtype=torch.float64).expand(K, 4))
        return out
    chunks = int(lib.fiveeq_row_moments_chunks(K, n))
    work = torch.empty((K * chunks + (K if out is None else 0)) * 4, dtype=torch.float64, device=rows.device)
    if out is None:
        out = work[K * chunks * 4:].view(K, 4)
    fn = lib.fiveeq_row_moments_f64 if rows.dtype == torch.float64 else lib.fiveeq_row_moments_f32
    with _on(rows.device):
        _capi.check(lib, fn(K, n, rows.stride(0), ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(work.data_ptr()),
                            ctypes.c_void_p(out.data_ptr()), st))
    return out


# ---- the stages both summaries are made of -----------------------------------------------------------------------------
class _Run:
    """What the stages of ONE summary call share: the process group as _dist sees it, the library behind the switch
    (_lib_and_stream, looked up here, at call time), the rows' device, and the pass family ("" unweighted, "w" weighted)
    and dtype suffix that name its entry points."""

    def __init__(self, rows, group, family):
        self.dist, self.rank, self.world, self.exchange = _dist(group)
        self.lib, self.capi, _, self.st = _lib_and_stream(rows)
        self.group, self.dev, self.family = group, rows.device, family
        self.sfx = "f64" if rows.dtype == torch.float64 else "f32"
        self.host_wire = self.exchange and self.dist.get_backend(group) == "gloo"

    def launch(self, name, *args):
        """fiveeq_<family><name>_<f64|f32>(*args, stream); a failed pass raises.  (The caller is inside _on(self.dev).)"""
        self.capi.check(self.lib, getattr(self.lib, f"fiveeq_{self.family}{name}_{self.sfx}")(*args, self.st))

    def all_gather_np(self, arr):
        return _all_gather_np(self.dist, self.group, self.world, arr, self.dev)


def _alloc_head(K, n_bins, rec_words, dev):
    """ONE zeroed device buffer for everything that comes back after the histogram: the per-bin counts [K, n_bins] int64, then
    the moments pass's records [K, rec_words] of 8-byte words.  Returns (head, counts, records), the last two views."""
    head = torch.zeros(K * n_bins + K * rec_words, dtype=torch.int64, device=dev)
    return head, head[:K * n_bins].view(K, n_bins), head[K * n_bins:].view(K, rec_words)


def _histogram_stage(run, rows, weights, ranges, head, counts, stats):
    """Pass 2 and what follows it at once: the ranged histogram of this rank's rows into `counts` (the weight per bin when
    `weights` is given: integer sums, so the all-reduce is exact), the SUM all-reduce over the ranks, THE device-to-host copy
    of the summary's first half (`head`: counts and records together), and the initial `stats`.  Returns (counts [K, n_bins]
    int64, records [K, rec_words] int64) as NumPy views of that one copy."""
    K, n_bins = counts.shape
    n_local = rows.shape[1]
    if n_local > 0:
        with _on(run.dev):
            run.launch("hist_rows_ranged", K, n_local, rows.stride(0), _ptr(rows), *(() if weights is None else (_ptr(weights),)),
                       _ptr(ranges), n_bins, _ptr(counts))
    if run.exchange:
        _all_reduce(run.dist, run.group, counts, run.dist.ReduceOp.SUM)
    head_np = head.cpu().numpy()
    if stats is not None:
        stats["bytes_to_root"], stats["allreduce_bytes"] = 0, (counts.numel() * 8 if run.exchange else 0)
        stats["bytes_to_root_per_rank"] = [0] * run.world
    return head_np[:K * n_bins].reshape(K, n_bins), head_np[K * n_bins:].reshape(K, -1)


def _pack_bin_mask(marked):
    """marked [K, n_bins] bool -> [K, ceil(n_bins / 32)] uint32, bin b in bit b % 32 of word b // 32: what the selection
    passes read."""
    K, n_bins = marked.shape
    words = (n_bins + 31) // 32
    bits = np.zeros((K, words * 32), dtype=np.uint8)
    bits[:, :n_bins] = marked
    return np.packbits(bits.reshape(K, words, 32), axis=2, bitorder="little").view(np.uint32).reshape(K, words)


def _selection_plan(counts, cum, want, side, skip, fill):
    """The host step between the histogram and the selection.  counts / cum [K, n_bins] int64: members (or weight) per bin
    over all ranks and the running sum; want [Q] (shared) or [K, Q]: cumulative positions to find; skip [K]: rows that need
    no selection.  Position v lies in the first bin b with cum[b] > v (side "right": v is a 0-based member index) or with
    cum[b] >= v (side "left": v is a cumulative weight to reach); the last bin if there is none.  Those bins are marked and
    their members are the CANDIDATES.  Returns (pos [K, Q] int64: each position counted among the candidates alone — what
    the marked bins below b hold, plus v less what ALL bins below b hold —, `fill` in a skipped row; n_cand [K]: what the
    marked bins hold; the packed mask of _pack_bin_mask; a skipped row marks nothing)."""
    K, n_bins = counts.shape
    want = np.asarray(want)
    bb = np.stack([np.searchsorted(cum[k], want[k] if want.ndim == 2 else want, side=side) for k in range(K)])
    bb = bb.clip(max=n_bins - 1)                                                            # [K, Q]
    bb[skip] = 0
    rk = np.arange(K)[:, None]
    marked = np.zeros((K, n_bins), dtype=bool)
    marked[rk, bb] = True
    marked[skip] = False
    zero = np.zeros((K, 1), dtype=np.int64)
    held = counts * marked
    below_bin = np.concatenate([zero, cum[:, :-1]], axis=1)                                 # in bins < b
    cand_below = np.concatenate([zero, np.cumsum(held, axis=1)[:, :-1]], axis=1)            # in MARKED bins < b
    pos = cand_below[rk, bb] + (want - below_bin[rk, bb])
    pos[skip] = fill
    return pos.astype(np.int64), held.sum(axis=1), _pack_bin_mask(marked)


def _upload_plan(pos, binmask, dev):
    """THE upload of a summary: the positions [K, Q] int64, then the bin masks [K, words] uint32, in one device buffer.
    Returns (buffer, byte offset of the masks)."""
    up = torch.from_numpy(np.concatenate([pos.reshape(-1).view(np.uint8), binmask.reshape(-1).view(np.uint8)])).to(dev)
    return up, pos.size * 8


def _candidates_to_root(run, cands, cand_n, cap, cand_bytes, dst, stats):
    """Several ranks: the candidates travel to rank `dst` (a few thousand values out of the ensemble).  cands: this rank's
    candidate tensors [Kb, cap] (values; then their weights), cand_n [Kb] how many of each row it found.  The counts are
    all-gathered, every tensor is cut or zero-padded to the widest row of any rank and gathered, one collective per tensor in
    list order; `stats` counts cand_bytes per candidate that is not the root's own.  Returns (all_n [world, Kb], width, and
    on `dst` — else None, None — the pools [Kb, world, width], one per tensor, and seg_n [Kb, world], on the device)."""
    Kb = cand_n.shape[0]
    all_n = run.all_gather_np(cand_n)
    width = max(int(all_n.max()), 1)
    send = []
    for t in cands:
        t = t[:, :min(width, cap)]
        if t.shape[1] < width:
            t = torch.cat([t, t.new_zeros((Kb, width - t.shape[1]))], dim=1)
        t = t.contiguous()
        send.append(t.cpu() if run.host_wire else t)
    recv = [[torch.empty_like(t) for _ in range(run.world)] if run.rank == dst else None for t in send]
    for t, r in zip(send, recv):
        run.dist.gather(t, r, dst=dst, group=run.group)
    if stats is not None:
        per_rank = [0 if r == dst else int(all_n[r].sum()) * cand_bytes for r in range(run.world)]
        stats["bytes_to_root"] += sum(per_rank)
        stats["bytes_to_root_per_rank"] = [a + b for a, b in zip(stats["bytes_to_root_per_rank"], per_rank)]
    if run.rank != dst:
        return all_n, width, None, None
    pools = [torch.stack(r, dim=1).to(run.dev).contiguous() for r in recv]
    return all_n, width, pools, torch.from_numpy(np.ascontiguousarray(all_n.T)).to(run.dev)


def _select_and_pick(run, rows, weights, ranges, up, t_off, m_off, k0, k1, n_targets, n_bins, cap, dst, stats):
    """Passes 3 and 4 for rows k0..k1: the selection pass compacts this rank's members of the marked bins (with their weights
    when `weights` is given) into candidate buffers of `cap` per row; one rank: the pick pass selects the wanted positions
    among them; several: the candidates travel (_candidates_to_root) and the root's pick pass runs over one segment per rank.
    up / t_off / m_off: the uploaded plan and the byte offsets of these rows' positions and masks in it.  Ends with the
    device-to-host copy of tail = [cand_n Kb (uint64) | picked Kb * n_targets (fp64)].  Returns (candidates found per row over
    all ranks [Kb], picked [Kb, n_targets] fp64) as NumPy arrays — (None, None) on a rank that is not `dst`."""
    Kb, n_local, ld, w_el = k1 - k0, rows.shape[1], rows.stride(0), rows.element_size()
    wts = () if weights is None else (_ptr(weights),)
    tail = torch.zeros(Kb + Kb * n_targets, dtype=torch.int64, device=run.dev)
    cands = [torch.empty((Kb, cap), dtype=dt, device=run.dev) for dt in (rows.dtype, torch.int64)[:1 + len(wts)]]
    with _on(run.dev):
        if n_local > 0:
            run.launch("select_bins", Kb, n_local, ld, _ptr(rows, k0 * ld * w_el), *wts, _ptr(ranges, k0 * 16), n_bins,
                       _ptr(up, m_off), *map(_ptr, cands), cap, _ptr(tail))
        if not run.exchange:
            run.launch("select_pick", Kb, 1, cap, *map(_ptr, cands), _ptr(tail), n_targets, _ptr(up, t_off), _ptr(tail, Kb * 8))
    if run.exchange:
        all_n, width, pools, seg_n = _candidates_to_root(run, cands, tail[:Kb].cpu().numpy(), cap, w_el + 8 * len(wts), dst, stats)
        if pools is None:
            return None, None
        with _on(run.dev):
            run.launch("select_pick", Kb, run.world, width, *map(_ptr, pools), _ptr(seg_n), n_targets, _ptr(up, t_off),
                       _ptr(tail, Kb * 8))
    tail_np = tail.cpu().numpy()                          # one rank: THE second (and last) device-to-host copy
    return all_n.sum(axis=0) if run.exchange else tail_np[:Kb], tail_np[Kb:].view(np.float64).reshape(Kb, n_targets)


def _first_lost(cols, lo, hi, skip):
    """The sanity check of the pick: in every row that went through the selection, lo <= cols[0] <= cols[1] <= ... <= hi must
    hold (cols: [K, P] arrays of picked values; a NaN fails).  Returns (row, column) of the first failure, or None."""
    chain = [lo[:, None], *cols, hi[:, None]]
    with np.errstate(invalid="ignore"):
        good = chain[0] <= chain[1]
        for a, b in zip(chain[1:], chain[2:]):
            good &= a <= b
    good |= skip[:, None]
    return None if good.all() else tuple(int(v) for v in np.argwhere(~good)[0])


def _fix_up(values, lo, nan_row, flat):
    """The rows the selection skipped: a row holding a NaN is NaN (like np.percentile), a constant row is its one value."""
    return np.where(nan_row[:, None], np.nan, np.where(flat[:, None], np.broadcast_to(lo[:, None], values.shape), values))


# ---- the unweighted summary ---------------------------------------------------------------------------------------------
def _merge_sum_records(parts):
    """parts [R, K, 5]: per rank and row (member count, sum, sum of squares, min, max) -> [K, 5] fp64 (count, mean, M2, min,
    max) over the ranks, merged in rank order (merge_moments).  Ranks whose shard is empty take no part."""
    rec = parts[parts[:, 0, 0] > 0]                          # (a copy: the sums become mean and M2 in place)
    if rec.shape[0] == 0:
        raise ValueError("gather_summary: no members on any rank")
    cnt, mean_r = rec[:, :, 0], rec[:, :, 1]
    mean_r /= cnt
    with np.errstate(invalid="ignore", over="ignore"):       # a row with an infinite member: its moments are inf / nan, quietly
        rec[:, :, 2] = np.maximum(rec[:, :, 2] - cnt * mean_r * mean_r, 0.0)
    return rec[0] if rec.shape[0] == 1 else merge_moments(torch.from_numpy(rec)).numpy()      # (one record: nothing to merge)


def _with_count(n_local, sums):
    """sums [K, 4] NumPy -> this rank's record [K, 5] for _merge_sum_records."""
    return np.concatenate([np.full((sums.shape[0], 1), float(n_local)), sums], axis=1)


def _moments_and_ranges(run, rows, sums_dev, local_sums, gmin, gmax, n_total, want_moments):
    """Pass 1 of the unweighted summary: this rank's (sum, sum of squares, min, max) into sums_dev [K, 4] — from local_sums
    when the caller has them, not at all when it brought the extrema and wants no moments — and the histogram's ranges.
    Several ranks all-gather and merge the records here; one rank leaves them on the device (they come back with the
    histogram) unless the extrema were handed in.  Returns (mom [K, 5] or None, lo [K] or None, hi [K] or None, ranges [K, 2]
    fp64 on the device, the member count over all ranks); lo is None exactly when moments and extrema are still to come."""
    K, n_local = rows.shape
    have_sums = gmin is None or want_moments
    if have_sums:
        if local_sums is not None:
            sums_dev.copy_(local_sums.to(device=run.dev, dtype=torch.float64))
        else:
            device_row_sums(rows, out=sums_dev)
    if not run.exchange and gmin is None:
        return None, None, None, sums_dev[:, 2:4].contiguous(), n_local      # the extrema never leave the device before the histogram
    mom = None
    if have_sums:
        mine = _with_count(n_local, sums_dev.cpu().numpy())
        mom = _merge_sum_records(run.all_gather_np(mine) if run.exchange else mine[None])
    if gmin is None:
        lo, hi, n_tot = mom[:, 3].copy(), mom[:, 4].copy(), int(round(float(mom[0, 0])))
    else:
        lo, hi = (np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v, dtype=np.float64).reshape(K).copy()
                  for v in (gmin, gmax))
        n_tot = int(n_total)
    return mom, lo, hi, torch.from_numpy(np.stack([lo, hi], axis=1)).to(run.dev), n_tot


def _summary_in_halves(rows, percentiles, dst, group, stats, lo, hi, n_tot, n_bins):
    """One row with heavy ties would size the candidate buffer of EVERY row: the rows are summarised in two halves (the
    decision rests on the all-reduced histogram, so every rank takes it alike), each through _device_summary with the extrema
    and the member count handed in; a half may halve again.  Returns pct [K, P] on `dst`, None elsewhere."""
    K = rows.shape[0]
    h = K // 2
    half_stats = [None if stats is None else {} for _ in range(2)]
    halves = [_device_summary(rows[a:b], percentiles, dst, group, st_h, gmin=lo[a:b], gmax=hi[a:b], n_total=n_tot,
                              want_moments=False, n_bins=n_bins)[1] for (a, b), st_h in zip(((0, h), (h, K)), half_stats)]
    if stats is not None:
        # what travelled is what the halves sent (each half all-reduces its own histogram again: counted too)
        stats["split_rows"] = True
        stats["bytes_to_root"] = sum(st_h["bytes_to_root"] for st_h in half_stats)
        stats["allreduce_bytes"] += sum(st_h["allreduce_bytes"] for st_h in half_stats)
        stats["bytes_to_root_per_rank"] = [sum(v) for v in zip(*(st_h["bytes_to_root_per_rank"] for st_h in half_stats))]
    return None if halves[0] is None else np.concatenate(halves, axis=0)


def _device_summary(rows, percentiles, dst, group, stats, local_sums=None, gmin=None, gmax=None, n_total=None,
                    want_moments=True, n_bins=None):
    """Moments + exact percentiles of device rows [K, n_local] over all ranks.  Returns (mom [K, 5] NumPy fp64 =
    (count, mean, M2, min, max) merged over the ranks — None if want_moments is False —, pct [K, P] NumPy fp64 on rank `dst`
    else None).  local_sums: this rank's [K, 4] (sum, sum^2, min, max) when the caller already has them (the engine's
    in-kernel records); gmin / gmax / n_total: global extrema and member count when the caller already has THOSE
    (exact_percentiles' signature) — then no moments pass runs at all.

    The histogram between the global extrema holds EXACT counts and its bin rule is monotone in the value, so the order
    statistic of global index i is the (i - cdf[b-1])-th smallest member of the bin b with cdf[b-1] <= i < cdf[b].  Hence:
    _moments_and_ranges (moments pass; one rank: ranges straight from the moments, on the device) -> _histogram_stage
    (histogram pass and ONE device-to-host copy, moments + counts) -> _selection_plan (the host marks the bins that hold wanted
    order statistics and computes each statistic's rank among the members of marked bins; past SELECT_CAND_BYTES of
    candidates: _summary_in_halves) -> _upload_plan (ONE upload) -> _select_and_pick (selection pass: members of marked
    bins, compacted; pick pass: radix selection of those ranks; ONE copy back) -> _first_lost, _fix_up.  Several ranks add
    the exchanges where those stages say so."""
    run = _Run(rows, group, "")
    n_bins = SELECT_BINS if n_bins is None else int(n_bins)
    K, n_local = rows.shape
    P = len(percentiles)
    if P < 1:
        raise ValueError("no percentiles asked for")
    head, counts, rec_dev = _alloc_head(K, n_bins, 4, run.dev)
    mom, lo_np, hi_np, ranges, n_tot = _moments_and_ranges(run, rows, rec_dev.view(torch.float64), local_sums, gmin, gmax,
                                                           n_total, want_moments)
    counts_np, rec_np = _histogram_stage(run, rows, None, ranges, head, counts, stats)
    if lo_np is None:
        mom = _merge_sum_records(_with_count(n_local, rec_np.view(np.float64))[None])
        lo_np, hi_np = mom[:, 3].copy(), mom[:, 4].copy()
    cdf = np.cumsum(counts_np, axis=1)
    # a NaN member has no bin: a row whose counts do not add up to the member count holds one, and np.percentile of it is NaN
    nan_row = cdf[:, -1] != n_tot
    if n_tot < 1:
        raise ValueError("gather_summary: no members on any rank")
    i0, i1, frac = linear_positions(n_tot, percentiles)
    flat = ~(hi_np > lo_np)                              # a constant row: every member IS the answer, nothing to select
    skip = nan_row | flat
    ranks, n_cand, binmask = _selection_plan(counts_np, cdf, np.concatenate([i0, i1]), "right", skip, -1)     # [K, 2P]
    if K > 1 and K * int(n_cand.max()) * rows.element_size() > SELECT_CAND_BYTES:
        return mom, _summary_in_halves(rows, percentiles, dst, group, stats, lo_np, hi_np, n_tot, n_bins)
    cap = max(1, int(min(n_local, n_cand.max())))
    up, o_mask = _upload_plan(ranks, binmask, run.dev)
    tot_c, picked = _select_and_pick(run, rows, None, ranges, up, 0, o_mask, 0, K, 2 * P, n_bins, cap, dst, stats)
    if picked is None:
        return mom, None
    c0, c1 = picked[:, :P], picked[:, P:]
    # the selection pass must have found exactly the members the histogram counted in the marked bins (same rule, same ranges)
    if not np.array_equal(tot_c[~skip], n_cand[~skip]):
        k = int(np.argwhere((tot_c != n_cand) & ~skip)[0, 0])
        raise RuntimeError(f"percentile selection: row {k} has {int(tot_c[k])} candidates where the histogram counts {int(n_cand[k])}")
    lost = _first_lost((c0, c1), lo_np, hi_np, skip)
    if lost is not None:
        k, j = lost
        raise RuntimeError(f"percentile selection lost its order statistic (row {k}, p={percentiles[j]}): ranks "
                           f"{int(ranks[k, j])},{int(ranks[k, j + P])} of {int(tot_c[k])} candidates, values {c0[k, j]}, {c1[k, j]}")
    with np.errstate(invalid="ignore"):
        out = lerp(c0, c1, frac[None, :])
    return mom, _fix_up(out, lo_np, nan_row, flat)


def gather_summary(rows, percentiles=(5.0, 50.0, 95.0), dst=0, group=None, stats=None, local_sums=None):
    """rows [K, n_local] ON THE GPU: this rank's members at K output times.  Collective over `group`.
    Returns on every rank a dict with the merged moments (mean, var, min, max, count; [K] each, fp64, host tensors);
    on rank `dst` it also holds 'percentiles' [K, len(percentiles)] over ALL members (None elsewhere) —
    exact (np.percentile's 'linear' rule bit for bit), found by selection through the four HIP passes (_device_summary).
    `stats` (dict) receives 'bytes_to_root' (candidate members the root received) and 'allreduce_bytes' (the histogram).
    `local_sums` [K, 4] = this rank's (sum, sum of squares, min, max) per row spares the moments pass when the caller already
    has those — the engine's in-kernel records, EnsembleEngine.gather_summary."""
    rows = rows.contiguous()
    _need_device_rows(rows)
    mom_np, pct_np = _device_summary(rows, percentiles, dst, group, stats, local_sums=local_sums)
    mom = torch.from_numpy(mom_np)           # a few numbers per row: they stay on the host
    return {"count": mom[:, 0].clone(), "mean": mom[:, 1].clone(), "var": mom[:, 2] / mom[:, 0], "min": mom[:, 3].clone(),
            "max": mom[:, 4].clone(), "percentiles": None if pct_np is None else torch.from_numpy(pct_np)}


# ---------------------------------------------------------------------------------------------------------------------
# The WEIGHTED summary: integer importance weights, exact weighted percentiles (include/fiveeq.h, "WEIGHTED SUMMARY").
# ---------------------------------------------------------------------------------------------------------------------
WMOM_WORDS = 8                   # 8-byte words per row record of fiveeq_wrow_moments_* (layout: include/fiveeq.h)


def _empty_weighted_records(K):
    """[K, WMOM_WORDS] int64: the neutral record of a shard without members (sums 0, min +inf, max -inf, no flags)."""
    rec = np.zeros((K, WMOM_WORDS), dtype=np.int64)
    rec[:, 3:5] = np.array([np.inf, -np.inf]).view(np.int64)
    return rec


def weighted_rank(p, weight_sum):
    """k_p = max(1, ceil(p / 100 * W)): the cumulative weight percentile p must reach, in exact rational arithmetic on the
    exact value of p (Fraction(p)) — a Python int."""
    f = Fraction(p)
    if not 0 <= f <= 100:
        raise ValueError(f"percentile {p} outside [0, 100]")
    k = f * int(weight_sum) / 100
    return max(1, -((-k.numerator) // k.denominator))


def _weighted_plan(counts_np, cumw, W, percentiles, skip):
    """The host step between the weighted histogram and the selection.  counts_np / cumw [K, n_bins] int64: the weight per
    bin over all ranks and its running sum; W their total; skip [K]: rows that need no selection.  Returns (targets [K, P]
    int64, binmask [K, ceil(n_bins / 32)] uint32): per row the bins that hold a k_p, marked, and per percentile the
    cumulative weight to reach AMONG THE CANDIDATES (the members of marked bins, ascending): the weight of the marked bins
    below its bin plus k_p minus the weight of all bins below it — at least 1; 0 for a skipped row.  (_selection_plan with
    the k_p of weighted_rank as the positions.)"""
    kp = np.array([weighted_rank(p, W) for p in percentiles], dtype=np.int64)               # [P]
    targets, _, binmask = _selection_plan(counts_np, cumw, kp, "left", skip, 0)
    return targets, binmask


def _weighted_moments_dev(lib, _capi, ctypes, st, rows, weights, out):
    """fiveeq_wrow_moments_* of this rank's rows into `out` (a [K, 8] view of 8-byte words on the rows' device)."""
    K, n = rows.shape
    if n == 0:                                             # an empty shard: the neutral record
        out.copy_(torch.from_numpy(_empty_weighted_records(K)))
        return
    chunks = int(lib.fiveeq_wrow_moments_chunks(K, n))
    work = torch.empty(K * chunks * WMOM_WORDS, dtype=torch.float64, device=rows.device)
    fn = lib.fiveeq_wrow_moments_f64 if rows.dtype == torch.float64 else lib.fiveeq_wrow_moments_f32
    with _on(rows.device):
        _capi.check(lib, fn(K, n, rows.stride(0), ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(weights.data_ptr()),
                            ctypes.c_void_p(work.data_ptr()), ctypes.c_void_p(out.data_ptr()), st))


def _weighted_records_and_ranges(run, rows, weights, rec_dev):
    """Pass 1 of the weighted summary: this rank's records into rec_dev [K, WMOM_WORDS], and with them the extrema over the
    members that carry weight.  Several ranks all-gather the records (with the member count behind them).  Returns (every
    rank's records [world, K, WMOM_WORDS] int64 — None for one rank: they come back with the histogram —, members per rank,
    the histogram's ranges [K, 2] fp64 on the device)."""
    K, n_local = rows.shape
    _weighted_moments_dev(run.lib, run.capi, ctypes, run.st, rows, weights, rec_dev)
    if not run.exchange:
        # one rank: the extrema never leave the device here
        return None, np.array([n_local], dtype=np.int64), rec_dev[:, 3:5].view(torch.float64).contiguous()
    mine = np.concatenate([rec_dev.cpu().numpy().reshape(-1), np.array([n_local], dtype=np.int64)])
    got = run.all_gather_np(mine)                                                           # [world, K * 8 + 1]
    parts = got[:, :-1].reshape(run.world, K, WMOM_WORDS)
    f = parts[:, :, :5].view(np.float64)
    ranges = torch.from_numpy(np.ascontiguousarray(np.stack([f[:, :, 3].min(axis=0), f[:, :, 4].max(axis=0)], axis=1)))
    return parts, got[:, -1], ranges.to(run.dev)


def _merge_weighted_records(parts, n_each):
    """parts [R, K, WMOM_WORDS] int64: every rank's records; n_each [R]: its members.  The argument checks that need all
    ranks (member count, weight range, weight sum), then the merge, in rank order: the same bits every run.  Returns (the
    summary's dict without percentiles, W the weight sum, n_pos [R] members with w > 0 per rank, lo [K], hi [K], nan_row
    [K])."""
    K = parts.shape[1]
    n_total = int(n_each.sum())
    if n_total >= (1 << 31):
        raise ValueError(f"weighted summary: {n_total} members over all ranks; integer weights need fewer than 2^31")
    flags = np.bitwise_or.reduce(parts[:, :, 6], axis=0)                                    # [K]
    if (flags & 2).any():
        raise ValueError("weights: values outside [0, 2^32]")
    W = sum(int(v) for v in parts[:, 0, 7])                                                 # the weights are shared by the rows
    if W == 0:
        raise ValueError("weighted summary: the weights of all members on all ranks sum to 0")
    n_pos = parts[:, 0, 5].astype(np.int64)                                                 # members with w > 0, per rank
    fp = parts[:, :, :5].view(np.float64)
    s1, s2, sw2 = np.zeros(K), np.zeros(K), 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(parts.shape[0]):
            s1, s2, sw2 = s1 + fp[r, :, 0], s2 + fp[r, :, 1], sw2 + float(fp[r, 0, 2])
        lo_np, hi_np = fp[:, :, 3].min(axis=0), fp[:, :, 4].max(axis=0)
        mean = s1 / float(W)
        var = np.maximum(s2 / float(W) - mean * mean, 0.0)                                  # (NaN stays NaN)
    nan_row = (flags & 1) != 0
    mean, var = np.where(nan_row, np.nan, mean), np.where(nan_row, np.nan, var)
    out = {"count": torch.full((K,), float(n_pos.sum()), dtype=torch.float64), "mean": torch.from_numpy(mean),
           "var": torch.from_numpy(var), "std": torch.from_numpy(np.sqrt(var)), "min": torch.from_numpy(lo_np.copy()),
           "max": torch.from_numpy(hi_np.copy()), "weight_sum": W, "ess": float(W) * float(W) / sw2,
           "method": "weighted_inverted_cdf", "percentiles": None}
    return out, W, n_pos, lo_np, hi_np, nan_row


def gather_weighted_summary(rows, weights, percentiles=(5.0, 50.0, 95.0), dst=0, group=None, stats=None, n_bins=None):
    """rows [K, n_local] ON THE GPU with this rank's integer weights [n_local] (int64 on the same device, 0..2^32 each:
    constrain.importance_weights, or the caller's own).  Collective over `group`.  The definition is include/fiveeq.h's
    "WEIGHTED SUMMARY": percentile p = the smallest x whose cumulative weight reaches k_p = weighted_rank(p, W) — exact, and
    the same bits for every world size and shard split, because every sum that decides it is an integer sum.
    Returns on every rank a dict: count (members with w > 0), mean, var, std, min, max ([K] fp64 host tensors), weight_sum
    (Python int), ess (float), method; on rank `dst` also 'percentiles' [K, P] fp64 (None elsewhere).
    Flow: _weighted_records_and_ranges (moments pass, all-gather of the records) -> _histogram_stage (weighted histogram
    between the global extrema, all-reduce SUM int64, the one download) -> _merge_weighted_records -> _weighted_plan (the host
    marks the bins holding each k_p) -> _upload_plan -> per block of rows _select_and_pick (selection of (value, weight)
    pairs, gather to `dst`, pick) -> _first_lost, _fix_up.
    A rank whose members all weigh 0, or that has none, takes part in every collective."""
    if rows.dim() != 2:
        raise ValueError("rows: want [K, n_local]")
    if rows.shape[1] > 0 and (rows.stride(1) != 1 or rows.stride(0) < rows.shape[1]):      # rows of a wider buffer are read in place
        rows = rows.contiguous()
    _need_device_rows(rows)
    weights = int_weights(weights, rows.shape[1], rows.device, check_range=False).contiguous()
    P = len(percentiles)
    if P < 1:
        raise ValueError("no percentiles asked for")
    for p in percentiles:
        weighted_rank(p, 1)                               # the range check, before anything is launched
    run = _Run(rows, group, "w")
    n_bins = SELECT_BINS if n_bins is None else int(n_bins)
    K = rows.shape[0]
    head, counts, rec_dev = _alloc_head(K, n_bins, WMOM_WORDS, run.dev)
    parts, n_each, ranges = _weighted_records_and_ranges(run, rows, weights, rec_dev)
    counts_np, rec_np = _histogram_stage(run, rows, weights, ranges, head, counts, stats)
    out, W, n_pos, lo_np, hi_np, nan_row = _merge_weighted_records(rec_np[None] if parts is None else parts, n_each)

    cumw = np.cumsum(counts_np, axis=1)                                                     # int64: W < 2^63
    flat = ~(hi_np > lo_np)                               # one value carries all the weight: it IS every percentile
    skip = nan_row | flat
    if not np.array_equal(cumw[~nan_row, -1], np.full(int((~nan_row).sum()), W, dtype=np.int64)):
        k = int(np.argwhere((cumw[:, -1] != W) & ~nan_row)[0, 0])
        raise RuntimeError(f"weighted summary: row {k}'s histogram weighs {int(cumw[k, -1])} where the weights sum to {W}")
    targets, binmask = _weighted_plan(counts_np, cumw, W, percentiles, skip)
    up, o_mask = _upload_plan(targets, binmask, run.dev)

    # The weighted histogram does not count members, so a row's candidate buffer is sized by this rank's members with w > 0
    # (most members of a tightly constrained ensemble weigh 0); rows go in blocks while rows x that bound (the largest over
    # the ranks: every rank blocks alike) exceeds SELECT_CAND_BYTES
    cap = max(1, int(n_pos[run.rank if run.exchange else 0]))
    block = max(1, min(K, SELECT_CAND_BYTES // (max(1, int(n_pos.max())) * (rows.element_size() + 8))))
    picked = np.full((K, P), np.nan)
    for k0 in range(0, K, block):
        k1 = min(K, k0 + block)
        _, got = _select_and_pick(run, rows, weights, ranges, up, k0 * P * 8, o_mask + k0 * binmask.shape[1] * 4, k0, k1, P,
                                  n_bins, cap, dst, stats)
        if got is not None:
            picked[k0:k1] = got
    if run.exchange and run.rank != dst:
        return out
    lost = _first_lost((picked,), lo_np, hi_np, skip)
    if lost is not None:
        k, j = lost
        raise RuntimeError(f"weighted selection lost its percentile (row {k}, p={percentiles[j]}): target {int(targets[k, j])}, "
                           f"picked {picked[k, j]}")
    out["percentiles"] = torch.from_numpy(_fix_up(picked, lo_np, nan_row, flat))
    return out
