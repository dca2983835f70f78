"""Constraining an ensemble against an observed temperature record (round 7).

Each member is scored against the record while it is stepped: the kernels carry three fp64 accumulators per member
(include/fiveeq.h, "CONSTRAINED RUNS"), so no historical T row has to be stored.  With T_t the member's T after step t:

    A = A + b_t T_t;   d = T_t - o_t;   pd = p_t d;   U = U + pd;   V = V + pd d        (steps with p_t = b_t = 0 skipped)

and the score of the baseline-corrected series is chi2 = V - 2 A U + A^2 P = sum_t p_t (T_t - mean_ref T - o_t)^2, P = sum_t p_t.
A run that STORED its rows is scored after the fact, against records of T or of any gas's concentration and in every mode, pool
layout and precision, by `score_rows` / EnsembleEngine.score (include/fiveeq.h, "SCORING STORED ROWS"): the same accumulators,
bit for bit.  Members are then kept by a threshold on chi2 or by rejection sampling, and the summaries are computed over the kept members
(EnsembleEngine.gather_summary(..., accepted=mask)).

    obs = Observations.from_years(run_years, obs_years, T_obs, sigma, baseline=(1850, 1900))
    eng = EnsembleEngine(params, N, E, observations=obs, ...);  eng.run(mode="auto")
    keep = accept_rejection(eng.chi2(), seed, m0, n_total, group)

or every member is kept and weighted by its likelihood (include/fiveeq.h, "WEIGHTED SUMMARY"):

    w = importance_weights(eng.chi2(), group);  eng.gather_summary(steps, weights=w)
"""
import hashlib
from dataclasses import dataclass

import numpy as np

ACCEPT_SEED = 0x0B5E47ED            # the rejection rule's default key: its uniforms are a dimension of their own LHS
W_ONE = 1 << 32                     # the integer weight of the best member (importance_weights); the largest weight a member may carry
MAX_WEIGHTED_MEMBERS = 1 << 31      # fewer members than this over all ranks: every sum of weights then fits int64


class Observations:
    """The shared observation table obs [n_steps, 4] fp64: per step (o_t, p_t = 1/sigma_t^2 or 0, b_t = 1/n_ref inside the
    reference period or 0, 0).  Build it with `from_years`; `table`, `P` (= sum p_t) and `sha256` (of the table's bytes).
    anomaly=False: a record of ABSOLUTE values (an observed concentration; `absolute` builds it) — no reference period, so
    every b_t must be 0; A then stays 0 and chi2 = V."""

    def __init__(self, table, anomaly=True):
        t = np.array(table, dtype=np.float64, order="C")
        if t.ndim != 2 or t.shape[1] != 4 or t.shape[0] < 1:
            raise ValueError(f"observation table: shape {t.shape}, want [n_steps, 4]")
        if not np.isfinite(t).all():
            raise ValueError("observation table: non-finite entries")
        if (t[:, 1] < 0).any() or (t[:, 2] < 0).any() or (t[:, 3] != 0).any():
            raise ValueError("observation table: weights must be >= 0 and column 3 zero")
        self.anomaly = bool(anomaly)
        if self.anomaly:
            if not t[:, 2].any():
                raise ValueError("observation table: empty baseline period")
        else:
            if t[:, 2].any():
                raise ValueError("observation table: anomaly=False takes no baseline period (every b_t must be 0)")
            if not t[:, 1].any():
                raise ValueError("observation table: no observation (every p_t is 0)")
        self.table = t
        self.table.setflags(write=False)
        self.P = float(np.sum(t[:, 1]))
        self.n_obs = int(np.count_nonzero(t[:, 1]))
        self.sha256 = hashlib.sha256(t.tobytes()).hexdigest()
        live = np.nonzero((t[:, 1] != 0) | (t[:, 2] != 0))[0]
        self.window = (int(live[0]), int(live[-1]) + 1)           # [first, last + 1) steps with a nonzero weight

    @property
    def n_steps(self):
        return int(self.table.shape[0])

    @property
    def live_steps(self):
        """The steps whose record is live (p_t != 0 or b_t != 0), increasing: the rows a score needs."""
        return np.nonzero((self.table[:, 1] != 0) | (self.table[:, 2] != 0))[0]

    @staticmethod
    def _match_years(run_years, obs_years, values, sigma, what, extra=()):
        """(run years, step of each observation, values, sigmas) after the checks from_years and absolute share."""
        ry = np.asarray(run_years, dtype=np.float64).reshape(-1)
        oy = np.asarray(obs_years, dtype=np.float64).reshape(-1)
        To = np.asarray(values, dtype=np.float64).reshape(-1)
        sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), oy.shape).copy()
        if To.shape != oy.shape:
            raise ValueError(f"{what} has {To.size} values for {oy.size} years")
        for name, v in (("run_years", ry), ("obs_years", oy), (what, To), ("sigma", sg)) + tuple(extra):
            if not np.isfinite(v).all():
                raise ValueError(f"{name}: non-finite values")
        if (sg <= 0).any():
            raise ValueError("sigma must be > 0")
        if ry.size > 1 and (np.diff(ry) <= 0).any():
            raise ValueError("run_years must increase")
        idx = np.searchsorted(ry, oy)
        ok = (idx < ry.size) & (ry[np.minimum(idx, ry.size - 1)] == oy)
        if not ok.all():
            raise ValueError(f"observation years {oy[~ok][:5].tolist()} are not steps of the run")
        if np.unique(idx).size != idx.size:
            raise ValueError("an observation year appears twice")
        return ry, idx, To, sg

    @classmethod
    def from_years(cls, run_years, obs_years, T_obs, sigma, baseline):
        """Match observations to the run's steps by year.  run_years [n_steps]: the year of each step (T after step t is the
        state at run_years[t]); obs_years / T_obs / sigma [n_obs]; baseline = (y0, y1), inclusive: the reference period
        whose mean T is subtracted from each member's series before it is compared (b_t = 1/n_ref on its steps)."""
        ry, idx, To, sg = cls._match_years(run_years, obs_years, T_obs, sigma, "T_obs",
                                           (("baseline", np.asarray(baseline, dtype=float)),))
        y0, y1 = (float(b) for b in baseline)
        ref = (ry >= y0) & (ry <= y1)
        n_ref = int(ref.sum())
        if n_ref == 0:
            raise ValueError(f"baseline ({y0}, {y1}) holds no step of the run")
        t = np.zeros((ry.size, 4), dtype=np.float64)
        t[idx, 0] = To
        t[idx, 1] = 1.0 / (sg * sg)
        t[ref, 2] = 1.0 / n_ref
        return cls(t)

    @classmethod
    def absolute(cls, run_years, obs_years, values, sigma):
        """A record of absolute values (an observed concentration), matched to the run's steps by year like from_years and
        under its checks: no baseline, b_t = 0 everywhere (anomaly=False)."""
        ry, idx, vals, sg = cls._match_years(run_years, obs_years, values, sigma, "values")
        if idx.size == 0:
            raise ValueError("values: no observation")
        t = np.zeros((ry.size, 4), dtype=np.float64)
        t[idx, 0] = vals
        t[idx, 1] = 1.0 / (sg * sg)
        return cls(t, anomaly=False)


def misfit_numpy(T_rows, table, acc=None):
    """The accumulators of section 1 in NumPy: T_rows [n_steps, N] (T after each step, any float dtype, widened exactly),
    table [n_steps, 4] -> [3, N] fp64, added onto `acc` if given.  Step order, each operation rounded on its own."""
    table = np.asarray(table, dtype=np.float64)
    T_rows = np.asarray(T_rows)
    out = np.zeros((3, T_rows.shape[1])) if acc is None else np.array(acc, dtype=np.float64)
    A, U, V = out[0], out[1], out[2]
    for t in range(T_rows.shape[0]):
        o, p, b = table[t, 0], table[t, 1], table[t, 2]
        if p == 0.0 and b == 0.0:
            continue
        Tw = T_rows[t].astype(np.float64)
        A[:] = A + b * Tw
        d = Tw - o
        pd = p * d
        U[:] = U + pd
        V[:] = V + pd * d
    return out


def chi2_from_misfit(misfit, P):
    """chi2 = V - 2 A U + A^2 P per member (NumPy array or torch tensor [3, N] -> [N])."""
    A, U, V = misfit[0], misfit[1], misfit[2]
    return V - 2.0 * A * U + A * A * P


# ---- scoring STORED rows (include/fiveeq.h, "SCORING STORED ROWS"; csrc/fiveeq_score.hpp) -----------------------------------
def _lib_and_stream(rows):
    """(library, _capi, stream, device guard) for rows on a GPU.  (_score_host.host_passes() replaces this function and the
    next.)"""
    import ctypes

    import torch

    from . import _capi
    lib = _capi.load()
    return lib, _capi, ctypes.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream), torch.cuda.device(rows.device)


def _passes_apply(rows):
    import torch
    return rows.is_cuda and rows.dtype in (torch.float32, torch.float64)


def score_rows(rows, steps, observations, acc=None):
    """The misfit accumulators of STORED rows against observed records — one streaming HIP pass, bit for bit what a run that
    carries the record in-loop (EnsembleEngine(observations=)) leaves in `misfit`, for rows of any run.
    rows [n_rows, N] with ONE Observations -> [3, N] fp64 (A, U, V);  rows [n_rows, n_q, N] with a sequence of n_q Observations
    (tables of equal n_steps; quantity j of the rows against record j) -> [n_q, 3, N].  rows: fp32 / fp64 ON THE GPU, read in
    place whenever the column stride is 1 (engine.T, engine.C and row / gas / member slices of them), copied otherwise.
    steps [n_rows]: the model step each row holds, strictly increasing and inside the tables.  Rows whose record is dead
    (p_t = b_t = 0) are neither read nor do their values matter.  acc: the result of an earlier call over EARLIER rows of the
    same members — the call continues a copy of it, and the result is that of one call over all the rows.  chi2 of quantity
    j: chi2_from_misfit(out[j], observations[j].P).  Runs on the current stream; there is no CPU path."""
    import torch

    from . import _rowargs
    single = isinstance(observations, Observations)
    recs = [observations] if single else list(observations)
    if not recs or not all(isinstance(o, Observations) for o in recs):
        raise ValueError("observations: want an Observations or a non-empty sequence of them")
    if not isinstance(rows, torch.Tensor) or rows.dim() != (2 if single else 3):
        raise ValueError("rows: want a tensor [n_rows, N] with one Observations, [n_rows, n_q, N] with a sequence of them")
    if not _passes_apply(rows):
        raise TypeError(f"rows must be fp32 / fp64 rows on a GPU (got {rows.dtype} on {rows.device}): the score runs through the "
                        "HIP kernel and has no CPU fallback")
    x = rows.unsqueeze(1) if single else rows
    K, Q, N = x.shape
    from . import _capi
    if Q != len(recs):
        raise ValueError(f"rows hold {Q} quantities, observations {len(recs)}")
    if not 1 <= Q <= _capi.MAX_SCORE_Q:
        raise ValueError(f"{Q} quantities: at most {_capi.MAX_SCORE_Q} per call")
    if N < 1:
        raise ValueError("rows: no members")
    n_steps = recs[0].n_steps
    if any(o.n_steps != n_steps for o in recs):
        raise ValueError(f"observations: tables of {[o.n_steps for o in recs]} steps, want equal n_steps")
    st = _rowargs.model_steps(steps, K, n_steps=n_steps)
    dev = rows.device
    out_shape = (3, N) if single else (Q, 3, N)
    if acc is None:
        misfit = torch.zeros((Q, 3, N), dtype=torch.float64, device=dev)
    else:
        if not isinstance(acc, torch.Tensor) or acc.dtype != torch.float64 or tuple(acc.shape) != out_shape or acc.device != dev:
            raise ValueError(f"acc: want an fp64 tensor of shape {list(out_shape)} on {dev}")
        misfit = acc.reshape(Q, 3, N).clone()
    x, (row_stride, q_stride) = _rowargs.walk_in_place(x, N)
    lib, capi, stream, guard = _lib_and_stream(rows)
    st32 = _rowargs.steps_i32(st, dev)
    obs = torch.from_numpy(np.stack([o.table for o in recs])).to(dev)          # [Q, n_steps, 4]
    ptr = _rowargs.ptr
    _rowargs.call(lib, capi, "fiveeq_score_rows", rows.dtype, dev, Q, K, N, ptr(x) if K else None, row_stride, q_stride,
                  ptr(st32) if K else None, ptr(obs), n_steps, ptr(misfit), N, stream=stream, guard=guard)
    return misfit[0] if single else misfit


@dataclass
class Score:
    """What EnsembleEngine.score returns.  Per record key ("T" or a gas index): misfit[key] [3, N] fp64 (A, U, V), chi2[key] [N]
    (chi2_from_misfit) and n_obs[key], the number of observations; total [N]: the chi2 added in the fixed order T, then the
    gases ascending — what accept_*, importance_weights and resample take."""
    misfit: dict
    chi2: dict
    total: object
    n_obs: dict


def accept_threshold(chi2, max_chi2):
    """Members with chi2 <= max_chi2 (a NaN score is rejected).  Member-local: the same mask for any shard split."""
    return chi2 <= float(max_chi2)


def _global_min(chi2, group):
    """min of chi2 over the shard and, when torch.distributed runs, over every rank of `group` (all-reduce MIN)."""
    import torch

    from .distributed import _all_reduce, _dist
    if isinstance(chi2, torch.Tensor):
        v = chi2[~torch.isnan(chi2)]
        local = float(v.min()) if v.numel() else float("inf")
    else:
        c = np.asarray(chi2, dtype=np.float64)
        c = c[~np.isnan(c)]
        local = float(c.min()) if c.size else float("inf")
    dist, _, _, exchange = _dist(group)
    if not exchange:
        return local
    # RCCL reduces device tensors only: the value travels on the rank's GPU there (gloo takes it through the host either way)
    if isinstance(chi2, torch.Tensor) and chi2.is_cuda:
        dev = chi2.device
    elif dist.get_backend(group) != "gloo":
        dev = torch.device("cuda", torch.cuda.current_device())
    else:
        dev = torch.device("cpu")
    x = torch.tensor([local], dtype=torch.float64, device=dev)
    _all_reduce(dist, group, x, dist.ReduceOp.MIN)
    return float(x[0])


def accept_rejection(chi2, seed, m0, n_total, group=None):
    """Rejection sampling on the likelihood exp(-chi2 / 2): keep member m iff u_m < exp(-(chi2_m - chi2_min) / 2), chi2_min
    the global minimum (all-reduce MIN over `group`), u_m the uniform of GLOBAL member index m (this shard holds members
    [m0, m0 + len(chi2)) of n_total) — one dimension of the Latin hypercube keyed by `seed` (params.lhs_rows; on the
    device its HIP twin, the same bits).  Collective over `group` when torch.distributed runs; the mask is the same for
    every world size and shard split.  A NaN score is rejected."""
    import torch

    from . import params
    n = int(chi2.shape[0])
    cmin = _global_min(chi2, group)
    if isinstance(chi2, torch.Tensor):
        if chi2.is_cuda and n > 0:
            u = params.lhs_rows_device(int(n_total), [0], int(m0), int(m0) + n, chi2.device, seed=int(seed))[0]
        else:                                                     # host scores, or an empty shard (fewer members than ranks)
            u = torch.from_numpy(params.lhs_rows(int(n_total), [0], int(m0), int(m0) + n, seed=int(seed))[0]).to(chi2.device)
        return u < torch.exp(-(chi2.to(torch.float64) - cmin) / 2.0)
    u = params.lhs_rows(int(n_total), [0], int(m0), int(m0) + n, seed=int(seed))[0]
    with np.errstate(invalid="ignore", over="ignore"):
        return u < np.exp(-(np.asarray(chi2, dtype=np.float64) - cmin) / 2.0)


def importance_weights(chi2, group=None):
    """Integer importance weights w_m = floor(W_ONE exp(-(chi2_m - chi2_min) / 2)), W_ONE = 2^32, chi2_min the global minimum
    (all-reduce MIN over `group`): the likelihood of every member instead of accept_rejection's coin flip on it.  int64 [N],
    a torch tensor on chi2's device or a NumPy array, like chi2.  The best member gets exactly W_ONE, a NaN score 0.
    Member-local and evaluated by ONE routine (NumPy's exp on the host, wherever the scores live), so a member gets the same
    weight for every shard split and world size.  Collective over `group` when torch.distributed runs (the minimum, and the
    member count: fewer than 2^31 members over all ranks, so that every sum of weights fits int64 — ValueError beyond)."""
    import torch

    from .distributed import _all_reduce, _dist
    n = int(chi2.shape[0])
    if n >= MAX_WEIGHTED_MEMBERS:
        raise ValueError(f"importance_weights: {n} members; integer weights need fewer than 2^31 over all ranks")
    cmin = _global_min(chi2, group)
    dist, _, _, exchange = _dist(group)
    if exchange:
        on_gpu = isinstance(chi2, torch.Tensor) and chi2.is_cuda
        dev = chi2.device if on_gpu else torch.device("cpu" if dist.get_backend(group) == "gloo" else f"cuda:{torch.cuda.current_device()}")
        total = torch.tensor([n], dtype=torch.int64, device=dev)
        _all_reduce(dist, group, total, dist.ReduceOp.SUM)
        if int(total[0]) >= MAX_WEIGHTED_MEMBERS:
            raise ValueError(f"importance_weights: {int(total[0])} members over all ranks; integer weights need fewer than 2^31")
    c = chi2.detach().to(torch.float64).cpu().numpy() if isinstance(chi2, torch.Tensor) else np.asarray(chi2, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        like = np.exp(-(c - cmin) / 2.0)                       # <= 1: cmin is the minimum; NaN for a NaN score
    w = np.floor(np.where(np.isnan(like), 0.0, np.minimum(like, 1.0)) * float(W_ONE)).astype(np.int64)   # exact: a power of two
    return torch.from_numpy(w).to(chi2.device) if isinstance(chi2, torch.Tensor) else w


# ---- resampling: (members, integer weights) -> a dense equal-weight posterior (include/fiveeq.h, "RESAMPLING") ------------
MAX_RESAMPLED = (1 << 31) - 1       # outputs over all ranks: int32 source indices, and j s + b < 2^62 on the device
_PER_MEMBER_KEYS = ("r0", "rC", "rT", "q", "f_scale", "fx_scale")


def resample_offset(seed, n_out, weight_sum):
    """The offset rho of the resampling positions: 0 without a seed, else the first 8 bytes (little-endian) of
    sha256("<seed>:<M>:<W>") modulo W — a pure function of its arguments, computed on the host."""
    if seed is None:
        return 0
    digest = hashlib.sha256(f"{seed}:{int(n_out)}:{int(weight_sum)}".encode()).digest()
    return int.from_bytes(digest[:8], "little") % int(weight_sum)


def resample_plan(local_sums, rank, n_out, rho):
    """The rank arithmetic of the resampling, in Python integers (no process group needed): local_sums = every rank's weight
    sum in rank order, rank = this one, n_out = M outputs over all ranks, 0 <= rho < W.  Returns a dict
      W, C_lo   the weight of all ranks, and of the ranks before this one
      j0, j1    this rank's outputs [j0, j1): j(C) = min(M, max(0, ceil((C M - rho) / W))) at C_lo and C_lo + its own sum
      q, a, s, b   W = q M + s, rho = a M + b: p_j = j q + a + (j s + b) div M stays inside int64 on the device."""
    sums = [int(v) for v in local_sums]
    M, rho, rank = int(n_out), int(rho), int(rank)
    if not 0 <= rank < len(sums):
        raise ValueError(f"rank {rank} outside 0..{len(sums) - 1}")
    if any(v < 0 for v in sums):
        raise ValueError("resample: negative weight sums")
    W = sum(sums)
    if W == 0:
        raise ValueError("resample: the weights of all members on all ranks sum to 0")
    if W >= 1 << 63:
        raise ValueError("resample: the weights sum to 2^63 or more")
    if not 1 <= M <= MAX_RESAMPLED:
        raise ValueError(f"resample: n_out={M} outside 1..2^31-1")
    if not 0 <= rho < W:
        raise ValueError(f"resample: offset {rho} outside [0, W={W})")
    C_lo = sum(sums[:rank])
    first = lambda C: min(M, max(0, -((rho - C * M) // W)))          # noqa: E731   ceil((C M - rho) / W)
    q, s = divmod(W, M)
    a, b = divmod(rho, M)
    return {"W": W, "C_lo": C_lo, "j0": first(C_lo), "j1": first(C_lo + sums[rank]), "q": q, "a": a, "s": s, "b": b}


class Resample:
    """What constrain.resample returns: this rank's share of the M equal-weight outputs.
      n_out       M, the outputs over all ranks          n_members   this rank's outputs — differs per rank and CAN BE 0
      j0          the global index of this rank's first output        n_source    this rank's source members
      weight_sum  W over all ranks (Python int)          offset      rho
      src         int32 [n_members] on the weights' device (a NumPy array for host weights): output k is a copy of this
                  rank's member src[k]; non-decreasing."""

    def __init__(self, n_out, j0, weight_sum, offset, src, n_source):
        self.n_out, self.j0, self.weight_sum, self.offset, self.src, self.n_source = n_out, j0, weight_sum, offset, src, n_source
        self.n_members = int(src.shape[0])

    def gather(self, rows):
        """rows [..., N] (N = this rank's source members; contiguous, fp64 or fp32) -> a NEW tensor [..., n_members] with
        out[..., k] = rows[..., src[k]]; the leading axes are flattened into the row count of one fiveeq_gather_rows_* launch.
        Rows on the GPU need device weights behind this plan and go through the HIP kernel; host rows (NumPy arrays or CPU
        tensors) are gathered by its NumPy twin."""
        import torch

        from . import _resample_host
        if tuple(rows.shape[-1:]) != (self.n_source,):
            raise ValueError(f"gather: rows of shape {tuple(rows.shape)}, want [..., {self.n_source}]")
        on_gpu = isinstance(rows, torch.Tensor) and rows.is_cuda
        if not on_gpu:
            src = self.src.cpu().numpy() if isinstance(self.src, torch.Tensor) else self.src
            if isinstance(rows, torch.Tensor):
                return torch.from_numpy(_resample_host.gather_rows(rows.detach().numpy(), src))
            return _resample_host.gather_rows(rows, src)
        if not isinstance(self.src, torch.Tensor) or self.src.device != rows.device:
            raise ValueError(f"gather: rows on {rows.device}, but the plan's indices are not (resample device weights there)")
        if rows.dtype not in (torch.float64, torch.float32) or not rows.is_contiguous():
            raise ValueError("gather: want contiguous fp64 or fp32 rows")
        from . import _capi
        from ._rowargs import call, ptr
        lib = _capi.load()
        M, N = self.n_members, self.n_source
        out = torch.empty(tuple(rows.shape[:-1]) + (M,), dtype=rows.dtype, device=rows.device)
        n_rows = rows.numel() // N
        if M and n_rows:
            call(lib, _capi, "fiveeq_gather_rows", rows.dtype, rows.device, n_rows, M, N, ptr(rows), M, ptr(out), ptr(self.src))
        return out

    def gather_params(self, params):
        """A copy of the parameter dict in which the per-member entries r0, rC, rT, q, f_scale and fx_scale — those of shape
        [K, N] — are gathered to [K, n_members]; everything else is shared by reference."""
        out = dict(params)
        for key in _PER_MEMBER_KEYS:
            v = params.get(key)
            if v is not None and getattr(v, "ndim", 0) == 2 and v.shape[-1] == self.n_source:
                out[key] = self.gather(v if getattr(v, "is_contiguous", lambda: True)() else v.contiguous())
        return out


def resample(weights, n_out=None, seed=None, group=None):
    """Systematic resampling in integer arithmetic (include/fiveeq.h, "RESAMPLING"): this shard's members with their integer
    weights -> a Resample naming, for each of this rank's outputs, the member it copies.  The M = n_out outputs over all ranks
    carry equal weight; member m is drawn floor or ceil of M w_m / W times, a member of weight 0 never; the ranks' outputs in
    rank order are the same list for every world size and shard split.
    weights: int64 [N] (importance_weights; 0..2^32 each, n_out required), or a boolean mask (0 / 1 weights).  A mask WITHOUT
    n_out is compacted: M = the number accepted over all ranks and the offset is 0 WHATEVER `seed` says, so the outputs are
    exactly the accepted members, each once, in order; a mask with n_out is resampled like any other weights.  A CUDA tensor takes the HIP kernels (scan, pick) and gives device indices; a NumPy array their NumPy twins.
    seed: None puts the first position at 0; else the offset is resample_offset(seed, M, W).
    Collective over `group` when torch.distributed runs: ONE all-gather of (local weight sum, member count, range flag).
    ValueError on EVERY rank — also when only one rank's argument is at fault, since the local findings travel in the flag —
    for an array of another type or shape, weights outside [0, 2^32], 2^31 or more members, a total weight of 0, and n_out
    missing or outside 1..2^31-1.  Outputs are not rebalanced: a rank owns the outputs its members' cumulative weight covers, so n_members
    differs per rank and can be 0 (shards of one Latin hypercube carry near-equal posterior mass)."""
    import torch

    from . import _resample_host
    from .distributed import _all_gather_np, _dist
    on_torch = isinstance(weights, torch.Tensor)
    w = weights if on_torch else np.asarray(weights)
    is_mask = w.dtype == (torch.bool if on_torch else np.dtype(bool))
    # what only THIS rank may see wrong travels in the gathered flag word, so that every rank raises and none is left waiting
    # in the collective: bit 2 the array's type or shape, bit 3 the shard's size, bit 4 n_out
    flag = 0
    if w.ndim != 1 or not (is_mask or w.dtype == (torch.int64 if on_torch else np.dtype(np.int64))):
        flag |= 4
    n = int(w.shape[0]) if w.ndim >= 1 else 0
    if n >= MAX_WEIGHTED_MEMBERS:
        flag |= 8
    if (n_out is None and not is_mask) or (n_out is not None and not 1 <= int(n_out) <= MAX_RESAMPLED):
        flag |= 16
    on_gpu = on_torch and w.is_cuda
    cum = None
    local_sum = 0
    if flag:
        pass                                                   # nothing is scanned: the refusal follows the exchange
    elif on_gpu and n:
        from . import _capi
        from ._rowargs import call, ptr
        lib = _capi.load()
        w = w.to(torch.int64).contiguous()
        cum = torch.empty(n + 1, dtype=torch.int64, device=w.device)       # the scan, and behind it the flag word
        work = torch.empty(int(lib.fiveeq_wscan_chunks(n)), dtype=torch.int64, device=w.device)
        call(lib, _capi, "fiveeq_wscan", None, w.device, n, ptr(w), ptr(work), ptr(cum), ptr(cum[n:]))
        local_sum, flag = (int(v) for v in cum[n - 1:].cpu())                # bit 1: a weight outside [0, 2^32]
        cum = cum[:n]
    elif n:
        host_w = w.detach().numpy() if on_torch else w
        cum, flag = _resample_host.wscan(host_w.astype(np.int64))
        local_sum = int(cum[-1].astype(np.int64))

    dist, rank, world, exchange = _dist(group)
    mine = np.array([local_sum, n, flag], dtype=np.int64)
    if exchange:
        dev = w.device if on_gpu else torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) != "gloo" else None
        got = _all_gather_np(dist, group, world, mine, dev)
    else:
        got = mine[None]
    flags = int(np.bitwise_or.reduce(got[:, 2]))
    if flags & 4:
        raise ValueError("resample: weights must be an int64 [N] array of integer weights or a boolean [N] mask")
    if flags & 16:
        raise ValueError(f"resample: n_out={n_out} must be given for integer weights (a mask defaults to the number accepted) "
                         "and lie in 1..2^31-1")
    if flags & 2:
        raise ValueError("resample: weights outside [0, 2^32]")
    if flags & 8 or int(got[:, 1].sum()) >= MAX_WEIGHTED_MEMBERS:
        raise ValueError(f"resample: {int(got[:, 1].sum())} members over all ranks; integer weights need fewer than 2^31")
    sums = [int(v) for v in got[:, 0]]
    W = sum(sums)
    if W == 0:
        raise ValueError("resample: the weights of all members on all ranks sum to 0")
    M = W if n_out is None else int(n_out)
    if not 1 <= M <= MAX_RESAMPLED:
        raise ValueError(f"resample: n_out={M} outside 1..2^31-1")
    rho = 0 if is_mask and n_out is None else resample_offset(seed, M, W)
    plan = resample_plan(sums, rank if exchange else 0, M, rho)
    j0, mine_out = plan["j0"], plan["j1"] - plan["j0"]
    args = (plan["C_lo"], M, plan["q"], plan["a"], plan["s"], plan["b"], j0, mine_out)
    if on_gpu:
        src = torch.empty(mine_out, dtype=torch.int32, device=w.device)
        if mine_out:
            call(lib, _capi, "fiveeq_resample_pick", None, w.device, n, ptr(cum), *args, ptr(src))
    else:
        src = _resample_host.pick(cum, *args) if mine_out else np.zeros(0, dtype=np.int32)
        if on_torch:
            src = torch.from_numpy(src)
    return Resample(M, j0, W, rho, src, n)
