"""Constraining an ensemble against an observed temperature record (round 7).

Each member is scored against the record while it is stepped: the kernels carry three fp64 accumulators per member
(include/fiveeq.h, "CONSTRAINED RUNS"), so no historical T row has to be stored.  With T_t the member's T after step t:

    A = A + b_t T_t;   d = T_t - o_t;   pd = p_t d;   U = U + pd;   V = V + pd d        (steps with p_t = b_t = 0 skipped)

and the score of the baseline-corrected series is chi2 = V - 2 A U + A^2 P = sum_t p_t (T_t - mean_ref T - o_t)^2, P = sum_t p_t.
Members are then kept by a threshold on chi2 or by rejection sampling, and the summaries are computed over the kept members
(EnsembleEngine.gather_summary(..., accepted=mask)).

    obs = Observations.from_years(run_years, obs_years, T_obs, sigma, baseline=(1850, 1900))
    eng = EnsembleEngine(params, N, E, observations=obs, ...);  eng.run(mode="auto")
    keep = accept_rejection(eng.chi2(), seed, m0, n_total, group)

or every member is kept and weighted by its likelihood (include/fiveeq.h, "WEIGHTED SUMMARY"):

    w = importance_weights(eng.chi2(), group);  eng.gather_summary(steps, weights=w)
"""
import hashlib

import numpy as np

ACCEPT_SEED = 0x0B5E47ED            # the rejection rule's default key: its uniforms are a dimension of their own LHS
W_ONE = 1 << 32                     # the integer weight of the best member (importance_weights); the largest weight a member may carry
MAX_WEIGHTED_MEMBERS = 1 << 31      # fewer members than this over all ranks: every sum of weights then fits int64


class Observations:
    """The shared observation table obs [n_steps, 4] fp64: per step (o_t, p_t = 1/sigma_t^2 or 0, b_t = 1/n_ref inside the
    reference period or 0, 0).  Build it with `from_years`; `table`, `P` (= sum p_t) and `sha256` (of the table's bytes)."""

    def __init__(self, table):
        t = np.array(table, dtype=np.float64, order="C")
        if t.ndim != 2 or t.shape[1] != 4 or t.shape[0] < 1:
            raise ValueError(f"observation table: shape {t.shape}, want [n_steps, 4]")
        if not np.isfinite(t).all():
            raise ValueError("observation table: non-finite entries")
        if (t[:, 1] < 0).any() or (t[:, 2] < 0).any() or (t[:, 3] != 0).any():
            raise ValueError("observation table: weights must be >= 0 and column 3 zero")
        if not t[:, 2].any():
            raise ValueError("observation table: empty baseline period")
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

    @classmethod
    def from_years(cls, run_years, obs_years, T_obs, sigma, baseline):
        """Match observations to the run's steps by year.  run_years [n_steps]: the year of each step (T after step t is the
        state at run_years[t]); obs_years / T_obs / sigma [n_obs]; baseline = (y0, y1), inclusive: the reference period
        whose mean T is subtracted from each member's series before it is compared (b_t = 1/n_ref on its steps)."""
        ry = np.asarray(run_years, dtype=np.float64).reshape(-1)
        oy = np.asarray(obs_years, dtype=np.float64).reshape(-1)
        To = np.asarray(T_obs, dtype=np.float64).reshape(-1)
        sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), oy.shape).copy()
        if To.shape != oy.shape:
            raise ValueError(f"T_obs has {To.size} values for {oy.size} years")
        for name, v in (("run_years", ry), ("obs_years", oy), ("T_obs", To), ("sigma", sg), ("baseline", np.asarray(baseline,
                                                                                                              dtype=float))):
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
