"""Joint statistics of per-member device rows: how outputs co-vary with parameters, and which parameter explains what share
of an output's spread.

    jm = joint_moments(eng.parameter_rows()[1], eng.T[-1:], weights=w)        # cov, corr, slope [Kx, Ky]
    s = sensitivity(x, y, bins=16, accepted=mask)                             # eta2 [Kx, Ky]: first-order sensitivity index
    s = eng.drivers(eng.trajectory_metrics().peak[None])                      # the engine's parameters against any y rows

Two HIP passes (include/fiveeq.h, "JOINT STATISTICS"; csrc/fiveeq_joint.hpp): co-moments about the global weighted means, and
sums of y conditional on the bin of x between exact weighted percentiles of x.  Weights are the integers of the weighted
summary (constrain.importance_weights), a boolean `accepted` mask means weights 0 / 1, neither means weight 1.  Both functions
are collective over `group`: the small records are all-gathered and merged in rank order, the integer results are exact for
every world size.  Device rows only: there is no CPU path (_joint_host.py is the NumPy twin the CPU tests put behind the same
switch).
"""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _rowargs


def _lib_and_stream(rows):
    """(library, _capi, stream) for rows on a GPU.  (_joint_host.host_passes() replaces this function and the next.)"""
    from . import _capi
    return _capi.load(), _capi, ctypes.c_void_p(torch.cuda.current_stream(rows.device).cuda_stream)


def _passes_apply(rows):
    return rows.is_cuda and rows.dtype in (torch.float32, torch.float64)


@dataclass
class JointMoments:
    """Host fp64 tensors.  cov, corr, slope are [Kx, Ky]; slope = cov / var_x is the regression slope of y on x.  A pair with
    a NaN member of positive weight is NaN; corr and slope are NaN where a variance is 0."""
    mean_x: torch.Tensor
    mean_y: torch.Tensor
    var_x: torch.Tensor
    var_y: torch.Tensor
    cov: torch.Tensor
    corr: torch.Tensor
    slope: torch.Tensor
    weight_sum: int
    count: int
    ess: float


@dataclass
class Sensitivity:
    """eta2 [Kx, Ky]: the share of the variance of y row j that the binned conditional mean over x row i explains (the
    correlation ratio: an estimate of the first-order variance-based sensitivity index); an unrelated pair has the expected
    value noise_floor = (B - 1) / (ess - 1).  cond_mean [Kx, B, Ky] (NaN for an empty bin), bin_weight [Kx, B] int64, edges
    [Kx, B - 1]: the exact weighted percentiles 100 b / B of the x rows."""
    eta2: torch.Tensor
    cond_mean: torch.Tensor
    bin_weight: torch.Tensor
    edges: torch.Tensor
    noise_floor: float
    moments: JointMoments


def _rows_of(t, name):
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError(f"{name}: want a tensor [K, N]")
    if not _passes_apply(t):
        raise TypeError(f"{name} must be fp32 / fp64 rows on a GPU (got {t.dtype} on {t.device}): the joint statistics run through "
                        "the HIP passes and have no CPU fallback")
    return t


def _in_place(t):
    t, (ld,) = _rowargs.walk_in_place(t, t.shape[1])
    return t, (ld if t.shape[0] > 1 else max(ld, 1))           # one row of no members still reports 1


def _weights_of(N, dev, weights, accepted):
    if weights is not None and accepted is not None:
        raise ValueError("weights= and accepted= exclude each other (a weight of 0 drops a member)")
    if accepted is not None:
        return _rowargs.bool_mask(accepted, N, dev).to(torch.int64)
    if weights is None:
        return torch.ones(N, dtype=torch.int64, device=dev)
    return _rowargs.int_weights(weights, N, dev, check_range=True).contiguous()


def _prepare(x, y, weights, accepted):
    from . import _capi
    x, y = _rows_of(x, "x"), _rows_of(y, "y")
    if x.device != y.device or x.shape[1] != y.shape[1]:
        raise ValueError(f"x {tuple(x.shape)} on {x.device} and y {tuple(y.shape)} on {y.device}: want rows of the same members")
    for name, t in (("x", x), ("y", y)):
        if not 1 <= t.shape[0] <= _capi.MAX_JOINT_ROWS:
            raise ValueError(f"{name}: {t.shape[0]} rows, want 1..{_capi.MAX_JOINT_ROWS}")
    if x.dtype != y.dtype:                                   # a mix is widened (exactly) on the device
        x, y = x.to(torch.float64), y.to(torch.float64)
    return x, y, _weights_of(x.shape[1], x.device, weights, accepted)


def _gather(dist, group, world, exchange, arr, dev):
    """[world, ...] of every rank's int64 record, rank order."""
    from .distributed import _all_gather_np
    return _all_gather_np(dist, group, world, arr, dev) if exchange else arr[None]


class _Core:
    """What both functions share: the rows as the passes take them, the merged weighted moments, pass (a) merged over the
    ranks."""

    def __init__(self, x, y, weights, accepted, group):
        from . import distributed as D
        self.x, self.y, self.w = _prepare(x, y, weights, accepted)
        (self.x, self.ldx), (self.y, self.ldy) = _in_place(self.x), _in_place(self.y)
        self.group = group
        self.dist, self.rank, self.world, self.exchange = D._dist(group)
        self.Kx, self.Ky, self.N = self.x.shape[0], self.y.shape[0], self.x.shape[1]
        self.dev = self.x.device
        self.lib, self.capi, self.st = _lib_and_stream(self.x)
        self.sfx = "f64" if self.x.dtype == torch.float64 else "f32"
        Kx, Ky, R = self.Kx, self.Ky, self.Kx + self.Ky
        # ---- the weighted moments of every row (the pass of the weighted summary), merged in rank order: the pivots ---------
        wlib, wcapi, wct, wst = D._lib_and_stream(self.x)
        rec = torch.zeros((R, D.WMOM_WORDS), dtype=torch.int64, device=self.dev)
        D._weighted_moments_dev(wlib, wcapi, wct, wst, self.x, self.w, rec[:Kx])
        D._weighted_moments_dev(wlib, wcapi, wct, wst, self.y, self.w, rec[Kx:])
        parts = _gather(self.dist, group, self.world, self.exchange, rec.cpu().numpy(), self.dev)        # [world, R, 8]
        if (np.bitwise_or.reduce(parts[:, :, 6].reshape(-1)) & 2) != 0:
            raise ValueError("weights: values outside [0, 2^32]")
        self.W = sum(int(v) for v in parts[:, 0, 7])
        if self.W == 0:
            raise ValueError("joint statistics: the weights of all members on all ranks sum to 0")
        self.count = int(parts[:, 0, 5].sum())
        fp = parts[:, :, :5].view(np.float64)
        s1, sw2 = np.zeros(R), 0.0
        with np.errstate(invalid="ignore", over="ignore"):
            for r in range(parts.shape[0]):
                s1, sw2 = s1 + fp[r, :, 0], sw2 + float(fp[r, 0, 2])
            self.pivots = s1 / float(self.W)
            self.flat = ~(fp[:, :, 4].max(axis=0) > fp[:, :, 3].min(axis=0))       # one value carries all the weight: variance 0
        self.ess = float(self.W) * float(self.W) / sw2
        # ---- pass (a): co-moments about the pivots — the same bits on every rank — merged in rank order ------------------------
        n_out = Kx * Ky + 2 * R + 4 + R
        if self.N > 0:
            out = torch.empty(n_out, dtype=torch.int64, device=self.dev)
            piv = torch.from_numpy(self.pivots).to(self.dev)
            chunks = int(self.lib.fiveeq_joint_chunks(self.N))
            work = torch.empty(chunks * int(self.lib.fiveeq_joint_moments_words(Kx, Ky)), dtype=torch.float64, device=self.dev)
            o = [0, Kx * Ky, Kx * Ky + 2 * R, Kx * Ky + 2 * R + 4]
            with D._on(self.dev):
                self.capi.check(self.lib, getattr(self.lib, f"fiveeq_joint_moments_{self.sfx}")(
                    self.N, Kx, self.ldx, self._p(self.x), Ky, self.ldy, self._p(self.y), self._p(self.w), self._p(piv), self._p(work),
                    self._p(out, o[0]), self._p(out, o[1]), self._p(out, o[2]), self._p(out, o[3]), self.st))
            mine = out.cpu().numpy()
        else:
            mine = np.zeros(n_out, dtype=np.int64)
        got = _gather(self.dist, group, self.world, self.exchange, mine, self.dev)
        f = got.view(np.float64)
        co, mar = np.zeros(Kx * Ky), np.zeros(2 * R)
        with np.errstate(invalid="ignore", over="ignore"):
            for r in range(got.shape[0]):
                co, mar = co + f[r, :Kx * Ky], mar + f[r, Kx * Ky:Kx * Ky + 2 * R]
        self.co, self.margins = co.reshape(Kx, Ky), mar.reshape(R, 2)
        self.nanrows = got[:, Kx * Ky + 2 * R + 4:].sum(axis=0)
        if int(got[:, Kx * Ky + 2 * R].sum()) != self.W:
            raise RuntimeError(f"joint statistics: the co-moment pass weighs {int(got[:, Kx * Ky + 2 * R].sum())} where the weights sum to {self.W}")

    @staticmethod
    def _p(t, word=0):
        return ctypes.c_void_p(t.data_ptr() + 8 * word)

    def moments(self):
        Kx, W = self.Kx, float(self.W)
        nan = self.nanrows != 0
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            s, ss = self.margins[:, 0], self.margins[:, 1]
            mean = self.pivots + s / W
            var = np.where(self.flat, 0.0, np.maximum((ss - s * s / W) / W, 0.0))
            var = np.where(nan, np.nan, var)
            cov = (self.co - s[:Kx, None] * s[None, Kx:] / W) / W
            cov = np.where(self.flat[:Kx, None] | self.flat[None, Kx:], 0.0, cov)
            cov = np.where(nan[:Kx, None] | nan[None, Kx:], np.nan, cov)
            vx, vy = var[:Kx, None], var[None, Kx:]
            corr = np.where((vx > 0) & (vy > 0), cov / np.sqrt(vx * vy), np.nan)
            slope = np.where(vx > 0, cov / vx, np.nan) + 0.0 * cov
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))      # noqa: E731
        return JointMoments(mean_x=t(np.where(nan[:Kx], np.nan, mean[:Kx])), mean_y=t(np.where(nan[Kx:], np.nan, mean[Kx:])),
                            var_x=t(var[:Kx]), var_y=t(var[Kx:]), cov=t(cov), corr=t(corr), slope=t(slope), weight_sum=self.W,
                            count=self.count, ess=self.ess)


def joint_moments(x, y, weights=None, accepted=None, group=None):
    """x [Kx, n_local], y [Ky, n_local]: fp32 / fp64 rows ON THE GPU of this rank's members (1..32 rows each; a mix of dtypes
    is widened to fp64 on the device).  weights: int64 [n_local], 0..2^32 each; accepted: a boolean mask (weights 0 / 1);
    neither: weight 1; both: ValueError.  Collective over `group`.  Returns JointMoments (host tensors) on every rank.
    Flow: weighted moments of every row -> all-gather, merge in rank order: the global means are the pivots -> co-moments
    about the pivots -> all-gather, merge in rank order -> cov = (co - sx sy / W) / W on the host.  The weights of all ranks
    summing to 0 is a ValueError on every rank."""
    return _Core(x, y, weights, accepted, group).moments()


def _edges(core, B):
    """[Kx, B - 1] fp64: the exact weighted percentiles 100 b / B of the x rows, the same bits on every rank."""
    from .distributed import gather_weighted_summary
    Kx = core.Kx
    if B == 1:
        return np.zeros((Kx, 0))
    pct = [100.0 * b / B for b in range(1, B)]
    out = gather_weighted_summary(core.x, core.w, pct, dst=0, group=core.group)["percentiles"]
    if not core.exchange:
        return out.numpy().copy()
    dist = core.dist
    bits = out.contiguous().view(torch.int64) if core.rank == 0 else torch.empty((Kx, B - 1), dtype=torch.int64)
    if dist.get_backend(core.group) != "gloo":
        bits = bits.to(core.dev)
    dist.broadcast(bits, src=dist.get_global_rank(core.group, 0) if core.group is not None else 0, group=core.group)      # 8-byte patterns
    return bits.cpu().numpy().view(np.float64).copy()


def sensitivity(x, y, bins=16, weights=None, accepted=None, group=None):
    """The rows, weights and collectives of joint_moments.  Per x row the members are binned between the exact weighted
    percentiles 100 b / `bins` of that row (a value equal to an edge belongs to the lower bin; 1 <= bins <= 32); eta2[i, j] =
    sum over the non-empty bins of W_b (m_bj - m_j)^2 / (syy_j - sy_j^2 / W), with m_bj the weighted mean of y row j in bin b of
    x row i.  NaN where y row j has no variance or x row i or y row j has a NaN of positive weight; 0 where all the weight sits
    in one bin.  Returns Sensitivity (host tensors) on every rank."""
    from . import _capi
    from . import distributed as D
    B = int(bins)
    if not 1 <= B <= _capi.MAX_COND_BINS:
        raise ValueError(f"bins: {bins} given, want 1..{_capi.MAX_COND_BINS}")
    core = _Core(x, y, weights, accepted, group)
    jm = core.moments()
    Kx, Ky, W = core.Kx, core.Ky, float(core.W)
    edges = _edges(core, B)
    n_out = Kx * B * Ky + Kx * B + Kx
    if core.N > 0:
        out = torch.empty(n_out, dtype=torch.int64, device=core.dev)
        ed = torch.from_numpy(np.ascontiguousarray(edges.reshape(-1))).to(core.dev)
        piv = torch.from_numpy(np.ascontiguousarray(core.pivots[Kx:])).to(core.dev)
        chunks = int(core.lib.fiveeq_joint_chunks(core.N))
        work = torch.empty(chunks * int(core.lib.fiveeq_cond_sums_words(Kx, Ky, B)), dtype=torch.float64, device=core.dev)
        p = core._p
        with D._on(core.dev):
            core.capi.check(core.lib, getattr(core.lib, f"fiveeq_cond_sums_{core.sfx}")(
                core.N, Kx, core.ldx, p(core.x), Ky, core.ldy, p(core.y), p(core.w), B, p(ed) if B > 1 else None, p(piv), p(work),
                p(out), p(out, Kx * B * Ky), p(out, Kx * B * Ky + Kx * B), core.st))
        mine = out.cpu().numpy()
    else:
        mine = np.zeros(n_out, dtype=np.int64)
    got = _gather(core.dist, group, core.world, core.exchange, mine, core.dev)
    f = got.view(np.float64)
    sums = np.zeros(Kx * B * Ky)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(got.shape[0]):
            sums = sums + f[r, :Kx * B * Ky]
    sums = sums.reshape(Kx, B, Ky)
    binw = got[:, Kx * B * Ky:Kx * B * Ky + Kx * B].sum(axis=0).reshape(Kx, B)
    xnan = got[:, Kx * B * Ky + Kx * B:].sum(axis=0)
    if not np.array_equal(binw.sum(axis=1) + xnan, np.full(Kx, core.W, dtype=np.int64)):
        raise RuntimeError(f"sensitivity: the bins weigh {(binw.sum(axis=1) + xnan).tolist()} where the weights sum to {core.W}")
    nan_y = core.nanrows[Kx:] != 0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        Wb = binw.astype(np.float64)
        live = binw > 0
        dev_b = np.where(live[:, :, None], sums / np.where(live, Wb, 1.0)[:, :, None], 0.0)       # m_bj - cy_j
        sy, syy = core.margins[Kx:, 0], core.margins[Kx:, 1]
        d = dev_b - (sy / W)[None, None, :]                                                        # m_bj - m_j
        num = (Wb[:, :, None] * d * d * live[:, :, None]).sum(axis=1)
        den = np.where(core.flat[Kx:], 0.0, syy - sy * sy / W)
        eta2 = np.where(den[None, :] > 0, num / den[None, :], np.nan)
        eta2 = np.where((live.sum(axis=1) <= 1)[:, None] & ~np.isnan(eta2), 0.0, eta2)             # all weight in one bin
        eta2 = np.where((xnan != 0)[:, None] | nan_y[None, :], np.nan, eta2)
        cond = np.where(live[:, :, None], core.pivots[None, None, Kx:] + dev_b, np.nan)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
    return Sensitivity(eta2=t(eta2), cond_mean=t(cond), bin_weight=t(binw.astype(np.int64)), edges=t(edges),
                       noise_floor=(B - 1) / (core.ess - 1.0) if core.ess > 1.0 else float("nan"), moments=jm)
