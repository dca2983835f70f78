"""Reference for the WEIGHTED summary (include/fiveeq.h, "WEIGHTED SUMMARY") that shares no code with the passes: a stable
argsort of the values, a cumulative sum of the weights as Python ints, the first index whose cumulative weight reaches k_p;
moments with math.fsum.  Slow and obvious on purpose."""
import math
from fractions import Fraction

import numpy as np

W_ONE = 1 << 32


def rank_of(p, W):
    """k_p = max(1, ceil(Fraction(p) / 100 * W)) in rational arithmetic."""
    return max(1, math.ceil(Fraction(p) / 100 * W))


def weighted_row(x, w, percentiles):
    """x [n] floats (any float dtype; widened exactly), w [n] integers -> dict(percentiles [P] fp64, mean, std, ess, min, max,
    count, weight_sum, sum_abs_wx, sum_abs_wx2, sum_w2) — the last three are what the error bounds of the moments are made of."""
    x = np.asarray(x).astype(np.float64)
    w = [int(v) for v in np.asarray(w)]
    keep = [i for i, v in enumerate(w) if v > 0]
    W = sum(w)
    if W == 0:
        raise ValueError("no weight")
    xs, ws = [float(x[i]) for i in keep], [w[i] for i in keep]
    out = {"count": len(keep), "weight_sum": W, "sum_w2": sum(v * v for v in ws)}
    out["ess"] = float(Fraction(W * W, out["sum_w2"]))
    live = [v for v in xs if not math.isnan(v)]
    out["min"], out["max"] = (min(live), max(live)) if live else (math.inf, -math.inf)
    if len(live) != len(xs):                                   # a NaN value with positive weight
        out.update(percentiles=np.full(len(percentiles), np.nan), mean=math.nan, std=math.nan, sum_abs_wx=math.nan,
                   sum_abs_wx2=math.nan)
        return out
    order = np.argsort(np.array(xs), kind="stable")
    pct = []
    for p in percentiles:
        k, cum, got = rank_of(p, W), 0, None
        for i in order:
            cum += ws[i]
            if cum >= k:
                got = xs[i]
                break
        pct.append(got)
    out["percentiles"] = np.array(pct, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        s1 = math.fsum(wi * xi for wi, xi in zip(ws, xs)) if all(math.isfinite(v) for v in xs) else math.nan
        s2 = math.fsum(wi * xi * xi for wi, xi in zip(ws, xs)) if all(math.isfinite(v) for v in xs) else math.nan
    out["sum_abs_wx"] = math.fsum(abs(wi * xi) for wi, xi in zip(ws, xs))
    out["sum_abs_wx2"] = math.fsum(wi * xi * xi for wi, xi in zip(ws, xs))
    out["mean"] = s1 / W
    out["std"] = math.sqrt(max(s2 / W - out["mean"] ** 2, 0.0))
    return out


def weighted_rows(rows, w, percentiles):
    """rows [K, n] -> list of weighted_row results."""
    return [weighted_row(r, w, percentiles) for r in np.asarray(rows)]
