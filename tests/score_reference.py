"""The plain-NumPy reference of the SCORING STORED ROWS pass (include/fiveeq.h), built on constrain.misfit_numpy — the function
the in-loop misfit is held to: one quantity at a time, the LIVE rows only (a dead row-quantity is dropped before misfit_numpy
sees it, so nothing planted there can reach the result)."""
import numpy as np

from fiveeqscm_amd.constrain import Observations, misfit_numpy


def reference(rows, steps, tables, acc=None):
    """rows [K, Q, N] (or [K, N] with one table) host array, steps [K], tables: Q tables [n_steps, 4] -> [Q, 3, N] ([3, N]) fp64."""
    rows = np.asarray(rows)
    single = rows.ndim == 2
    x = rows[:, None] if single else rows
    tabs = [np.asarray(tables, dtype=np.float64)] if single else [np.asarray(t, dtype=np.float64) for t in tables]
    K, Q, N = x.shape
    assert len(tabs) == Q
    steps = np.asarray(steps, dtype=np.int64)
    out = np.zeros((Q, 3, N)) if acc is None else np.array(acc, dtype=np.float64).reshape(Q, 3, N)
    for j, tab in enumerate(tabs):
        rec = tab[steps] if K else tab[:0]                      # the record of every row
        live = (rec[:, 1] != 0) | (rec[:, 2] != 0)
        if live.any():
            out[j] = misfit_numpy(x[live, j], rec[live], acc=out[j])
    return out[0] if single else out


def make_table(n_steps, seed, live_every=1, baseline=None, anomaly=True, lo=0):
    """A table with an observation on every `live_every`-th step from `lo` and (anomaly) the baseline block [a, b)."""
    rng = np.random.default_rng(seed)
    t = np.zeros((n_steps, 4))
    idx = np.arange(lo, n_steps, live_every)
    t[idx, 0] = rng.normal(1.0, 0.5, idx.size)
    t[idx, 1] = 1.0 / rng.uniform(0.05, 0.3, idx.size) ** 2
    if anomaly:
        a, b = baseline if baseline is not None else (0, max(1, n_steps // 4))
        t[a:b, 2] = 1.0 / (b - a)
    return Observations(t, anomaly=anomaly)


def make_rows(K, Q, N, dtype, seed):
    """[K, Q, N] values around 1 with a trend, exactly representable in `dtype`."""
    rng = np.random.default_rng(seed)
    x = rng.normal(1.0, 0.7, (K, Q, N)) + np.linspace(0.0, 1.0, K)[:, None, None]
    return x.astype(dtype)
