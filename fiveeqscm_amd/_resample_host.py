"""NumPy twins of the three RESAMPLING kernels of the C ABI (include/fiveeq.h, "RESAMPLING": fiveeq_wscan,
fiveeq_resample_pick, fiveeq_gather_rows_*): the same outputs bit for bit — every one is an integer or a copied value.

This is the path of HOST weights (constrain.resample of a NumPy array), in the role _wsummary_host.py plays for the weighted
summary: the rank arithmetic and the exchanges of constrain.resample run on it where there is no GPU.  Device weights go
through the HIP kernels, never through here.
"""
import numpy as np

W_ONE = 1 << 32


def wscan(weights):
    """weights [n] (any integer dtype, taken as uint64 bit patterns) -> (cum [n] uint64: the inclusive scan modulo 2^64,
    flags: 2 when a weight is above 2^32 — a negative int64 is, as a bit pattern — else 0)."""
    w = np.ascontiguousarray(weights).astype(np.int64, copy=False).view(np.uint64)
    cum = np.cumsum(w, dtype=np.uint64)
    return cum, (2 if w.size and bool((w > np.uint64(W_ONE)).any()) else 0)


def pick(cum, c_lo, M, q, a, s, b, j0, n_out):
    """src [n_out] int32: the first local member m with cum[m] > p_j - c_lo for j = j0 .. j0 + n_out - 1,
    p_j = j q + a + (j s + b) div M in 64-bit integers; clamped to [0, n - 1] like the kernel."""
    if n_out == 0:
        return np.zeros(0, dtype=np.int32)
    j = np.arange(j0, j0 + n_out, dtype=np.uint64)
    u = np.uint64
    p = j * u(q) + u(a) + (j * u(s) + u(b)) // u(M)
    t = np.where(p > u(c_lo), p - u(c_lo), u(0))
    at = np.searchsorted(np.asarray(cum, dtype=np.uint64), t, side="right")
    return np.minimum(at, len(cum) - 1).astype(np.int32)


def gather_rows(rows, src):
    """rows [..., n] -> a new array [..., len(src)]: rows[..., src]."""
    rows = np.asarray(rows)
    return np.ascontiguousarray(rows[..., np.asarray(src, dtype=np.int64)])
