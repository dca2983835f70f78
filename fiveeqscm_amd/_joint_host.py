"""NumPy restatement of the two JOINT STATISTICS passes of the C ABI (include/fiveeq.h, "JOINT STATISTICS":
fiveeq_joint_moments_*, fiveeq_cond_sums_*) behind the same pointer-and-size signatures.  The integer outputs are the
kernel's bit for bit; the fp64 sums are taken in plain member order (the kernel's order is its own: both lie within the
rounding bound of any order).

NOT a fallback: the product takes device rows through the HIP passes and refuses host rows.  `host_passes()` puts this object
behind joint.py's switch (_lib_and_stream / _passes_apply) and the weighted-summary twin (_wsummary_host.py) behind
distributed.py's, so that the HOST side of joint.joint_moments / sensitivity — the merges in rank order, the edges, the
exchanges over gloo — runs on CPU tensors where there is no GPU (tests/test_joint_cpu.py).
"""
import contextlib

import numpy as np

from ._wsummary_host import _view

CHUNK = 4096


def _rows(ptr, dtype, k, n, ld):
    """[k][n] view of rows ld elements apart."""
    flat = _view(ptr, dtype, (k - 1) * ld + n)
    return np.lib.stride_tricks.as_strided(flat, (k, n), (ld * flat.itemsize, flat.itemsize))


class JointPasses:
    """The two passes with the C ABI's signatures; `stream` is ignored.  Every function returns 0."""

    def fiveeq_joint_chunks(self, n):
        return 0 if n < 1 else (n + CHUNK - 1) // CHUNK

    def fiveeq_joint_moments_words(self, n_x, n_y):
        return n_x * n_y + 3 * (n_x + n_y) + 3

    def fiveeq_cond_sums_words(self, n_x, n_y, n_bins):
        return n_x * n_bins * (n_y + 1) + n_x

    def _moments(self, dtype, n, n_x, ld_x, x, n_y, ld_y, y, weights, pivots, partial, co, margins, info, nanrows, stream):
        w = _view(weights, np.uint64, n)
        pos = w > 0
        wp = w[pos]
        wd = wp.astype(np.float64)
        c = _view(pivots, np.float64, n_x + n_y)
        v = np.concatenate([_rows(x, dtype, n_x, n, ld_x)[:, pos], _rows(y, dtype, n_y, n, ld_y)[:, pos]]).astype(np.float64)
        out_co = _view(co, np.float64, n_x * n_y).reshape(n_x, n_y)
        out_m = _view(margins, np.float64, 2 * (n_x + n_y)).reshape(n_x + n_y, 2)
        with np.errstate(invalid="ignore", over="ignore"):
            d = v - c[:, None]
            p = wd[None, :] * d
            for i in range(n_x):
                for j in range(n_y):
                    out_co[i, j] = (d[i] * p[n_x + j]).sum()
            out_m[:, 0], out_m[:, 1] = p.sum(axis=1), (p * d).sum(axis=1)
        isnan = np.isnan(v)
        _view(nanrows, np.uint64, n_x + n_y)[:] = [int(wp[isnan[r]].sum(dtype=np.uint64)) for r in range(n_x + n_y)]
        flags = (1 if isnan.any() else 0) | (2 if (w > np.uint64(1 << 32)).any() else 0)
        _view(info, np.uint64, 4)[:] = (int(w.sum(dtype=np.uint64)), int(pos.sum()), flags, 0)
        return 0

    def _cond(self, dtype, n, n_x, ld_x, x, n_y, ld_y, y, weights, n_bins, edges, pivots, partial, sums, binw, xnan, stream):
        w = _view(weights, np.uint64, n)
        pos = w > 0
        wp = w[pos]
        wd = wp.astype(np.float64)
        c = _view(pivots, np.float64, n_y)
        ed = _view(edges, np.float64, n_x * (n_bins - 1)).reshape(n_x, n_bins - 1) if n_bins > 1 else np.zeros((n_x, 0))
        xs = _rows(x, dtype, n_x, n, ld_x)[:, pos].astype(np.float64)
        out_s = _view(sums, np.float64, n_x * n_bins * n_y).reshape(n_x, n_bins, n_y)
        out_w = _view(binw, np.uint64, n_x * n_bins).reshape(n_x, n_bins)
        out_n = _view(xnan, np.uint64, n_x)
        with np.errstate(invalid="ignore", over="ignore"):
            t = wd[None, :] * (_rows(y, dtype, n_y, n, ld_y)[:, pos].astype(np.float64) - c[:, None])
            for i in range(n_x):
                isnan = np.isnan(xs[i])
                b = (ed[i][:, None] < xs[i][None, :]).sum(axis=0)           # THE BIN: the number of edges below the value
                out_n[i] = int(wp[isnan].sum(dtype=np.uint64))
                for k in range(n_bins):
                    sel = (b == k) & ~isnan
                    out_w[i, k] = int(wp[sel].sum(dtype=np.uint64))
                    out_s[i, k] = t[:, sel].sum(axis=1)
        return 0

    def fiveeq_last_error(self):
        return b""


for _name, _dt in (("f64", np.float64), ("f32", np.float32)):
    for _fn, _impl in (("fiveeq_joint_moments", "_moments"), ("fiveeq_cond_sums", "_cond")):
        setattr(JointPasses, f"{_fn}_{_name}", (lambda impl, dt: lambda self, *a: getattr(self, impl)(dt, *a))(_impl, _dt))


class _Check:
    @staticmethod
    def check(lib, rc):
        if rc != 0:
            raise RuntimeError(f"host pass returned {rc}")


def install():
    """Put the NumPy passes behind joint.py's switch, and the weighted summary's behind distributed.py's, for the rest of the
    process (spawned test workers); returns what host_passes() needs to undo it."""
    import torch

    from . import _wsummary_host, joint
    saved = joint._lib_and_stream, joint._passes_apply, _wsummary_host.install()
    passes = JointPasses()
    joint._lib_and_stream = lambda rows: (passes, _Check, None)
    joint._passes_apply = lambda rows: rows.dtype in (torch.float32, torch.float64)
    return saved


@contextlib.contextmanager
def host_passes():
    """`with host_passes():` — joint.joint_moments / sensitivity take HOST rows through the NumPy passes inside the block."""
    from . import distributed, joint
    saved = install()
    try:
        yield
    finally:
        joint._lib_and_stream, joint._passes_apply = saved[0], saved[1]
        distributed._lib_and_stream, distributed._passes_apply = saved[2]
