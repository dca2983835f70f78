"""NumPy restatement of the TRAJECTORY METRICS pass of the C ABI (include/fiveeq.h, "TRAJECTORY METRICS":
fiveeq_traj_metrics_f64 / _f32) behind the same pointer-and-size signature, bit for bit: every result is an integer or an
fp64 sum taken in row order.

NOT a fallback: the product takes device rows through the HIP kernel and refuses host rows.  `host_passes()` puts this object
behind metrics.py's switch (_lib_and_stream / _passes_apply), in the role _wsummary_host.py plays for the weighted summary, so
that the HOST side of metrics.trajectory_metrics — shapes, strides, the step checks, state continuation, window counts — runs
on CPU tensors where there is no GPU (tests/test_traj_metrics_cpu.py).
"""
import contextlib
import ctypes

import numpy as np

_CT = {np.float64: ctypes.c_double, np.float32: ctypes.c_float, np.int32: ctypes.c_int32}


def _view(ptr, dtype, count):
    addr = ptr.value if isinstance(ptr, ctypes.c_void_p) else int(ptr)
    if count == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array((_CT[dtype] * count).from_address(addr))


def _block(ptr, dtype, lead, stride, rows, n, ld):
    """[lead][rows][n] view of a buffer whose blocks are `stride` elements apart and whose rows are ld apart."""
    if lead == 0 or rows == 0:
        return np.zeros((lead, rows, n), dtype=dtype)
    flat = _view(ptr, dtype, (lead - 1) * stride + (rows - 1) * ld + n)
    return np.lib.stride_tricks.as_strided(flat, (lead, rows, n), (stride * flat.itemsize, ld * flat.itemsize, flat.itemsize))


class MetricsPasses:
    """fiveeq_traj_metrics_* with the C ABI's signature; `stream` is ignored.  Returns 0."""

    def _metrics(self, dtype, n_scen, n_rows, n, ld, rows, scen_stride, steps, n_levels, levels, n_windows, windows, fmet, imet,
                 first_call, stream):
        lv = _view(levels, np.float64, n_levels)
        win = _view(windows, np.int32, 2 * n_windows).reshape(n_windows, 2)
        fm = _block(fmet, np.float64, n_scen, (1 + n_windows) * ld, 1 + n_windows, n, ld)
        im = _block(imet, np.int32, n_scen, (2 + 2 * n_levels) * ld, 2 + 2 * n_levels, n, ld)
        if first_call:
            fm[:, 0], fm[:, 1:] = -np.inf, 0.0
            im[:, 0], im[:, 1] = -1, 0
            im[:, 2:2 + n_levels], im[:, 2 + n_levels:] = -1, 0
        if n_rows == 0:
            return 0
        x = _block(rows, dtype, n_scen, scen_stride, n_rows, n, ld)
        st = _view(steps, np.int32, n_rows)
        with np.errstate(invalid="ignore"):
            for k in range(n_rows):
                t = int(st[k])
                Tw = x[:, k].astype(np.float64)
                im[:, 1] += np.isnan(Tw)
                up = Tw > fm[:, 0]
                fm[:, 0] = np.where(up, Tw, fm[:, 0])
                im[:, 0] = np.where(up, t, im[:, 0])
                for l in range(n_levels):
                    at = Tw >= lv[l]
                    im[:, 2 + n_levels + l] += at
                    im[:, 2 + l] = np.where(at & (im[:, 2 + l] < 0), t, im[:, 2 + l])
                for w in range(n_windows):
                    if win[w, 0] <= t < win[w, 1]:
                        fm[:, 1 + w] = fm[:, 1 + w] + Tw
        return 0

    def fiveeq_traj_metrics_f64(self, *a):
        return self._metrics(np.float64, *a)

    def fiveeq_traj_metrics_f32(self, *a):
        return self._metrics(np.float32, *a)

    def fiveeq_last_error(self):
        return b""


class _Check:
    @staticmethod
    def check(lib, rc):
        if rc != 0:
            raise RuntimeError(f"host pass returned {rc}")


def install():
    """Put the NumPy pass behind metrics.py's switch for the rest of the process (spawned test workers); returns the previous
    (_lib_and_stream, _passes_apply)."""
    import torch

    from . import metrics
    saved = metrics._lib_and_stream, metrics._passes_apply
    passes = MetricsPasses()
    metrics._lib_and_stream = lambda rows: (passes, _Check, None, contextlib.nullcontext())
    metrics._passes_apply = lambda rows: rows.dtype in (torch.float32, torch.float64)
    return saved


@contextlib.contextmanager
def host_passes():
    """`with host_passes():` — metrics.trajectory_metrics takes HOST rows through the NumPy pass inside the block."""
    from . import metrics
    saved = install()
    try:
        yield
    finally:
        metrics._lib_and_stream, metrics._passes_apply = saved
