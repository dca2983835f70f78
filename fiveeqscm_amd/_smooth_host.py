"""NumPy restatement of the RUNNING MEANS AND TRENDS passes of the C ABI (include/fiveeq.h: fiveeq_running_mean_f64 / _f32,
fiveeq_window_trends_f64 / _f32) behind the same pointer-and-size signatures, bit for bit: every running mean is summed afresh
in ascending row order and divided once, every trend sum is an fp64 sum in row order.

NOT a fallback: the product takes device rows through the HIP kernels and refuses host rows.  `host_passes()` puts this object
behind smooth.py's switch (_lib_and_stream / _passes_apply), in the role _metrics_host.py plays for the trajectory metrics, so
that the HOST side of smooth.running_mean / window_trends — shapes, strides, the step checks, the tail and state continuation,
the dating of the outputs, the slope — runs on CPU tensors where there is no GPU (tests/test_smooth_cpu.py).
"""
import contextlib

import numpy as np

from ._metrics_host import _Check, _block, _view


class SmoothPasses:
    """fiveeq_running_mean_* / fiveeq_window_trends_* with the C ABI's signatures; `stream` is ignored.  Return 0."""

    def _mean(self, dtype, n_scen, n_rows, n, ld, rows, scen_stride, window, n_tail, tail, tail_scen_stride, out, out_scen_stride,
              stream):
        n_out = max(0, n_tail + n_rows - window + 1)
        if n_out == 0:
            return 0
        x = np.concatenate([_block(tail, dtype, n_scen, tail_scen_stride, n_tail, n, ld),
                            _block(rows, dtype, n_scen, scen_stride, n_rows, n, ld)], axis=1)
        o = _block(out, np.float64, n_scen, out_scen_stride, n_out, n, ld)
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(n_out):
                s = x[:, k].astype(np.float64)
                for i in range(1, window):
                    s = s + x[:, k + i].astype(np.float64)
                o[:, k] = s / np.float64(window)
        return 0

    def _trends(self, dtype, n_scen, n_rows, n, ld, rows, scen_stride, steps, n_windows, windows, tsum, first_call, stream):
        if n_windows == 0:
            return 0
        win = _view(windows, np.int32, 2 * n_windows).reshape(n_windows, 2)
        ts = _block(tsum, np.float64, n_scen, 2 * n_windows * ld, 2 * n_windows, n, ld)
        if first_call:
            ts[:] = 0.0
        if n_rows == 0:
            return 0
        x = _block(rows, dtype, n_scen, scen_stride, n_rows, n, ld)
        st = _view(steps, np.int32, n_rows)
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(n_rows):
                t = int(st[k])
                Tw = x[:, k].astype(np.float64)
                for w in range(n_windows):
                    a, b = int(win[w, 0]), int(win[w, 1])
                    if a <= t < b:
                        u = np.float64(t - a)
                        ts[:, 2 * w] = ts[:, 2 * w] + Tw
                        p = u * Tw
                        ts[:, 2 * w + 1] = ts[:, 2 * w + 1] + p
        return 0

    def fiveeq_running_mean_f64(self, *a):
        return self._mean(np.float64, *a)

    def fiveeq_running_mean_f32(self, *a):
        return self._mean(np.float32, *a)

    def fiveeq_window_trends_f64(self, *a):
        return self._trends(np.float64, *a)

    def fiveeq_window_trends_f32(self, *a):
        return self._trends(np.float32, *a)

    def fiveeq_last_error(self):
        return b""


def install():
    """Put the NumPy passes behind smooth.py's switch for the rest of the process (spawned test workers); returns the previous
    (_lib_and_stream, _passes_apply)."""
    import torch

    from . import smooth
    saved = smooth._lib_and_stream, smooth._passes_apply
    passes = SmoothPasses()
    smooth._lib_and_stream = lambda rows: (passes, _Check, None, contextlib.nullcontext())
    smooth._passes_apply = lambda rows: rows.dtype in (torch.float32, torch.float64)
    return saved


@contextlib.contextmanager
def host_passes():
    """`with host_passes():` — smooth.running_mean / window_trends take HOST rows through the NumPy passes inside the block."""
    from . import smooth
    saved = install()
    try:
        yield
    finally:
        smooth._lib_and_stream, smooth._passes_apply = saved
