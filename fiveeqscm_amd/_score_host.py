"""NumPy restatement of the SCORING STORED ROWS pass of the C ABI (include/fiveeq.h, "SCORING STORED ROWS": fiveeq_score_rows_f64
/ _f32) behind the same pointer-and-size signature, bit for bit: the accumulators are fp64 sums taken in row order, every
operation rounded on its own.

NOT a fallback: the product takes device rows through the HIP kernel and refuses host rows.  `host_passes()` puts this object
behind constrain.py's switch (_lib_and_stream / _passes_apply), in the role _metrics_host.py plays for the trajectory metrics, so
that the HOST side of constrain.score_rows and EnsembleEngine.score — shapes, strides, the step checks, `acc=` continuation,
the coverage check — runs on CPU tensors where there is no GPU (tests/test_score_cpu.py).
"""
import contextlib

import numpy as np

from ._metrics_host import _Check, _view


class ScorePasses:
    """fiveeq_score_rows_* with the C ABI's signature; `stream` is ignored.  Returns 0.  Like the kernel it reads no element of a
    row-quantity whose record is dead, and skips a row whose step lies outside the tables."""

    def _score(self, dtype, n_q, n_rows, n, rows, row_stride, q_stride, steps, obs, n_steps, misfit, ld_m, stream):
        if n_rows == 0:
            return 0
        st = _view(steps, np.int32, n_rows)
        ob = _view(obs, np.float64, n_q * n_steps * 4).reshape(n_q, n_steps, 4)
        acc = _view(misfit, np.float64, (3 * n_q - 1) * ld_m + n)
        base = rows.value if hasattr(rows, "value") else int(rows)
        size = np.dtype(dtype).itemsize
        with np.errstate(invalid="ignore", over="ignore"):
            for j in range(n_q):
                A, U, V = (acc[(3 * j + w) * ld_m:(3 * j + w) * ld_m + n] for w in range(3))
                for k in range(n_rows):
                    t = int(st[k])
                    if not 0 <= t < n_steps:
                        continue
                    o, p, b = ob[j, t, 0], ob[j, t, 1], ob[j, t, 2]
                    if p == 0.0 and b == 0.0:
                        continue
                    Tw = _view(base + (k * row_stride + j * q_stride) * size, dtype, n).astype(np.float64)
                    A[:] = A + b * Tw
                    d = Tw - o
                    pd = p * d
                    U[:] = U + pd
                    V[:] = V + pd * d
        return 0

    def fiveeq_score_rows_f64(self, *a):
        return self._score(np.float64, *a)

    def fiveeq_score_rows_f32(self, *a):
        return self._score(np.float32, *a)

    def fiveeq_last_error(self):
        return b""


def install():
    """Put the NumPy pass behind constrain.py's switch for the rest of the process; returns the previous (_lib_and_stream,
    _passes_apply)."""
    import torch

    from . import constrain
    saved = constrain._lib_and_stream, constrain._passes_apply
    passes = ScorePasses()
    constrain._lib_and_stream = lambda rows: (passes, _Check, None, contextlib.nullcontext())
    constrain._passes_apply = lambda rows: rows.dtype in (torch.float32, torch.float64)
    return saved


@contextlib.contextmanager
def host_passes():
    """`with host_passes():` — constrain.score_rows takes HOST rows through the NumPy pass inside the block."""
    from . import constrain
    saved = install()
    try:
        yield
    finally:
        constrain._lib_and_stream, constrain._passes_apply = saved
