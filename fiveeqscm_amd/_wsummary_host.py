"""NumPy restatement of the four WEIGHTED summary passes of the C ABI (include/fiveeq.h, "WEIGHTED SUMMARY":
fiveeq_wrow_moments_*, fiveeq_whist_rows_ranged_*, fiveeq_wselect_bins_*, fiveeq_wselect_pick_*) behind the same
pointer-and-size signatures.

NOT a fallback: the product summarises device rows through the HIP passes and refuses host rows.  `host_passes()` puts this
object behind the switch distributed.py's summaries share (_lib_and_stream / _passes_apply), so that the HOST side of
gather_weighted_summary — the integer ranks, which bins are marked, the residual targets, the exchanges over gloo — runs on
CPU tensors where there is no GPU (tests/test_weighted_summary_cpu.py).
"""
import contextlib
import ctypes

import numpy as np

_CT = {np.float64: ctypes.c_double, np.float32: ctypes.c_float, np.int64: ctypes.c_int64, np.uint64: ctypes.c_uint64,
       np.uint32: ctypes.c_uint32}
WMOM_WORDS = 8


def _view(ptr, dtype, count):
    addr = ptr.value if isinstance(ptr, ctypes.c_void_p) else int(ptr)
    if count == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array((_CT[dtype] * count).from_address(addr))


def _row(ptr, dtype, k, n, ld):
    return _view(ptr, dtype, k * ld + n)[k * ld:k * ld + n]


def bin_rule(x, lo, hi, n_bins, dtype):
    """THE BIN RULE of include/fiveeq.h; NaN -> -1.  fp32 rows: one fp32 FMA (evaluated in fp64, rounded to fp32 once)."""
    inv_w = n_bins / (hi - lo) if hi > lo else 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        if dtype == np.float32:
            big = 3.0e38
            scale = np.float64(np.float32(min(max(inv_w, -big), big)))
            offset = np.float64(np.float32(min(max(-lo * inv_w, -big), big)))
            pos = (x.astype(np.float64) * scale + offset).astype(np.float32)
        else:
            pos = (x - lo) * inv_w
        b = np.trunc(np.clip(np.nan_to_num(pos, nan=0.0, posinf=np.inf, neginf=-np.inf), 0.0, n_bins - 1)).astype(np.int64)
    return np.where(np.isnan(x), -1, b)


class WeightedPasses:
    """The four passes with the C ABI's signatures; `stream` is ignored.  Every function returns 0."""

    def fiveeq_wrow_moments_chunks(self, n_rows, n):
        return 1 if n_rows > 0 and n > 0 else 0

    def _moments(self, dtype, n_rows, n, ld, rows, weights, partial, moments, stream):
        w = _view(weights, np.uint64, n)
        pos = w > 0
        wd = w[pos].astype(np.float64)
        out = _view(moments, np.float64, n_rows * WMOM_WORDS).reshape(n_rows, WMOM_WORDS)
        for k in range(n_rows):
            x = _row(rows, dtype, k, n, ld)[pos].astype(np.float64)
            live = x[~np.isnan(x)]
            with np.errstate(invalid="ignore", over="ignore"):
                out[k, :5] = ((wd * x).sum(), (wd * x * x).sum(), (wd * wd).sum(), live.min() if live.size else np.inf,
                              live.max() if live.size else -np.inf)
            flags = (1 if np.isnan(x).any() else 0) | (2 if (w > np.uint64(1 << 32)).any() else 0)
            out[k, 5:].view(np.uint64)[:] = (int(pos.sum()), flags, int(w.sum(dtype=np.uint64)))
        return 0

    def _hist(self, dtype, n_rows, n, ld, rows, weights, ranges, n_bins, hist, stream):
        w = _view(weights, np.uint64, n)
        rg = _view(ranges, np.float64, n_rows * 2).reshape(n_rows, 2)
        h = _view(hist, np.uint64, n_rows * n_bins).reshape(n_rows, n_bins)
        for k in range(n_rows):
            b = bin_rule(_row(rows, dtype, k, n, ld), rg[k, 0], rg[k, 1], n_bins, dtype)
            ok = (b >= 0) & (w > 0)
            np.add.at(h[k], b[ok], w[ok])                       # integer adds: exact
        return 0

    def _select(self, dtype, n_rows, n, ld, rows, weights, ranges, n_bins, binmask, cand, candw, cap, cand_n, stream):
        w = _view(weights, np.uint64, n)
        rg = _view(ranges, np.float64, n_rows * 2).reshape(n_rows, 2)
        words = (n_bins + 31) // 32
        mask = _view(binmask, np.uint32, n_rows * words).reshape(n_rows, words)
        out = _view(cand, dtype, n_rows * cap).reshape(n_rows, cap) if cap else None
        outw = _view(candw, np.uint64, n_rows * cap).reshape(n_rows, cap) if cap else None
        cn = _view(cand_n, np.uint64, n_rows)
        for k in range(n_rows):
            bits = np.unpackbits(mask[k].view(np.uint8), bitorder="little")[:n_bins].astype(bool)
            x = _row(rows, dtype, k, n, ld)
            b = bin_rule(x, rg[k, 0], rg[k, 1], n_bins, dtype)
            sel = (b >= 0) & (w > 0) & bits[np.maximum(b, 0)]
            px, pw = x[sel][::-1], w[sel][::-1]                 # any order: the kernel's is not the row's either
            start = int(cn[k])
            cn[k] += np.uint64(px.size)
            room = max(0, min(px.size, cap - start))
            if room:
                out[k, start:start + room] = px[:room]
                outw[k, start:start + room] = pw[:room]
        return 0

    def _pick(self, dtype, n_rows, n_seg, width, pool, poolw, seg_n, n_targets, targets, picked, stream):
        p = _view(pool, dtype, n_rows * n_seg * width).reshape(n_rows, n_seg, width)
        pw = _view(poolw, np.uint64, n_rows * n_seg * width).reshape(n_rows, n_seg, width)
        sn = _view(seg_n, np.uint64, n_rows * n_seg).reshape(n_rows, n_seg)
        tg = _view(targets, np.int64, n_rows * n_targets).reshape(n_rows, n_targets)
        out = _view(picked, np.float64, n_rows * n_targets).reshape(n_rows, n_targets)
        for k in range(n_rows):
            keep = [slice(0, min(int(sn[k, g]), width)) for g in range(n_seg)]
            c = np.concatenate([p[k, g, keep[g]] for g in range(n_seg)]).astype(np.float64)
            cw = np.concatenate([pw[k, g, keep[g]] for g in range(n_seg)])
            order = np.argsort(c, kind="stable")
            c, cum = c[order], np.cumsum(cw[order], dtype=np.uint64)
            for q in range(n_targets):
                t = int(tg[k, q])
                at = int(np.searchsorted(cum, np.uint64(max(t, 0)), side="left")) if c.size else 0
                out[k, q] = c[at] if t >= 1 and at < c.size else np.nan
        return 0

    def fiveeq_last_error(self):
        return b""


for _name, _dt in (("f64", np.float64), ("f32", np.float32)):
    for _fn, _impl in (("fiveeq_wrow_moments", "_moments"), ("fiveeq_whist_rows_ranged", "_hist"),
                       ("fiveeq_wselect_bins", "_select"), ("fiveeq_wselect_pick", "_pick")):
        setattr(WeightedPasses, f"{_fn}_{_name}",
                (lambda impl, dt: lambda self, *a: getattr(self, impl)(dt, *a))(_impl, _dt))


class _Check:
    @staticmethod
    def check(lib, rc):
        if rc != 0:
            raise RuntimeError(f"host pass returned {rc}")


def install():
    """Put the NumPy passes behind distributed.py's switch for the rest of the process (spawned test workers); returns the
    previous (_lib_and_stream, _passes_apply)."""
    import torch

    from . import distributed
    saved = distributed._lib_and_stream, distributed._passes_apply
    passes = WeightedPasses()
    distributed._lib_and_stream = lambda rows: (passes, _Check, ctypes, None)
    distributed._passes_apply = lambda rows: rows.dtype in (torch.float32, torch.float64)
    return saved


@contextlib.contextmanager
def host_passes():
    """`with host_passes():` — gather_weighted_summary takes HOST rows through the NumPy passes inside the block."""
    from . import distributed
    saved = install()
    try:
        yield
    finally:
        distributed._lib_and_stream, distributed._passes_apply = saved
