"""Independent restatement of the RUNNING MEANS AND TRENDS definitions (include/fiveeq.h), written from the text and not from
fiveeqscm_amd/_smooth_host.py: Python loops over the rows, fp64 values, one `s = s + x` per row, Python's `/` for the one
division.  Plus the two implementations the definition EXCLUDES (a sliding add / subtract update, a multiply by the
reciprocal) so that a test can show its inputs tell them apart, the test inputs, and the buffer layouts and the check that the
CPU test of the NumPy twin and the GPU test of the kernels both run (check_mean / check_trend, through a backend)."""
import ctypes

import numpy as np

SENT = -777.25                                                 # what every output word holds that nothing may write


# ---- the definitions ---------------------------------------------------------------------------------------------------------
def running_mean(x, window):
    """x [n, N] (the whole sequence, tail included) -> [max(0, n - window + 1), N] fp64."""
    x = np.asarray(x)
    n = x.shape[0]
    out = np.empty((max(0, n - window + 1), x.shape[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(out.shape[0]):
            s = x[k].astype(np.float64)                        # exact widening
            for i in range(1, window):
                s = s + x[k + i].astype(np.float64)
            out[k] = s / np.float64(window)
    return out


def sliding_mean(x, window):
    """NOT the definition: the first window summed, then s = s + x[k + window - 1] - x[k - 1]."""
    x = np.asarray(x).astype(np.float64)
    out = np.empty((max(0, x.shape[0] - window + 1), x.shape[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(out.shape[0]):
            if k == 0:
                s = x[0].copy()
                for i in range(1, window):
                    s = s + x[i]
            else:
                s = (s + x[k + window - 1]) - x[k - 1]
            out[k] = s / np.float64(window)
    return out


def reciprocal_mean(x, window):
    """NOT the definition: the definition's sum times the rounded reciprocal of the window."""
    x = np.asarray(x)
    out = np.empty((max(0, x.shape[0] - window + 1), x.shape[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(out.shape[0]):
            s = x[k].astype(np.float64)
            for i in range(1, window):
                s = s + x[k + i].astype(np.float64)
            out[k] = s * (np.float64(1.0) / np.float64(window))
    return out


def trend_sums(rows, steps, windows):
    """rows [n_rows, N], steps [n_rows] -> (sx, stx), each [W, N] fp64."""
    rows = np.asarray(rows)
    sx, stx = np.zeros((len(windows), rows.shape[1])), np.zeros((len(windows), rows.shape[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(rows.shape[0]):
            t = int(steps[k])
            Tw = rows[k].astype(np.float64)
            for w, (a, b) in enumerate(windows):
                if a <= t < b:
                    u = np.float64(t - a)
                    sx[w] = sx[w] + Tw
                    p = u * Tw
                    stx[w] = stx[w] + p
    return sx, stx


def trend_moments(steps, windows):
    """Per window the exact integers (n, su, suu) over the steps inside it, u = t - a."""
    out = []
    for a, b in windows:
        u = [int(t) - a for t in steps if a <= int(t) < b]
        out.append((len(u), sum(u), sum(v * v for v in u)))
    return out


def slope_of(sx, stx, steps, windows, dt):
    """NumPy's evaluation of ((n stx - su sx) / (n suu - su su)) / dt on the sums, NaN below 2 stored steps."""
    out = np.empty_like(sx)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for w, (n, su, suu) in enumerate(trend_moments(steps, windows)):
            n, su, suu = np.float64(n), np.float64(su), np.float64(suu)
            out[..., w, :] = np.nan if n < 2 else ((n * stx[..., w, :] - su * sx[..., w, :]) / (n * suu - su * su)) / np.float64(dt)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- inputs on which order and rounding matter -------------------------------------------------------------------------------
POOL = (1e16, -1e16, 1.0, 3e-7, -0.0, 0.1, -2.5, 1.0 / 3.0, 7e15, -3e-7)


def make_rows(n_rows, n, dtype, seed, nan_row=None):
    """[n_rows, n]: every value drawn from POOL times a random factor in [1, 2) — per member a mix of magnitudes, so that
    ((a + b) + c) != (a + (b + c)) and add-then-subtract differs from a fresh sum — with exact -0.0 entries; and planted from
    the LAST member backwards, as far as n has room (members 0 .. 3 stay finite): +inf at a middle row, -inf at a middle row, a
    NaN at row `nan_row` (default: the middle row) in two members."""
    rng = np.random.default_rng(seed)
    x = (np.asarray(POOL)[rng.integers(0, len(POOL), size=(n_rows, n))] * (1.0 + rng.random((n_rows, n)))).astype(dtype)
    x[rng.random((n_rows, n)) < 0.05] = -0.0
    if n_rows:
        mid = n_rows // 2
        r = mid if nan_row is None else nan_row
        for k, (row, v) in enumerate([(mid, np.inf), (mid, -np.inf), (r, np.nan), (r, np.nan)]):
            if 4 + k < n:
                x[row, n - 1 - k] = v
    return x


def finite_members(x):
    return np.isfinite(np.asarray(x, dtype=np.float64)).all(axis=0)


def steps_of(n_rows, first=3, stride=1):
    return first + stride * np.arange(n_rows, dtype=np.int64)


# ---- the layouts and the check both tests run ----------------------------------------------------------------------------------
class HostBackend:
    """check_mean / check_trend on host buffers through an object with the C ABI's signatures (the NumPy twin)."""

    def __init__(self, lib):
        self.lib = lib

    def put(self, a):
        return a.copy()

    def addr(self, h):
        return h.ctypes.data

    def get(self, h):
        return h

    def check(self, rc):
        assert rc == 0, rc


def _fn(backend, base, dtype):
    return getattr(backend.lib, f"{base}_{'f64' if np.dtype(dtype) == np.float64 else 'f32'}")


def lay_out(xs, ld, off, gap):
    """xs: one [k, n] array per scenario -> (flat buffer, scenario stride): rows ld apart from element `off`, scenario blocks
    k * ld + gap apart, 99 in every element that is no member's."""
    S, (K, n) = len(xs), xs[0].shape
    stride = K * ld + gap
    host = np.full(off + S * stride + 4, 99.0, dtype=xs[0].dtype)
    for s, x in enumerate(xs):
        host[off + s * stride: off + s * stride + K * ld].reshape(K, ld)[:, :n] = x
    return host, stride


def check_mean(backend, xs, window, *, ld, off, gap, cuts=(), want=None):
    """The running mean of one [k, n] array per scenario through backend.lib's fiveeq_running_mean_*: rows laid out by lay_out,
    out [S][n_out][ld] at element `off` behind two guard rows, two more after it, SENT everywhere; the rows handed over in the
    segments `cuts` makes, each with the rows before it as its tail (read in place).  Asserts that the whole out buffer equals,
    bit for bit, SENT with the reference written into the members' columns.  want: the reference per scenario, if the caller
    holds it already."""
    S, (K, n) = len(xs), xs[0].shape
    dtype = xs[0].dtype
    w = dtype.itemsize
    host, stride = lay_out(xs, ld, off, gap)
    n_out = max(0, K - window + 1)
    o_stride = n_out * ld + gap
    out = np.full(off + 2 * ld + S * o_stride + 2 * ld, SENT)
    expect = out.copy()
    for s, x in enumerate(xs):
        ref = running_mean(x, window) if want is None else want[s]
        assert ref.shape == (n_out, n)
        expect[off + 2 * ld + s * o_stride:][:n_out * ld].reshape(n_out, ld)[:, :n] = ref
    rows_h, out_h = backend.put(host), backend.put(out)
    fn = _fn(backend, "fiveeq_running_mean", dtype)
    edges = [0, *cuts, K]
    for a, b in zip(edges[:-1], edges[1:]):
        n_tail = min(window - 1, a)
        done = max(0, a - window + 1)                          # outputs the earlier segments wrote
        tail = ctypes.c_void_p(backend.addr(rows_h) + (off + (a - n_tail) * ld) * w) if n_tail else None
        backend.check(fn(S, b - a, n, ld, ctypes.c_void_p(backend.addr(rows_h) + (off + a * ld) * w), stride, window, n_tail, tail, stride,
                         ctypes.c_void_p(backend.addr(out_h) + (off + 2 * ld + done * ld) * 8), o_stride, None))
    got = backend.get(out_h)
    assert np.array_equal(bits(got), bits(expect)), (n, K, window, ld, off, gap, cuts, np.flatnonzero(bits(got) != bits(expect))[:8])


def check_trend(backend, xs, steps, windows, *, ld, off, gap, cuts=(), poison=False):
    """The same for fiveeq_window_trends_*: tsum [S][2 W][ld] with SENT in the padding columns and a guard word after it;
    first_call = 1 for the first segment (poison: over a state of NaN, which it must not read), 0 for the others."""
    S, (K, n) = len(xs), xs[0].shape
    dtype = xs[0].dtype
    w = dtype.itemsize
    W = len(windows)
    host, stride = lay_out(xs, ld, off, gap)
    ts = np.full(S * 2 * W * ld + 1, SENT)
    expect = ts.copy()
    if poison:
        ts[:-1].reshape(S, 2 * W, ld)[:, :, :n] = np.nan
    for s, x in enumerate(xs):
        sx, stx = trend_sums(x, steps, windows)
        block = expect[s * 2 * W * ld:][:2 * W * ld].reshape(2 * W, ld)
        block[0::2, :n], block[1::2, :n] = sx, stx
    rows_h, ts_h = backend.put(host), backend.put(ts)
    st_h = backend.put(np.asarray(steps, dtype=np.int32))
    c_wn = (ctypes.c_int32 * max(2 * W, 1))(*[v for ab in windows for v in ab])
    fn = _fn(backend, "fiveeq_window_trends", dtype)
    edges = [0, *cuts, K]
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        backend.check(fn(S, b - a, n, ld, ctypes.c_void_p(backend.addr(rows_h) + (off + a * ld) * w), stride,
                         ctypes.c_void_p(backend.addr(st_h) + 4 * a), W, ctypes.cast(c_wn, ctypes.c_void_p), ctypes.c_void_p(backend.addr(ts_h)),
                         1 if i == 0 else 0, None))
    got = backend.get(ts_h)
    assert np.array_equal(bits(got), bits(expect)), (n, K, windows, ld, off, gap, cuts, np.flatnonzero(bits(got) != bits(expect))[:8])


def sizes_of(tile, lane):
    """n_members at the edges of a lane (`lane` members: 16 bytes of a row) and of a workgroup's tile."""
    return sorted({1, lane - 1, lane, lane + 1, tile - 1, tile, tile + 1, 2 * tile + 3} - {0})


def rows_of(window, unrolls):
    return sorted({0, window - 1, window, window + 1, 2 * window + 3} | {u + d for u in unrolls for d in (-1, 0, 1)})


def layouts_of(n, itemsize):
    """(ld, off, gap, S): 16-byte aligned rows with ld a multiple of 16 bytes beyond n — the 16-byte path, the ragged members
    in a launch of their own, guard columns — and one scenario; rows one element off with ld = n + 5 and three scenarios whose
    blocks lie further apart than their rows — the element path."""
    per16 = 16 // itemsize
    return [(-(-n // per16) * per16 + per16, 0, 0, 1), (n + 5, 1, 2 * per16 + 1, 3)]
