"""Plain NumPy reference of the trajectory metrics (include/fiveeq.h, "TRAJECTORY METRICS"), written from the definition and
independent of fiveeqscm_amd/_metrics_host.py: a Python loop over the rows, vectorised over the members, one
`acc = acc + Tw` per row.  Plus THE CASE TABLE (case_table) and the buffer layout (lay_out) that the CPU test of the NumPy twin
and the GPU test of the kernel both iterate."""
import numpy as np


def reference(rows, steps, levels=(), windows=()):
    """rows [n_rows, N] (float32 / float64), steps [n_rows] -> dict of peak [N] f64, t_peak [N] i32, n_nan [N] i32,
    first [L, N] i32, n_above [L, N] i32, wsum [W, N] f64."""
    rows = np.asarray(rows)
    K, N = rows.shape
    L, W = len(levels), len(windows)
    peak = np.full(N, -np.inf)
    t_peak = np.full(N, -1, dtype=np.int32)
    n_nan = np.zeros(N, dtype=np.int32)
    first = np.full((L, N), -1, dtype=np.int32)
    n_above = np.zeros((L, N), dtype=np.int32)
    wsum = np.zeros((W, N))
    with np.errstate(invalid="ignore"):
        for k in range(K):
            t = int(steps[k])
            Tw = rows[k].astype(np.float64)                    # exact widening
            n_nan[np.isnan(Tw)] += 1
            higher = Tw > peak
            peak[higher] = Tw[higher]
            t_peak[higher] = t
            for l, level in enumerate(levels):
                at = Tw >= np.float64(level)
                n_above[l, at] += 1
                first[l, at & (first[l] < 0)] = t
            for w, (a, b) in enumerate(windows):
                if a <= t < b:
                    acc = wsum[w]
                    acc = acc + Tw
                    wsum[w] = acc
    return {"peak": peak, "t_peak": t_peak, "n_nan": n_nan, "first": first, "n_above": n_above, "wsum": wsum}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_equal(got, want, where=""):
    for key, w in want.items():
        g = np.asarray(got[key])
        assert g.dtype == w.dtype and g.shape == w.shape, (where, key, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(bits(g), bits(w)), (where, key)


# ---- the shared case table --------------------------------------------------------------------------------------------------
LEVELS8 = (1.5, 0.0, 2.0, -0.5, 0.75, 3.0, 1.0, 2.5)           # unsorted; 0.0 meets the row of -0.0
STEPS_BASE = (3, 4, 9, 10, 40, 41, 42, 57, 60, 61, 70, 71, 72, 90, 91, 100, 130, 131, 150, 151, 152, 153, 170, 200, 201)


def steps_of(n_rows):
    s = list(STEPS_BASE[:n_rows])
    while len(s) < n_rows:
        s.append(s[-1] + 1 + len(s) % 3)
    return np.asarray(s, dtype=np.int64)


def windows_of(steps, W):
    """W windows over `steps`: both boundaries BETWEEN stored steps (where the steps have gaps), an empty window, and two
    windows that overlap the first."""
    lo, hi = int(steps[0]), int(steps[-1])
    mid = int(steps[len(steps) // 2])
    gaps = [int(steps[i]) + 1 for i in range(len(steps) - 1) if steps[i + 1] - steps[i] > 1]      # values no row holds
    first = (gaps[0], gaps[-1]) if len(gaps) >= 2 else (lo, hi + 1)
    return tuple([first, (hi + 5, hi + 9), (lo, hi + 1), (mid, mid + 3)][:W])


def spec_of(L, W, steps):
    return LEVELS8[:L] if L < 8 else LEVELS8, windows_of(steps, W)


def make_rows(n_rows, n, dtype, seed, level=1.5):
    """[n_rows, n] on the grid 0.25 * integers in [-4, 12] (ties at the peak and exact hits of a level are common), with the
    planted members, as far as n has room: NaN at the first / a middle / the last row, all NaN, +inf, -inf, a member constant
    at the level; and row 1 (if there is one) is -0.0 throughout the first quarter of the members."""
    rng = np.random.default_rng(seed)
    x = (0.25 * rng.integers(-4, 13, size=(n_rows, n))).astype(dtype)
    plant = [k for k in range(7) if 8 + k < n]
    col = lambda k: n - 1 - k                                  # noqa: E731  (planted at the END: the ragged tail lanes)
    for k in plant:
        c = col(k)
        if k == 0:
            x[0, c] = np.nan
        elif k == 1:
            x[n_rows // 2, c] = np.nan
        elif k == 2:
            x[n_rows - 1, c] = np.nan
        elif k == 3:
            x[:, c] = np.nan
        elif k == 4:
            x[n_rows // 2, c] = np.inf
        elif k == 5:
            x[n_rows // 2, c] = -np.inf
        elif k == 6:
            x[:, c] = level
    if n_rows > 1 and n >= 64:
        x[1, :n // 4] = -0.0
    return x


def has_tie_and_hit(x, levels):
    """At least one member attains its peak twice, and at least one value equals a level exactly."""
    with np.errstate(invalid="ignore"):
        pk = np.nanmax(np.where(np.isnan(x), -np.inf, x), axis=0)
        tie = bool(((x == pk[None, :]).sum(axis=0) >= 2).any())
        hit = any(bool((x == np.asarray(lv, dtype=x.dtype)).any()) for lv in levels) if len(levels) else True
    return tie, hit


# ---- THE CASE TABLE: iterated by tests/test_traj_metrics_cpu.py (the NumPy twin) and tests/test_traj_metrics_gpu.py (the kernel)
def sizes_of(tile):
    """n_members at the edges of a wave and of a workgroup's tile."""
    return [1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 3]


def case_table(tile, unroll, unroll_narrow):
    """Every case as a dict: n members, k rows, (L, W), and the layout — off: elements the row base is off a 16-byte boundary,
    ld, S scenarios, gap: elements between scenario blocks beyond k * ld — with a seed per scenario.
    Rows: the edges {1, U - 1, U, U + 1, 2 U + 1} of the 16-byte loop (U = unroll) and, where they differ, of the element-load
    loop (unroll_narrow).  (L, W) in {(0, 0), (1, 0), (0, 1), (8, 4)}.  Layouts: aligned with ld = n; one element off with
    ld = n + 5 and S = 3; aligned with ld = n + 5; S = 3 with ld = n — and, once per size, S = 3 with ld rounded up to whole
    16-byte groups so that every scenario takes the 16-byte loads.  `per16` (elements per 16 bytes) scales the gap."""
    U, V = unroll, unroll_narrow
    combos = [(1, 0, 0), (U - 1, 1, 0), (U, 0, 1), (U + 1, 8, 4), (2 * U + 1, 8, 4)]
    combos += [(k, L, W) for k, L, W in ((V, 1, 0), (V + 1, 0, 1), (2 * V + 1, 8, 4)) if k not in [c[0] for c in combos]]
    table = []
    for slot, n in enumerate(sizes_of(tile)):
        for i, (k, L, W) in enumerate(combos):
            layouts = [(0, 0, 1, False), (1, 5, 3, False)]
            if L == 8:
                layouts += [(0, 5, 1, False), (0, 0, 3, k == 2 * U + 1)]
            for off, pad, S, round_up in layouts:
                table.append(dict(n=n, k=k, L=L, W=W, off=off, pad=pad, S=S, round_up=round_up,
                                  seeds=[17 * slot + i] + [1000 + 17 * slot + i + s for s in range(1, S)]))
    return table


def ld_of(case, itemsize):
    per16 = 16 // itemsize
    return -(-case["n"] // per16) * per16 if case["round_up"] else case["n"] + case["pad"]


def lay_out(xs, ld, off, gap):
    """xs: one [k, n] array per scenario -> (flat host buffer, scenario stride): rows ld apart from element `off`, scenario
    blocks k * ld + gap apart, 99 in every element that is no member's."""
    S, (K, n) = len(xs), xs[0].shape
    stride = K * ld + gap
    host = np.full(off + S * stride + 4, 99.0, dtype=xs[0].dtype)
    for s, x in enumerate(xs):
        host[off + s * stride: off + s * stride + K * ld].reshape(K, ld)[:, :n] = x
    return host, stride


_CASES = {}


def case_data(k, n, dtype, seed, L, W):
    """(rows, steps, levels, windows, reference) of one scenario of a case, computed once, shared and read-only.  Checked here,
    on the CPU, for every case that can have them (at least two rows, at least 63 members — one row or one member cannot
    tie): some member attains its peak twice, and some value equals a level exactly."""
    key = (k, n, np.dtype(dtype).name, seed, L, W)
    if key not in _CASES:
        steps = steps_of(k)
        levels, windows = spec_of(L, W, steps)
        x = make_rows(k, n, dtype, seed)
        x.setflags(write=False)
        if k >= 2 and n >= 63:
            assert has_tie_and_hit(x, levels) == (True, True), key
        _CASES[key] = (x, steps, levels, windows, reference(x, steps, levels, windows))
    return _CASES[key]
