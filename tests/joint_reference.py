"""Independent reference for the JOINT STATISTICS passes (include/fiveeq.h): exact rational arithmetic over the exactly
converted inputs, rounded once at the end, and the case table the CPU and GPU tests share.

Every input is a binary float, so it is a Fraction with a power-of-two denominator; the sums are taken over Python integers
on one common denominator (which is what adding such Fractions does, without normalising after every term) and turned into a
Fraction once.  With every fp64 sum of n terms comes the exact sum of the absolute terms: the tests' only tolerance for sums is
    (n + 4) * 2**-53 * sum |term|
— the worst case of any summation order (n - 1 roundings, each at most 2**-53 of a partial sum that is at most sum |term|),
plus the three roundings inside a term (the difference, the product with the weight, the last product or the fma).  Derived,
not measured.
"""
from fractions import Fraction

import numpy as np

W_ONE = 1 << 32
U = 2.0 ** -53


def _ints(vals, shift):
    """exact integers v * 2**shift of an array of binary floats"""
    out = []
    for v in vals:
        f = Fraction(float(v))
        out.append(f.numerator * ((1 << shift) // f.denominator))
    return out


def _shift(*arrays):
    """the smallest power-of-two denominator that holds every finite value"""
    s = 0
    for a in arrays:
        for v in np.asarray(a, dtype=np.float64).reshape(-1):
            if np.isfinite(v):
                s = max(s, Fraction(float(v)).denominator.bit_length() - 1)
    return s


def _fl(num, shift):
    return float(Fraction(num, 1 << shift))


def tol(n_terms, abs_sum):
    return (n_terms + 4) * U * abs_sum


def finished_tol(n_terms):
    """The bound for the finished statistics, from the bound for sums.  With the pivots at the means, cov = co / W up to terms
    of second order in (pivot - mean), and by Cauchy-Schwarz sum w |dx| |dy| <= W sqrt(var_x var_y): the bound for co is at most
    (n + 4) 2**-53 sqrt(var_x var_y) in cov — twice that allows for the correction sx sy / W, the pivots' own rounding and the
    closing divisions.  corr adds the relative errors of the two variances, each at most (n + 4) 2**-53 by the same argument:
    4 (n + 4) 2**-53 absolute, as |corr| <= 1.  eta2 = num / den with num = sum_b S_b^2 / W_b - sy^2 / W: the bound for S_b
    times 2 |S_b| / W_b, with |S_b| <= sqrt(W_b sum_b w dy^2), sums over the bins to at most 2 (n + 4) 2**-53 den; den itself
    carries (n + 4) 2**-53 den and eta2 <= 1: again 4 (n + 4) 2**-53 absolute.  Returns (cov bound in units of
    sqrt(var_x var_y), bound for corr and eta2)."""
    return 2 * (n_terms + 4) * U, 4 * (n_terms + 4) * U


class Ref:
    """The exact results of both passes for x [Kx, n], y [Ky, n] (any float dtype: widened exactly), integer weights w [n],
    pivots [Kx + Ky] and, for the conditional sums, edges [Kx, B - 1].  Members of weight 0 do not exist.  Rows with a NaN
    under positive weight are reported in `nan` (their sums are NaN by definition and are not computed)."""

    def __init__(self, x, y, w, pivots, edges=None):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        w = [int(v) for v in w]
        keep = [m for m, v in enumerate(w) if v > 0]
        self.Kx, self.Ky, self.n = x.shape[0], y.shape[0], len(keep)
        self.W = sum(w[m] for m in keep)
        self.wk = [w[m] for m in keep]
        v = np.concatenate([x, y])[:, keep]
        R = self.Kx + self.Ky
        self.nan = np.isnan(v).any(axis=1)
        self.nanw = [sum(wv for wv, bad in zip(self.wk, np.isnan(v[r])) if bad) for r in range(R)]
        v = np.where(np.isnan(v), 0.0, v)                     # placeholders: rows in self.nan are never compared
        s = self.s = _shift(v, pivots)
        c = _ints(pivots, s)
        self.d = [[a - c[r] for a in _ints(v[r], s)] for r in range(R)]       # d * 2**s, exact
        self.xk = x[:, keep]
        self.edges = None if edges is None else np.asarray(edges, dtype=np.float64)

    def moments(self):
        """co [Kx, Ky], margins [R, 2] as floats, with the matching sums of absolute terms"""
        Kx, Ky, s, wk, d = self.Kx, self.Ky, self.s, self.wk, self.d
        co, co_abs = np.zeros((Kx, Ky)), np.zeros((Kx, Ky))
        wd = [[wv * a for wv, a in zip(wk, row)] for row in d]
        for i in range(Kx):
            for j in range(Ky):
                terms = [a * b for a, b in zip(d[i], wd[Kx + j])]
                co[i, j], co_abs[i, j] = _fl(sum(terms), 2 * s), _fl(sum(abs(t) for t in terms), 2 * s)
        mar, mar_abs = np.zeros((Kx + Ky, 2)), np.zeros((Kx + Ky, 2))
        for r in range(Kx + Ky):
            mar[r, 0], mar_abs[r, 0] = _fl(sum(wd[r]), s), _fl(sum(abs(t) for t in wd[r]), s)
            sq = sum(a * b for a, b in zip(wd[r], d[r]))
            mar[r, 1] = mar_abs[r, 1] = _fl(sq, 2 * s)
        return co, co_abs, mar, mar_abs

    def bins(self):
        """[Kx][n] the bin of every member with w > 0 (-1: NaN), by THE BIN RULE on exact comparisons of floats"""
        out = []
        for i in range(self.Kx):
            b = (self.edges[i][:, None] < self.xk[i][None, :]).sum(axis=0)
            out.append(np.where(np.isnan(self.xk[i]), -1, b))
        return out

    def cond(self, n_bins):
        """sums [Kx, B, Ky], their absolute sums, terms per bin [Kx, B], binw [Kx, B] (int), xnan [Kx] (int)"""
        Kx, Ky, s, wk, d = self.Kx, self.Ky, self.s, self.wk, self.d
        sums, sabs = np.zeros((Kx, n_bins, Ky)), np.zeros((Kx, n_bins, Ky))
        cnt, binw, xnan = np.zeros((Kx, n_bins), dtype=np.int64), np.zeros((Kx, n_bins), dtype=np.int64), np.zeros(Kx, dtype=np.int64)
        self.exact_sums = {}
        for i, b in enumerate(self.bins()):
            xnan[i] = sum(wv for wv, k in zip(wk, b) if k < 0)
            for k in range(n_bins):
                sel = [m for m in range(self.n) if b[m] == k]
                cnt[i, k], binw[i, k] = len(sel), sum(wk[m] for m in sel)
                for j in range(Ky):
                    terms = [wk[m] * d[Kx + j][m] for m in sel]
                    self.exact_sums[i, k, j] = Fraction(sum(terms), 1 << s)
                    sums[i, k, j], sabs[i, k, j] = _fl(sum(terms), s), _fl(sum(abs(t) for t in terms), s)
        return sums, sabs, cnt, binw, xnan

    def finished(self, n_bins=None):
        """The exact statistics the Python layer reports: means, variances, cov, corr [Kx, Ky] and (with edges) eta2 —
        Fractions evaluated exactly, rounded once; NaN where the definition says so."""
        Kx, Ky, s, W, wk, d = self.Kx, self.Ky, self.s, self.W, self.wk, self.d
        R = Kx + Ky
        s1 = [Fraction(sum(wv * a for wv, a in zip(wk, d[r])), 1 << s) for r in range(R)]
        s2 = [Fraction(sum(wv * a * a for wv, a in zip(wk, d[r])), 1 << (2 * s)) for r in range(R)]
        var = [(s2[r] - s1[r] * s1[r] / W) / W for r in range(R)]
        cov, corr = np.full((Kx, Ky), np.nan), np.full((Kx, Ky), np.nan)
        for i in range(Kx):
            for j in range(Ky):
                if self.nan[i] or self.nan[Kx + j]:
                    continue
                co = Fraction(sum(wv * a * b for wv, a, b in zip(wk, d[i], d[Kx + j])), 1 << (2 * s))
                c = (co - s1[i] * s1[Kx + j] / W) / W
                cov[i, j] = float(c)
                if var[i] > 0 and var[Kx + j] > 0:
                    corr[i, j] = float(c) / float(np.sqrt(float(var[i]) * float(var[Kx + j])))
        out = {"cov": cov, "corr": corr, "var": np.array([np.nan if self.nan[r] else float(var[r]) for r in range(R)])}
        if n_bins is not None:
            _, _, _, binw, xnan = self.cond(n_bins)
            eta2 = np.full((Kx, Ky), np.nan)
            for i in range(Kx):
                for j in range(Ky):
                    den = s2[Kx + j] - s1[Kx + j] * s1[Kx + j] / W
                    if xnan[i] or self.nan[Kx + j] or den == 0:
                        continue
                    m = s1[Kx + j] / W
                    num = sum(int(binw[i, k]) * (self.exact_sums[i, k, j] / int(binw[i, k]) - m) ** 2 for k in range(n_bins) if binw[i, k])
                    eta2[i, j] = float(num / den)
            out.update(eta2=eta2, bin_weight=binw)
        return out


# ---- the case table: sizes at the edges of the kernels, row counts at the edges of the tiles --------------------------------
def case_table(tile_x, tile_y, chunk, lane_tile):
    """[(n_members, n_x, n_y, n_bins)]: every member count of the list with row and bin counts cycling through their edges; the
    32 x 32 case sits at a small member count (the exact reference is O(n n_x n_y))."""
    return [(1, 1, 1, 1), (63, tile_x, tile_y, 2), (64, tile_x + 1, tile_y + 1, 31), (65, 32, 32, 32),
            (lane_tile - 1, 1, 32, 2), (lane_tile + 1, 32, 1, 31), (chunk - 1, tile_x, tile_y + 1, 32), (chunk, tile_x + 1, tile_y, 1),
            (chunk + 1, 1, tile_y, 2), (2 * chunk + 37, tile_x + 1, tile_y + 1, 32)]


WEIGHT_KINDS = ("ones", "mix", "single")


def case_weights(kind, n, chunk, rng):
    """ones | mix: 0, 1 and 2^32, zeros clustered on one whole wave (members 64..127) and one whole chunk (chunk..2 chunk) |
    single: one non-zero member"""
    if kind == "ones":
        return np.ones(n, dtype=np.int64)
    if kind == "single":
        w = np.zeros(n, dtype=np.int64)
        w[(2 * n) // 3] = 3
        return w
    w = rng.choice(np.array([0, 1, 1, W_ONE], dtype=np.int64), size=n)
    w[64:128] = 0
    w[chunk:2 * chunk] = 0
    if not w.any():
        w[0] = W_ONE
    return w


def case_data(n, n_x, n_y, n_bins, kind, chunk, seed=11):
    """x [n_x, n], y [n_y, n] (fp64 values that fp32 holds exactly, so both dtypes share one reference), w [n] int64, pivots,
    edges [n_x, n_bins - 1] (values of the row: ties sit on edges).  NaN and inf sit under weight 0 where there is one."""
    rng = np.random.default_rng(seed + 1000 * n + 31 * n_x + n_y)
    r32 = lambda a: a.astype(np.float32).astype(np.float64)      # noqa: E731
    x = r32(np.round(rng.normal(size=(n_x, n)) * 64) / 64 + np.arange(n_x)[:, None])
    mix = rng.normal(size=(n_y, n_x)) / np.sqrt(n_x)
    y = r32(mix @ x + 0.5 * rng.normal(size=(n_y, n)) + 10.0)
    w = case_weights(kind, n, chunk, rng)
    zero = np.nonzero(w == 0)[0]
    for k, m in enumerate(zero[:6]):
        x[k % n_x, m] = (np.nan, np.inf, -np.inf)[k % 3]
        y[k % n_y, m] = (np.inf, np.nan, -np.inf)[k % 3]
    live = w > 0
    pivots = r32(np.concatenate([x[:, live].mean(axis=1), y[:, live].mean(axis=1)]))
    edges = np.zeros((n_x, n_bins - 1))
    for i in range(n_x):
        xs = np.sort(x[i, live])
        edges[i] = xs[np.minimum((np.arange(1, n_bins) * xs.size) // n_bins, xs.size - 1)]
    return x, y, w, pivots, edges
