"""Constructed rows for the exact histogram tests (tests/test_hist_reference_cpu.py, tests/test_hist_exact_gpu.py): every bin
edge of THE BIN RULE (include/fiveeq.h) with both neighbours, the special values, the operand triples on which a
double-rounded fp32 FMA gives another float than the correctly rounded one, and the deliberately WRONG rules the tests must
be able to tell from the right one.  The reference is oracle/summary_passes.bin_rule, proved against rational arithmetic in
tests/test_hist_reference_cpu.py.  Plain NumPy, no GPU."""
import functools
from fractions import Fraction

import numpy as np

from oracle.summary_passes import bin_rule, fma_f32, rule_constants_f32

F32, F64 = np.float32, np.float64
# (lo, hi) of section 2 of the issue: near zero; the header's far-from-zero example; a width that is a power-of-two multiple of
# every power-of-two n_bins (inv_w exact); hi - lo = 1e-40 (the fp32 constants are clamped to +-3e38); lo = -1e30
RANGES = ((-0.3, 7.1), (280.0, 295.0), (-4.0, 12.0), (0.0, 1e-40), (-1e30, 3e30))
N_BINS = (1, 2, 3, 4095, 4096)


# ---- exact fp32 arithmetic by rational numbers ------------------------------------------------------------------------------
def round_to_f32(q):
    """The fp32 value nearest the rational q, ties to even, subnormals and overflow to +-inf included (as a Python float)."""
    if q == 0:
        return 0.0
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1                                              # 2^e <= a < 2^(e+1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n = a / quantum
    r = n.numerator // n.denominator
    rest = n - r
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and r % 2 == 1):
        r += 1
    v = r * quantum
    out = float("inf") if v >= Fraction(2) ** 128 else float(v)
    return -out if q < 0 else out


def fma_exact(x, a, c):
    """fma(x, a, c) of three finite fp32 values by rational arithmetic, rounded once."""
    return round_to_f32(Fraction(float(x)) * Fraction(float(a)) + Fraction(float(c)))


def fma_double_rounded(x, a, c):
    """The restatement the reference used to be: product and sum in fp64 (the sum ROUNDS), then a second rounding to fp32."""
    x, a, c = (np.asarray(v, dtype=F32).astype(F64) for v in (x, a, c))
    with np.errstate(invalid="ignore", over="ignore"):
        return (x * a + c).astype(F32)


# ---- operand triples that tell the two apart -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def double_rounding_triples(n_bins=4096, count=128):
    """[(x, scale, offset, k)]: fp32 triples, FOUND BY SEARCH, whose exact fma(x, scale, offset) is pred(k) (bin k - 1) while
    the double-rounded restatement gives k (bin k).  The search: 24-bit integers u, v with u v = 2^47 - d, 0 < d < 2^18, so
    that x scale = h (1 - d 2^-47) with h = half an fp32 ulp of offset = pred(k): the fp64 sum rounds to the exact midpoint
    of pred(k) and k, the second rounding then ties to the even k; the exact sum lies below the midpoint.  Every candidate is
    checked with both evaluations before it is kept."""
    u = np.arange(2 ** 23 + 1, 2 ** 23 + 2 ** 17, dtype=np.int64)
    v = np.rint(2.0 ** 47 / u).astype(np.int64)
    d = 2 ** 47 - u * v
    keep = (d > 0) & (d < 2 ** 18) & (v < 2 ** 24) & (v >= 2 ** 23)
    u, v = u[keep], v[keep]
    out, ks = [], [1, 2, 3, 5, 64, 1000, 2047, 2048, 2049, 4094, 4095]
    for i in range(len(u)):
        k = ks[i % len(ks)]
        if k > n_bins - 1:
            continue
        off = np.nextafter(F32(k), F32(0))                                  # pred(k)
        ek = int(np.floor(np.log2(float(off))))                             # off in [2^ek, 2^(ek+1)): ulp = 2^(ek-23)
        scale = F32(float(v[i]) * 2.0 ** -14)                               # ~2^9 .. 2^10: a range a few units wide
        x = F32(float(u[i]) * 2.0 ** (ek - 24 - 47 + 14))
        good, bad = fma_f32(x, scale, off), fma_double_rounded(x, scale, off)
        if float(good) == float(off) and float(bad) == float(k) and fma_exact(x, scale, off) == float(off):
            out.append((x, scale, off, k))
        if len(out) == count:
            break
    return tuple(out)


def triple_range(scale, offset, n_bins):
    """A (lo, hi) in fp64 whose fp32 rule constants are exactly (scale, offset); None if rounding does not land there."""
    w = F64(n_bins) / F64(scale)
    lo = -F64(offset) * w / F64(n_bins)
    hi = lo + w
    inv_w = F64(n_bins) / (hi - lo)
    s, o = rule_constants_f32(lo, inv_w)
    return (float(lo), float(hi)) if (s == scale and o == offset) else None


# ---- the rule's edges ---------------------------------------------------------------------------------------------------------------
def edges_of_rule(lo, hi, n_bins, dtype):
    """For k = 1 .. n_bins - 1: the smallest finite value of `dtype` whose bin is >= k, found by bisection on the ordered
    values with the reference itself (the rule is monotone) — for fp32 rows this solves fma(x, scale, offset) = k."""
    big = np.finfo(dtype).max
    k = np.arange(1, n_bins, dtype=np.int64)
    a = np.full(k.shape, -big, dtype=dtype)                                  # bin(a) < k (bin 0), unless nothing is
    b = np.full(k.shape, big, dtype=dtype)                                   # bin(b) >= k (the top bin)
    ok = (bin_rule(b, lo, hi, n_bins, dtype) >= k) & (bin_rule(a, lo, hi, n_bins, dtype) < k)
    ia, ib = _to_key(a), _to_key(b)
    while True:
        go = ok & (ia + 1 < ib)
        if not go.any():
            break
        im = (ia >> 1) + (ib >> 1) + (ia & ib & 1)              # (the fp64 keys span more than 2^63: no ib - ia)
        up = bin_rule(_from_key(im, dtype), lo, hi, n_bins, dtype) >= k
        ib = np.where(go & up, im, ib)
        ia = np.where(go & ~up, im, ia)
    return _from_key(ib, dtype)[ok]


def _to_key(x):
    """Monotone map of finite floats to int64 (object arithmetic avoided: fp64 keys fit because only finite values occur)."""
    if x.dtype == F32:
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    i = x.view(np.int64)
    return np.where(i < 0, -(i & np.int64(0x7FFFFFFFFFFFFFFF)), i)


def _from_key(key, dtype):
    if dtype == F32:
        i = np.where(key < 0, (-key) | 0x80000000, key).astype(np.uint32)
        return i.view(F32)
    i = np.where(key < 0, (-key).astype(np.uint64) | np.uint64(0x8000000000000000), key.astype(np.uint64))
    return i.astype(np.uint64).view(F64)


def specials(lo, hi, dtype):
    fi = np.finfo(dtype)
    tiny_sub = np.nextafter(dtype(0), dtype(1))
    v = [lo, hi, 0.0, -0.0, np.inf, -np.inf, fi.max, -fi.max, fi.tiny, -fi.tiny, tiny_sub, -tiny_sub, fi.tiny / 4, -fi.tiny / 4,
         1e30, -1e30, 1.0, -1.0]
    with np.errstate(over="ignore"):
        return np.array(v, dtype=F64).astype(dtype)


@functools.lru_cache(maxsize=None)
def edge_pool(lo, hi, n_bins, dtype):
    """Every edge of the range with both neighbours, in `dtype`: the arithmetic edges lo + k w (k = 0 .. n_bins) rounded to the
    row type, the edges of the rule itself (edges_of_rule), lo, hi, the special values; shuffled once (seeded).  No NaN: the
    callers scatter those by position."""
    w = (F64(hi) - F64(lo)) / n_bins
    with np.errstate(over="ignore", invalid="ignore"):
        arith = (F64(lo) + np.arange(n_bins + 1, dtype=F64) * w).astype(dtype)
    base = np.concatenate([arith, edges_of_rule(lo, hi, n_bins, dtype), specials(lo, hi, dtype)])
    with np.errstate(over="ignore"):
        pool = np.concatenate([base, np.nextafter(base, dtype(-np.inf)), np.nextafter(base, dtype(np.inf))])
    pool = pool[~np.isnan(pool)]
    return np.random.default_rng(n_bins).permutation(pool)


def row_of(pool, n, nan_at=()):
    """n members: the pool repeated / cut to length, NaN at the given positions (those < n)."""
    x = np.resize(pool, n).copy()
    for i in nan_at:
        if -n <= i < n:
            x[i] = np.nan
    return x


NAN_AT = (0, -1, 37, 100)                                   # first, last, mid-wave (lane 37 of waves 0 and 1)


def counts(x, lo, hi, n_bins, dtype, rule=bin_rule):
    b = rule(x, lo, hi, n_bins, dtype)
    return np.bincount(b[b >= 0], minlength=n_bins).astype(np.int64)


# ---- the deliberately wrong rules (fp32 rows) ---------------------------------------------------------------------------------
def _finish(pos, x, n_bins):
    with np.errstate(invalid="ignore"):
        b = np.trunc(np.clip(np.nan_to_num(pos, nan=0.0, posinf=np.inf, neginf=-np.inf), 0.0, n_bins - 1)).astype(np.int64)
    return np.where(np.isnan(x), -1, b)


def _consts(lo, hi, n_bins):
    lo, hi = F64(lo), F64(hi)
    with np.errstate(over="ignore", divide="ignore"):
        inv_w = F64(n_bins) / (hi - lo) if hi > lo else F64(0.0)
    return (inv_w,) + rule_constants_f32(lo, inv_w)


def wrong_fp64_formula(x, lo, hi, n_bins, dtype):
    """fp32 rows binned with the fp64 formula."""
    return bin_rule(np.asarray(x).astype(F64), lo, hi, n_bins, F64)


def wrong_double_rounded(x, lo, hi, n_bins, dtype):
    """The FMA restated in fp64 and rounded twice."""
    _, s, o = _consts(lo, hi, n_bins)
    return _finish(fma_double_rounded(x, s, o), x, n_bins)


def wrong_truncate_first(x, lo, hi, n_bins, dtype):
    """Truncated to a 32-bit integer BEFORE the clamp (what does not fit becomes INT_MIN, as cvttss2si gives), then clamped."""
    _, s, o = _consts(lo, hi, n_bins)
    pos = fma_f32(x, s, o).astype(F64)
    with np.errstate(invalid="ignore"):
        fits = np.abs(pos) < 2.0 ** 31
        i = np.where(fits, np.trunc(np.where(fits, pos, 0.0)), -2.0 ** 31).astype(np.int64)
    return np.where(np.isnan(x), -1, np.clip(i, 0, n_bins - 1))


def wrong_clamp_first(x, lo, hi, n_bins, dtype):
    """The MEMBER clamped to [(float)lo, (float)hi] before the FMA, the index then capped at n_bins - 1."""
    _, s, o = _consts(lo, hi, n_bins)
    with np.errstate(over="ignore"):
        xc = np.clip(x, F32(lo), F32(hi))
    return _finish(fma_f32(xc, s, o), x, n_bins)


def wrong_packed_pos(x, lo, hi, n_bins, dtype):
    """A packed lane (members 2i, 2i + 1) that takes the first component's pos for both members."""
    _, s, o = _consts(lo, hi, n_bins)
    pos = fma_f32(x, s, o)
    pos[1::2] = pos[0:len(pos) - 1:2][:len(pos[1::2])]
    return _finish(pos, x, n_bins)


WRONG_RULES = {"fp64 formula on fp32 rows": wrong_fp64_formula, "double-rounded FMA": wrong_double_rounded,
               "truncate before clamp": wrong_truncate_first, "clamp before the multiply": wrong_clamp_first,
               "one packed pos for both members": wrong_packed_pos}


def section2_rows_f32():
    """{name: (x, lo, hi, n_bins)}: the fp32 rows of section 2 (every range x n_bins, one row each, plus one row per
    double-rounding triple in the range that gives its constants) — what the teeth of the tests are measured on."""
    rows = {}
    for lo, hi in RANGES:
        for nb in N_BINS:
            pool = edge_pool(lo, hi, nb, F32)
            rows[f"({lo:g}, {hi:g}) x {nb}"] = (row_of(pool, len(pool) | 1, NAN_AT), lo, hi, nb)
    for j, (x, s, o, k) in enumerate(double_rounding_triples()):
        rg = triple_range(s, o, 4096)
        if rg is not None:
            xs = np.array([x, np.nextafter(x, F32(-1)), np.nextafter(x, F32(1))], dtype=F32)
            rows[f"triple {j}"] = (xs, rg[0], rg[1], 4096)
    return rows


def moved(x, lo, hi, n_bins, dtype, rule):
    """Members the wrong rule counts in another bin than the reference (half the L1 distance of the two histograms)."""
    return int(np.abs(counts(x, lo, hi, n_bins, dtype, rule) - counts(x, lo, hi, n_bins, dtype)).sum()) // 2
