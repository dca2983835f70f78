"""Independent statements of the two oldest device kernels, written from include/fiveeq.h and the comments above the kernels
(fiveeq_summary.hpp), sharing no code with fiveeqscm_amd:

  lhs_ints        one coordinate of the shard-computable Latin hypercube (fiveeq_lhs_rows_f64) in Python integers and exact
                  rationals: splitmix64, the dimension key, the 4-round Feistel network on half_bits with cycle-walking, the 24
                  jitter bits; u is the correctly rounded value of (stratum 2^25 + 2 jbits + 1) / (2^25 n_total).
  lhs_rows_ref    whole rows of it in wrapping uint64 NumPy and ONE fp64 division of two exactly representable integers.
  hfc_decay_mp    exp(-t), the factor of the reference's one function (fiveeq_hfc_conc_f64: out[k][m] = e0[m] exp(-time[k])), at
                  50 digits, as exact rationals and rounded to the nearest fp64, subnormals included.
  ulp_err         |got - exact| in units of the spacing of the rounded exact value: 2^-1074 throughout the subnormal range.

and the time sets and design sizes that the CPU and the GPU tests of these kernels share.  Nothing here touches torch or the GPU."""
import collections
import functools
import math
from fractions import Fraction

import numpy as np

MASK = (1 << 64) - 1
GOLD, ROUND_ODD = 0x9E3779B97F4A7C15, 0xD1342543DE82EF95          # the dimension key's and the round keys' multipliers
JIT_MUL, JIT_ADD = 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53          # the jitter hash's key
LHS_MAX_TOTAL = 1 << 28                                            # FIVEEQ_LHS_MAX_TOTAL
ROUNDS = 4

# n_total at and around the even powers of two, where half_bits steps and the walked domain is nearly 4 n_total
LHS_TOTALS = (1, 2, 3, 4, 5, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 65_535, 65_536, 65_537, (1 << 28) - 1, 1 << 28)
LHS_DIMS = tuple(range(11))
LHS_SEEDS = (20261003, 0xFEDCBA9876543210)                         # the project's default seed; one with the top bit set
WINDOW = 513


def lhs_windows(n_total):
    """The member windows (m0, n) both test files look at: the whole of a small design and every n of {1, 255, 256, 257, 513}
    it has; for a large one [0, 513), [n_total - 513, n_total) and ragged middle windows that start at odd m0."""
    if n_total <= WINDOW:
        out = [(0, n_total)]
        out += [(n_total - n, n) for n in (1, 255, 256, 257) if n < n_total]
        return out
    mid = (n_total // 3) | 1
    if n_total == (1 << 28) - 1:
        # the domain has ONE point outside the design, x = n_total itself: only the member the network sends there walks on, and
        # only it can tell `x >= n_total` from `x > n_total`.  The middle windows go where dimension 0 has it.
        mid = min(max(lhs_preimage(LHS_SEEDS[0], n_total, 0, n_total) - 100, WINDOW), n_total - 2 * WINDOW - 1000) | 1
    return [(0, WINDOW), (n_total - WINDOW, WINDOW), (mid, 257), (mid + 2, 255), (mid + 514, 256), (n_total // 2 | 1, 1)]


# ---- the Latin hypercube in integers ---------------------------------------------------------------------------------------
def half_bits_of(n_total):
    """Half the width of the Feistel domain: the smallest h >= 1 with 4^h >= n_total (an even number of bits, at least two)."""
    h = 1
    while 4 ** h < n_total:
        h += 1
    return h


def _mix_int(z):
    """splitmix64's finaliser."""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def _dim_key_int(seed, dim):
    return _mix_int((seed + GOLD * (dim + 1)) & MASK)


def lhs_ints(seed, n_total, dim, m, half_bits=None, accept=None):
    """(stratum, jbits, u) of member m in dimension dim.  half_bits and accept (the rule that ends the cycle-walk, x < n_total)
    can be replaced only to show that a wrong one gives other numbers."""
    assert 1 <= n_total <= LHS_MAX_TOTAL and 0 <= m < n_total
    h = half_bits_of(n_total) if half_bits is None else half_bits
    mask = (1 << h) - 1
    key = _dim_key_int(seed, dim)
    x = m
    while True:
        left, right = x >> h, x & mask
        for rnd in range(ROUNDS):
            f = _mix_int(right ^ ((key + ROUND_ODD * (rnd + 1)) & MASK)) & mask
            left, right = right, left ^ f
        x = (left << h) | right
        if (x < n_total) if accept is None else accept(x, n_total):
            break
    jbits = _mix_int(m ^ ((key * JIT_MUL + JIT_ADD) & MASK)) >> 40
    u = float(Fraction(x * 2 ** 25 + 2 * jbits + 1, 2 ** 25 * n_total))      # Fraction.__float__ rounds correctly
    return x, jbits, u


def lhs_preimage(seed, n_total, dim, x):
    """The point of the Feistel domain that ONE pass of the network sends to x (the rounds undone in reverse order)."""
    h = half_bits_of(n_total)
    mask = (1 << h) - 1
    key = _dim_key_int(seed, dim)
    left, right = x >> h, x & mask
    for rnd in reversed(range(ROUNDS)):
        f = _mix_int(left ^ ((key + ROUND_ODD * (rnd + 1)) & MASK)) & mask
        left, right = right ^ f, left
    return (left << h) | right


# ---- the same in wrapping uint64 NumPy -------------------------------------------------------------------------------------
def _u(v):
    return np.uint64(v & MASK)


def _mix(z):
    z = (z ^ (z >> _u(30))) * _u(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> _u(27))) * _u(0x94D049BB133111EB)
    return z ^ (z >> _u(31))


def lhs_strata_ref(seed, n_total, dim, members, stop_at_n_total=False):
    """(stratum, jbits) as uint64 arrays for the members given.  stop_at_n_total: the WRONG walk that also accepts x == n_total,
    kept only to show which members tell it from the right one."""
    h = half_bits_of(n_total)
    mask, sh = _u((1 << h) - 1), _u(h)
    m = np.asarray(members, dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = _mix(np.array([(seed + GOLD * (dim + 1)) & MASK], dtype=np.uint64))[0]
        rkeys = [key + _u(ROUND_ODD * (rnd + 1)) for rnd in range(ROUNDS)]
        out = np.empty(m.shape, dtype=np.uint64)
        idx, x = np.arange(m.size), m.copy()
        while idx.size:
            left, right = x >> sh, x & mask
            for rk in rkeys:
                left, right = right, left ^ (_mix(right ^ rk) & mask)
            x = (left << sh) | right
            done = (x <= _u(n_total)) if stop_at_n_total else (x < _u(n_total))
            out[idx[done]] = x[done]
            idx, x = idx[~done], x[~done]
        jbits = _mix(m ^ (key * _u(JIT_MUL) + _u(JIT_ADD))) >> _u(40)
    return out, jbits


def lhs_rows_ref(seed, n_total, dims, lo, hi):
    """[len(dims), hi - lo] fp64.  The numerator stratum 2^25 + 2 jbits + 1 < 2^53 and the denominator 2^25 n_total <= 2^53 are
    exact in fp64, so the one division gives the correctly rounded quotient."""
    assert 1 <= n_total <= LHS_MAX_TOTAL and 0 <= lo <= hi <= n_total
    members = np.arange(lo, hi, dtype=np.uint64)
    out = np.empty((len(dims), hi - lo), dtype=np.float64)
    den = float(n_total << 25)
    for k, d in enumerate(dims):
        stratum, jbits = lhs_strata_ref(seed, n_total, int(d), members)
        num = (stratum << _u(25)) + (jbits << _u(1)) + _u(1)
        out[k] = num.astype(np.float64) / den
    return out


# ---- exp(-t) at 50 digits ----------------------------------------------------------------------------------------------------
Decay = collections.namedtuple("Decay", "exact rounded")          # exact: Fractions (floats at the special times); rounded: fp64


def _special_decay(t):
    """exp(-t) where no arbitrary-precision value is needed: -(+inf) -> +0, -(-inf) -> +inf, NaN -> NaN, -+0 -> 1."""
    if math.isnan(t):
        return math.nan
    if math.isinf(t):
        return 0.0 if t > 0 else math.inf
    assert t == 0.0
    return 1.0


def _round_fraction(q):
    """The nearest fp64 of a positive rational, subnormals included (int / int is correctly rounded); +inf past the range."""
    try:
        return float(q)
    except OverflowError:
        return math.inf


def hfc_decay_mp(time):
    """exp(-t) of every fp64 t: Decay(exact, rounded).  The arguments convert exactly; 50 digits leave a relative error below
    1e-49 — 1e-33 ulp — in `exact`."""
    import mpmath
    exact = []
    with mpmath.workdps(50):
        for t in np.asarray(time, dtype=np.float64).ravel().tolist():
            if t == 0.0 or math.isinf(t) or math.isnan(t):
                exact.append(_special_decay(t))
                continue
            sign, man, exp, _ = mpmath.exp(-mpmath.mpf(t))._mpf_
            assert sign == 0 and man > 0
            exact.append(Fraction(int(man)) * Fraction(2) ** int(exp))
    rounded = np.array([v if isinstance(v, float) else _round_fraction(v) for v in exact], dtype=np.float64)
    return Decay(exact, rounded)


DBL_MAX = float(np.finfo(np.float64).max)


def ulp_err(got, want_mp):
    """|got - exact| / spacing(|exact rounded to fp64|) per element — in units of 2^-1074 where the rounded value is subnormal or
    zero, of the last place of DBL_MAX where it overflowed.  A special value must be met exactly (0 ulp) or counts as inf; so
    does a result of the wrong class (inf or NaN for a finite value)."""
    got = np.asarray(got, dtype=np.float64).ravel()
    assert got.size == len(want_mp.exact)
    err = np.empty(got.size)
    for i, (g, q, r) in enumerate(zip(got.tolist(), want_mp.exact, want_mp.rounded.tolist())):
        if isinstance(q, float):                                   # a special time
            err[i] = 0.0 if (math.isnan(q) and math.isnan(g)) or (g == q and math.copysign(1.0, g) == math.copysign(1.0, q)) else math.inf
        elif math.isnan(g):
            err[i] = math.inf
        elif math.isinf(r):                                        # overflow: +inf is the answer
            err[i] = 0.0 if g == math.inf else (math.inf if math.isinf(g) else float((q - Fraction(g)) / Fraction(math.ulp(DBL_MAX))))
        elif math.isinf(g):
            err[i] = math.inf
        else:
            err[i] = float(abs(Fraction(g) - q) / Fraction(float(np.spacing(abs(r)))))
    return err


def is_subnormal_or_zero(x):
    return np.abs(np.asarray(x, dtype=np.float64)) < np.finfo(np.float64).tiny


# ---- the time sets of the exponential tests ------------------------------------------------------------------------------
# The bound on exp(-t) against the 50-digit value, in ulp_err units, for normal and subnormal results alike and with no absolute
# floor.  The rule: 1 ulp if the worst error measured on the device is within it (glibc and NumPy meet 1 ulp on the CPU:
# tests/test_first_kernels_cpu.py), 2 ulp — what the project holds its own primitives to — if it lies between 1 and 2; a worst
# error above 2 is a finding, not a wider bound.  Measured on an MI355X (ROCm 7.2.0, 2026-10-21): 0.7199 ulp at worst, per time
# set and result class in test_the_exponential_against_fifty_digits of tests/test_first_kernels_gpu.py — so 1 ulp.
EXP_ULP_BOUND = 1.0
CONFIG1_STEPS = 750


@functools.lru_cache(maxsize=None)
def hfc_time_sets():
    """{name: read-only fp64 times}: uniform draws on [-2, 30]; the integers 0..749 of BASELINE config 1 (through the subnormal
    range to zero); 513 points log-spaced in magnitude from 1e-6 to 745 over both signs, with 0 between them."""
    rng = np.random.default_rng(20261021)
    mag = np.geomspace(1e-6, 745.0, 256)
    sets = {"uniform": rng.uniform(-2.0, 30.0, 64), "integers": np.arange(CONFIG1_STEPS, dtype=np.float64),
            "logspaced": np.concatenate([-mag[::-1], [0.0], mag])}
    assert sets["logspaced"].size == 513 and sets["logspaced"][-1] == 745.0 and sets["logspaced"][0] == -745.0
    for v in sets.values():
        v.setflags(write=False)
    return sets


@functools.lru_cache(maxsize=None)
def hfc_time_refs():
    """{name: Decay} of hfc_time_sets(), computed once per process (1 327 values)."""
    return {name: hfc_decay_mp(t) for name, t in hfc_time_sets().items()}


def worst_errors(got, want_mp):
    """(worst ulp_err among normal rounded values, worst among subnormal or zero ones, index of the overall worst); a class
    without elements gives 0."""
    err = ulp_err(got, want_mp)
    sub = is_subnormal_or_zero(want_mp.rounded)
    worst_n = float(err[~sub].max()) if (~sub).any() else 0.0
    worst_s = float(err[sub].max()) if sub.any() else 0.0
    return worst_n, worst_s, int(err.argmax())
