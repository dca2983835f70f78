"""Host references for tests/test_utility_kernels_gpu.py: exact IEEE fp64 restatements that need no GPU and no libm — the busy
kernel's FMA chain, the ulp error of a device exp(-t) against a 50-digit value, and the stratum floor(u * n_total) of a
Latin-hypercube coordinate from its bits."""
import math
from fractions import Fraction

import numpy as np

BUSY_MUL, BUSY_ADD = 0.999999, 1.0e-9          # busy_kernel's constants (fiveeq_diag.hpp): the same decimal literals, the same doubles


def fma(a, b, c):
    """round(a * b + c), ONE rounding: math.fma where the interpreter has it, else the exact rational rounded once (CPython's
    int / int is correctly rounded, and that is what Fraction.__float__ does)."""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def busy_chain(iters):
    """What busy_kernel's lane 0 leaves: x <- fma(x, 0.999999, 1e-9), `iters` times from 0.0."""
    x = 0.0
    for _ in range(iters):
        x = fma(x, BUSY_MUL, BUSY_ADD)
    return x


def bits(x):
    """The int64 bit pattern(s) of fp64 value(s)."""
    return np.asarray(x, dtype=np.float64).view(np.int64)


def exp_neg_reference(time):
    """exp(-t) of every fp64 t to 50 digits, as Fractions: mpmath where it imports, else decimal.  The inputs convert exactly."""
    try:
        import mpmath
    except ImportError:
        import decimal
        with decimal.localcontext() as ctx:
            ctx.prec = 50
            return [Fraction((-decimal.Decimal(float(t))).exp()) for t in time]
    with mpmath.workprec(200):                 # 60 digits carried, 50 kept
        return [Fraction(mpmath.nstr(mpmath.exp(-mpmath.mpf(float(t))), 50)) for t in time]


def ulp_errors(got, ref):
    """|got - ref| in units of the last place of ref rounded to fp64, per element; ref from exp_neg_reference."""
    return np.array([float(abs(Fraction(float(g)) - r) / Fraction(math.ulp(float(r)))) for g, r in zip(got, ref)])


def strata(u, n_total):
    """floor(u * n_total) of fp64 u in (0, 1), n_total <= 2^28, in exact integer arithmetic from the bits of u — no rounded
    product, no epsilon.  u = M 2^-s with M < 2^53 and s >= 53.  Split M = Mh 2^26 + Ml: Mh n_total and Ml n_total stay below
    2^55, and floor(M n_total / 2^s) = floor((Mh n_total + floor(Ml n_total / 2^26)) / 2^(s - 26))."""
    u = np.asarray(u, dtype=np.float64)
    assert np.all((u > 0.0) & (u < 1.0)) and 1 <= n_total <= 1 << 28
    frac, exp = np.frexp(u)                                    # u = frac 2^exp, 0.5 <= frac < 1, exp <= 0
    M = np.ldexp(frac, 53).astype(np.int64)                    # exact: frac has 53 significant bits
    shift = 53 - exp.astype(np.int64) - 26
    top = (M >> 26) * n_total + (((M & ((1 << 26) - 1)) * n_total) >> 26)
    return np.where(shift > 62, 0, top >> np.minimum(shift, 62))


def strata_slow(u, n_total):
    """The same with Python's unbounded integers (the check of `strata`)."""
    out = []
    for v in np.asarray(u, dtype=np.float64).tolist():
        num, den = v.as_integer_ratio()
        out.append(num * n_total // den)
    return np.array(out, dtype=np.int64)
