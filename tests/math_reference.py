"""Exact references and structured inputs for the hand-written math of the step (fiveeq_math.hpp), CPU only.

The device routines are probed through fiveeq_math_probe_f64 / _f32 (ops 0..4: expm1 on x <= 0, exp, log, sqrt, reciprocal).
This module supplies

  reference(op, x, prec)   the exact value as an unevaluated sum hi + lo of two doubles (Exact): hi is the value rounded to
                           double, lo what that rounding left.  fp32 results: fp64 NumPy (its ~1 ulp(double) is 2e-9 of an
                           fp32 ulp), lo = 0.  fp64 results: mpmath at 160 bits (48 digits), or 80-bit long double
                           (method="longdouble", <= 1 ulp(long double) = 2^-11 ulp(double)) for the dense sets.
  ulp_err(got, want, prec) |got - want| / spacing(|want rounded to prec|), the convention of tests/test_engine_gpu.py.
  edge_grid / edge_points  the structured inputs by family, every centre with its +-32 neighbours in the tested precision.
  dense_points             2^20 (fp64) / 2^24 (fp32) draws from the distributions tests/test_engine_gpu.py uses.

Nothing here touches torch or the GPU: tests/test_math_reference_cpu.py shows that the references agree with each other and
that NumPy's own routines pass every bound the device is held to on every generated point.
"""
import collections
import functools
import math

import numpy as np

OPS = ("expm1", "exp", "log", "sqrt", "rcp")                   # probe op = index
PROBE_OP = {name: i for i, name in enumerate(OPS)}
PRECS = ("f64", "f32")
DTYPE = {"f64": np.float64, "f32": np.float32}
MANT = {"f64": 52, "f32": 23}
NEIGHBOURS = 32
LN2 = math.log(2.0)

# what the project documents (fiveeq_math.hpp, DESIGN section 3, tests/test_engine_gpu.py): max ulp per routine
CAPS = {("f64", "expm1"): 2.0, ("f64", "exp"): 2.0, ("f64", "log"): 2.0, ("f64", "sqrt"): 1.0, ("f64", "rcp"): 1.0,
        ("f32", "expm1"): 2.0, ("f32", "exp"): 2.0, ("f32", "log"): 2.5, ("f32", "sqrt"): 1.0, ("f32", "rcp"): 1.0}
F32_LOG_MEAN_CAP = 0.7
# expm1 keeps full RELATIVE accuracy for small arguments: |x| below, relative bound
EXPM1_SMALL = {"f64": (1e-5, 3e-16), "f32": (1e-4, 2e-7)}
# the clamps of the device routines: expm1 below, exp on both sides
EXPM1_CLAMP = {"f64": -800.0, "f32": -87.0}
EXP_CLAMP = {"f64": 700.0, "f32": 80.0}
EXPM1_KMAX = {"f64": 1154, "f32": 126}                         # every k of x = k ln2 + r the clamp admits
# positive normals the other three are specified for
POS_RANGE = {"f64": (1e-280, 1e280), "f32": (float(np.nextafter(np.float32(1e-30), np.float32(1))) if np.float32(1e-30) < 1e-30
                                             else float(np.float32(1e-30)),
                                             float(np.nextafter(np.float32(1e30), np.float32(1))) if np.float32(1e30) > 1e30
                                             else float(np.float32(1e30)))}
HAVE_LONGDOUBLE = np.finfo(np.longdouble).nmant >= 63
DENSE_N = {"f64": 1 << 20 if HAVE_LONGDOUBLE else 1 << 16, "f32": 1 << 24}
DENSE_SEED = 20240519

Exact = collections.namedtuple("Exact", "hi lo")


# ---- the exact value --------------------------------------------------------------------------------------------------
_MP_PREC = 160


def _mp_funcs():
    from mpmath import libmp
    P, R = _MP_PREC, "n"
    one = libmp.fone

    def expm1(m):
        if m[2] + m[3] < -70:                                  # |x| < 2^-70: x + x^2/2 + x^3/6, relative error < 2^-200
            x2 = libmp.mpf_mul(m, m, P, R)
            t = libmp.mpf_add(libmp.mpf_shift(x2, -1), libmp.mpf_div(libmp.mpf_mul(x2, m, P, R), libmp.from_int(6), P, R), P, R)
            return libmp.mpf_add(m, t, P + 80, R)
        return libmp.mpf_sub(libmp.mpf_exp(m, P + 80, R), one, P, R)      # 80 guard bits for the cancellation

    return {"expm1": expm1, "exp": lambda m: libmp.mpf_exp(m, P, R), "log": lambda m: libmp.mpf_log(m, P, R),
            "sqrt": lambda m: libmp.mpf_sqrt(m, P, R), "rcp": lambda m: libmp.mpf_div(one, m, P, R)}


def _reference_mpmath(op, x):
    from mpmath import libmp
    f = _mp_funcs()[op]
    hi, lo = np.empty(x.size), np.zeros(x.size)
    for i, v in enumerate(x.tolist()):
        if v == 0.0 or math.isinf(v) or math.isnan(v):
            hi[i] = _special(op, v)
            continue
        r = f(libmp.from_float(v))
        h = libmp.to_float(r, rnd="n")
        hi[i] = h
        if h != 0.0 and not math.isinf(h):
            lo[i] = libmp.to_float(libmp.mpf_sub(r, libmp.from_float(h), 64, "n"), rnd="n")
    return Exact(hi, lo)


def _special(op, v):
    """The value at 0, +-inf and NaN arguments, where an arbitrary-precision type has no say."""
    with np.errstate(all="ignore"):
        f = {"expm1": np.expm1, "exp": np.exp, "log": np.log, "sqrt": np.sqrt, "rcp": np.reciprocal}[op]
        return float(f(np.float64(v)))


def _numpy_op(op, x):
    """NumPy's routine in the precision of x (float32, float64 or long double)."""
    with np.errstate(all="ignore"):
        if op == "rcp":
            return 1 / x
        return {"expm1": np.expm1, "exp": np.exp, "log": np.log, "sqrt": np.sqrt}[op](x)


def reference(op, x, prec, method=None):
    """Exact(hi, lo) of op at the arguments x (an array of the tested precision's dtype).  method: None picks fp64 NumPy for
    prec = 'f32' and mpmath for 'f64'; 'longdouble' and 'mpmath' force one (fp64 arguments)."""
    x = np.ascontiguousarray(x, dtype=DTYPE[prec]).ravel()
    if method is None:
        method = "numpy64" if prec == "f32" else "mpmath"
    if method == "numpy64":
        assert prec == "f32"
        return Exact(_numpy_op(op, x.astype(np.float64)), np.zeros(x.size))
    if method == "mpmath":
        return _reference_mpmath(op, x.astype(np.float64))
    assert method == "longdouble" and HAVE_LONGDOUBLE
    v = _numpy_op(op, x.astype(np.longdouble))
    hi = v.astype(np.float64)
    with np.errstate(invalid="ignore"):
        lo = np.where(np.isfinite(hi), (v - hi.astype(np.longdouble)).astype(np.float64), 0.0)
    return Exact(hi, lo)


def rounded(want, prec):
    """The exact value rounded to the tested precision (ties cannot occur to the accuracy that matters here)."""
    return want.hi if prec == "f64" else want.hi.astype(np.float32)


def ulp_err(got, want, prec):
    """|got - want| / spacing(|want rounded to prec|); want an Exact or a plain array."""
    if not isinstance(want, Exact):
        want = Exact(np.asarray(want, dtype=np.float64), 0.0)
    got = np.asarray(got).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        same = got == want.hi                                  # also inf == inf
        d = np.where(same, -np.asarray(want.lo), (got - want.hi) - want.lo)   # got - hi is exact for neighbours of hi
        w = np.abs(rounded(want, prec))
        u = np.abs(d) / np.spacing(w).astype(np.float64)
        return np.where(same & (np.asarray(want.lo) == 0), 0.0, u)     # equal infinities, 0 against 0


# ---- the argument ranges ---------------------------------------------------------------------------------------------
def in_range(op, x, prec):
    """Mask of the arguments the routine is specified for (header comments, tests/test_engine_gpu.py)."""
    x = np.asarray(x)
    if op == "expm1":
        return x <= 0
    if op == "exp":
        return np.abs(x) <= EXP_CLAMP[prec]
    lo, hi = POS_RANGE[prec]
    return (x >= lo) & (x <= hi)


def with_neighbours(centres, prec):
    """[n, 65]: every centre between its 32 predecessors and 32 successors in the tested precision, ascending."""
    dt = DTYPE[prec]
    c = np.asarray(centres, dtype=dt).ravel()
    out = np.empty((c.size, 2 * NEIGHBOURS + 1), dtype=dt)
    out[:, NEIGHBOURS] = c
    for i in range(1, NEIGHBOURS + 1):
        out[:, NEIGHBOURS + i] = np.nextafter(out[:, NEIGHBOURS + i - 1], dt(np.inf))
        out[:, NEIGHBOURS - i] = np.nextafter(out[:, NEIGHBOURS - i + 1], dt(-np.inf))
    return out


def _pow2(exps):
    return np.ldexp(1.0, np.asarray(exps, dtype=np.int64))


def _exps_in(lo, hi):
    """Every e with lo <= 2^e <= hi."""
    return np.arange(math.ceil(math.log2(lo) - 1e-12), math.floor(math.log2(hi) + 1e-12) + 1)


def edge_centres(op, prec):
    """{family: centres (fp64 values, exactly representable in the tested precision after the cast)}."""
    dt, mant = DTYPE[prec], MANT[prec]
    fi = np.finfo(dt)
    cast = lambda v: np.asarray(v, dtype=np.float64).astype(dt).astype(np.float64)   # noqa: E731
    if op == "expm1":
        k = np.arange(EXPM1_KMAX[prec] + 1)
        e = np.arange(-1074, 1024) if prec == "f64" else np.arange(fi.minexp, fi.maxexp)
        tiny = [-0.0, -float(fi.tiny), -np.inf]
        if prec == "f64":
            tiny += [-5e-324, -float(np.nextafter(fi.tiny, 0))]                      # smallest and largest subnormal
        fam = {"tie": -(k + 0.5) * LN2, "kln2": -k * LN2, "pow2": -_pow2(e), "clamp": [EXPM1_CLAMP[prec]],
               "minus_one": [-(mant + 2) * LN2], "tiny": tiny}
    elif op == "exp":
        c = EXP_CLAMP[prec]
        kt = np.arange(int(c / LN2 - 0.5) + 1)
        kk = np.arange(int(c / LN2) + 1)
        e = np.arange(-1074 if prec == "f64" else fi.minexp, int(math.log2(c)) + 1)
        sym = lambda v: np.concatenate([v, -v])                                      # noqa: E731
        fam = {"tie": sym((kt + 0.5) * LN2), "kln2": sym(kk * LN2), "clamp": [c, -c], "zero": [0.0], "pow2": sym(_pow2(e)),
               "outside": [1e4, -1e4]}
    elif op == "log":
        lo, hi = POS_RANGE[prec]
        e = _exps_in(lo, hi)
        j = np.arange(1, mant + 1)
        fam = {"split": math.sqrt(0.5) * _pow2(e), "pow2": _pow2(e), "sqrt2": math.sqrt(2.0) * _pow2(e[:-1]),
               "near1": np.concatenate([1 + _pow2(-j), 1 - _pow2(-j)]), "one": [1.0]}
    elif op in ("sqrt", "rcp"):
        lo, hi = POS_RANGE[prec]
        e = _exps_in(lo, hi)
        # 2^e (1 + 2^-j): every e with one j, cycling so that every j meets even and odd e (mant + 1 is odd); and every j
        # at the ends of the range and around e = 0
        j = 1 + (e - e[0]) % (mant + 1)
        j = np.where(j > mant, 1, j)
        few = np.array([e[0], e[0] + 1, -2, -1, 0, 1, e[-1] - 2, e[-1] - 1])
        jj = np.arange(1, mant + 1)
        pj = np.concatenate([_pow2(e) * (1 + _pow2(-j)), (_pow2(few)[:, None] * (1 + _pow2(-jj))[None, :]).ravel()])
        below = np.nextafter(_pow2(e + 1).astype(dt), dt(0)).astype(np.float64)
        fam = {"pow2": _pow2(e), "pow2_1pj": pj, "below_pow2": below, "ends": [lo, hi]}
    else:
        raise ValueError(op)
    return {name: cast(v) for name, v in fam.items()}


@functools.lru_cache(maxsize=None)
def edge_grid(op, prec):
    """{family: [n_centres, 65] array of the tested dtype}: rows ascend through consecutive floats.  Read-only."""
    out = {}
    for name, c in edge_centres(op, prec).items():
        g = with_neighbours(c, prec)
        g.setflags(write=False)
        out[name] = g
    return out


@functools.lru_cache(maxsize=None)
def edge_points(op, prec):
    """{family: 1-D array}: the grid's points inside the routine's argument range; the family 'outside' (exp only) holds
    the points beyond the clamp instead, +-1e4 and the clamps' outer neighbours.  Read-only."""
    out = {}
    beyond = []
    for name, g in edge_grid(op, prec).items():
        flat = g.ravel()
        ok = in_range(op, flat, prec)
        if name == "outside":
            beyond.append(flat)
            continue
        if name == "clamp" and op == "exp":
            beyond.append(flat[~ok])
        out[name] = flat[ok]
    if beyond:
        out["outside"] = np.concatenate(beyond)
    for v in out.values():
        v.setflags(write=False)
    return out


def dense_points(op, prec, rng=None, n=None):
    """n (default 2^20 for fp64, 2^24 for fp32) arguments: half log-uniform over the routine's range, half uniform over its
    central interval — the distributions of tests/test_engine_gpu.py.  rng defaults to a generator with a fixed seed."""
    rng = np.random.default_rng(DENSE_SEED + PROBE_OP[op] + (100 if prec == "f32" else 0)) if rng is None else rng
    n = DENSE_N[prec] if n is None else n
    h = n // 2
    dt = DTYPE[prec]
    if op == "expm1":
        lo_dec, hi_dec = (-300.0, 2.9) if prec == "f64" else (-30.0, 1.9)
        x = -np.concatenate([10.0 ** rng.uniform(lo_dec, hi_dec, h), rng.uniform(0, 2, n - h)])
    elif op == "exp":
        c = EXP_CLAMP[prec]
        x = np.concatenate([rng.uniform(-c, c, h), rng.uniform(-12, 12, n - h)])
    elif op in ("log", "sqrt", "rcp"):
        d = 280.0 if prec == "f64" else 30.0
        x = np.concatenate([10.0 ** rng.uniform(-d, d, h), rng.uniform(0.5, 4.0, n - h)])
    else:
        raise ValueError(op)
    x = x.astype(dt)
    if op in ("log", "sqrt", "rcp"):
        x = np.clip(x, dt(POS_RANGE[prec][0]), dt(POS_RANGE[prec][1]))
    elif op == "exp":
        x = np.clip(x, dt(-EXP_CLAMP[prec]), dt(EXP_CLAMP[prec]))
    return x
