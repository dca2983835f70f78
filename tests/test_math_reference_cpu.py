"""The references and inputs of tests/test_math_edges_gpu.py are sound before any device runs (no GPU, no torch.cuda):
the two exact references agree, NumPy's own routines pass every bound the device is held to on every generated point
(so neither the inputs nor the ulp measure can fail a correct implementation), and every structural family holds what its
name says."""
import math

import numpy as np
import pytest

import math_reference as mr

F64_OPS = [("f64", op) for op in mr.OPS]
F32_OPS = [("f32", op) for op in mr.OPS]


def _edges(op, prec):
    ep = mr.edge_points(op, prec)
    return np.concatenate([v for name, v in ep.items() if name != "outside"])


@pytest.mark.parametrize("op", mr.OPS)
def test_mpmath_and_long_double_references_agree(op):
    """On a subsample of every structured set (every 29th point, plus the first and last of each family): the two references
    differ by < 2^-9 ulp(double).  mpmath works at 160 bits; glibc's long-double routines are good to ~1 ulp(long double) =
    2^-11 ulp(double)."""
    if not mr.HAVE_LONGDOUBLE:
        pytest.skip("long double has no 64-bit mantissa here")
    ep = mr.edge_points(op, "f64")
    x = np.concatenate([np.concatenate([v[:1], v[::29], v[-1:]]) for name, v in ep.items() if name != "outside"])
    a = mr.reference(op, x, "f64", "mpmath")
    b = mr.reference(op, x, "f64", "longdouble")
    assert np.array_equal(np.isfinite(a.hi), np.isfinite(b.hi))
    fin = np.isfinite(a.hi)
    d = np.abs((a.hi[fin] - b.hi[fin]) + (a.lo[fin] - b.lo[fin])) / np.spacing(np.abs(a.hi[fin]))
    assert x.size > 200 and d.max() < 2.0 ** -9, (op, d.max(), x[fin][d.argmax()].hex())


_LIBM_F32 = {"expm1": "expm1f", "exp": "expf", "log": "logf"}
LIBM_DENSE = 1 << 17


def _numpy_in_precision(op, x):
    return mr._numpy_op(op, x)


def _libm_f32(op, x):
    """The C library's float routine, one call per element (ctypes)."""
    import ctypes
    import ctypes.util
    f = getattr(ctypes.CDLL(ctypes.util.find_library("m")), _LIBM_F32[op])
    f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
    return np.array([f(v) for v in x.tolist()], dtype=np.float32)


@pytest.mark.parametrize("prec,op", F64_OPS + F32_OPS)
def test_numpy_routines_stay_inside_the_caps_on_every_generated_point(prec, op):
    """NumPy's expm1 / exp / log / sqrt / reciprocal in the tested precision, on the edge sets (fp64: against mpmath) and
    the dense sets (fp64: against long double), under the caps and the relative-accuracy properties of the device tests.

    fp32 expm1 / exp / log: NumPy's float32 loops are not the C library's routines but SIMD approximations with looser
    bounds of their own (measured on the edge sets with NumPy 2.2 on an AVX-512 host: expm1 2.08, exp 2.49, log 2.78 ulp),
    so they cannot show that a routine good to the caps passes.  For these three the C library's expm1f / expf / logf are
    called instead, element by element: on every edge point and on every 128th point of the dense set."""
    cap = mr.CAPS[prec, op]
    libm = prec == "f32" and op in _LIBM_F32
    for what, x, method in (("edge", _edges(op, prec), None), ("dense", mr.dense_points(op, prec), "longdouble" if prec == "f64" else None)):
        if method == "longdouble" and not mr.HAVE_LONGDOUBLE:
            method = None
        assert np.all(mr.in_range(op, x, prec)), (what, "a point outside the routine's range")
        if libm and what == "dense":
            x = x[::x.size // LIBM_DENSE]
        got = _libm_f32(op, x) if libm else _numpy_in_precision(op, x)
        assert got.dtype == mr.DTYPE[prec]
        want = mr.reference(op, x, prec, method)
        u = mr.ulp_err(got, want, prec)
        if op == "log":
            assert np.all(got[x == 1] == 0)
            u = u[x != 1]
        assert np.all(np.isfinite(u)) and u.max() <= cap, (prec, op, what, u.max(), x[np.argmax(u)].item().hex())
        if (prec, op) == ("f32", "log"):
            assert u.mean() < mr.F32_LOG_MEAN_CAP
        if op == "expm1":
            lim, rel = mr.EXPM1_SMALL[prec]
            small = (np.abs(x) < lim) & (x != 0)
            err = np.abs((got[small].astype(np.float64) - want.hi[small]) - np.asarray(want.lo)[small] if prec == "f64"
                         else got[small].astype(np.float64) - want.hi[small]) / np.abs(want.hi[small])
            assert small.sum() > 100 and err.max() < rel, (prec, what, err.max())


@pytest.mark.parametrize("prec", mr.PRECS)
def test_every_family_holds_what_its_name_says(prec):
    dt, mant = mr.DTYPE[prec], mr.MANT[prec]
    has = lambda arr, v: bool(np.any(arr == dt(v)))            # noqa: E731
    n65 = 2 * mr.NEIGHBOURS + 1
    for op in mr.OPS:
        ep = mr.edge_points(op, prec)
        for name, v in ep.items():
            assert v.size > 0 and v.dtype == dt, (op, name)
            assert np.all(mr.in_range(op, v, prec)) == (name != "outside"), (op, name)
        for name, g in mr.edge_grid(op, prec).items():
            inner = np.isfinite(g).all(axis=1)
            assert g.shape[1] == n65 and np.all(np.diff(g[inner].astype(np.float64), axis=1) >= 0), (op, name)
            assert np.all(g[~inner][:, 1:] >= g[~inner][:, :-1]), (op, name)
            steps = np.diff(g[inner].view(np.int64 if prec == "f64" else np.int32).astype(np.int64), axis=1)
            # consecutive floats: the bit patterns step by one (except across -0 / +0, where the sign bit flips)
            assert np.all((np.abs(steps) == 1) | (g[inner][:, 1:] == 0) | (g[inner][:, :-1] == 0)), (op, name)
        x = mr.dense_points(op, prec, n=1 << 12)
        assert x.dtype == dt and x.size == 1 << 12 and np.all(mr.in_range(op, x, prec)), op
    assert mr.DENSE_N[prec] == (1 << 24 if prec == "f32" else 1 << 20) or not mr.HAVE_LONGDOUBLE
    # expm1: every tie and multiple the clamp admits, the clamp and a step either side, the first argument that gives -1
    e = mr.edge_points("expm1", prec)
    kmax, clamp = mr.EXPM1_KMAX[prec], mr.EXPM1_CLAMP[prec]
    assert mr.edge_grid("expm1", prec)["tie"].shape[0] == kmax + 1 == mr.edge_grid("expm1", prec)["kln2"].shape[0]
    assert round((kmax + 0.5) * mr.LN2) in (800, 88) and -(kmax + 0.5) * mr.LN2 < clamp < -(kmax - 0.5) * mr.LN2
    for k in (0, 1, 7, kmax):
        assert has(e["tie"], -(k + 0.5) * mr.LN2) and has(e["kln2"], -k * mr.LN2)
    assert has(e["tie"], -0.34657359027997264)                  # the k = 0 / k = -1 switch
    for v in (clamp, np.nextafter(dt(clamp), dt(0)), np.nextafter(dt(clamp), dt(-np.inf))):
        assert has(e["clamp"], v)
    assert has(e["tiny"], -np.inf) and has(e["tiny"], np.finfo(dt).tiny) is False and has(e["tiny"], -np.finfo(dt).tiny)
    assert np.any((e["tiny"] == 0) & np.signbit(e["tiny"]))
    if prec == "f64":
        assert has(e["tiny"], -5e-324) and has(e["pow2"], -2.0 ** -1074)
    assert has(e["pow2"], -2.0 ** (np.finfo(dt).maxexp - 1)) and has(e["pow2"], -1.0) and has(e["pow2"], -np.finfo(dt).tiny)
    m1 = e["minus_one"]
    r = mr.rounded(mr.reference("expm1", m1, prec), prec)
    assert np.any(r == -1) and np.any(r != -1)                  # the family straddles the first argument that rounds to -1
    first = m1[r == -1].max()
    assert abs(float(first) + (mant + 2) * mr.LN2) < 40 * np.spacing(abs(dt(first))) and np.all(r[m1 > first] != -1)
    # exp: ties and multiples of both signs inside the clamp, the clamp, zero, +-1e4 outside
    e = mr.edge_points("exp", prec)
    c = mr.EXP_CLAMP[prec]
    kt = int(c / mr.LN2 - 0.5)
    assert (kt + 0.5) * mr.LN2 <= c < (kt + 1.5) * mr.LN2 and mr.edge_grid("exp", prec)["tie"].shape[0] == 2 * (kt + 1)
    for s in (1, -1):
        assert has(e["tie"], s * (kt + 0.5) * mr.LN2) and has(e["tie"], s * 0.5 * mr.LN2) and has(e["kln2"], s * int(c / mr.LN2) * mr.LN2)
        assert has(e["clamp"], s * c) and has(e["outside"], s * 1e4) and has(e["outside"], np.nextafter(dt(s * c), dt(s * np.inf)))
        assert has(e["pow2"], s * 2.0 ** int(math.log2(c))) and has(e["pow2"], s * np.finfo(dt).tiny)
    assert has(e["zero"], 0.0) and np.abs(e["outside"]).min() > c
    # log: the mantissa split, the powers of two and sqrt 2 at every exponent of the range; 1 +- 2^-j; exactly 1
    e = mr.edge_points("log", prec)
    lo, hi = mr.POS_RANGE[prec]
    n_e = len(mr._exps_in(lo, hi))
    assert n_e == (1861 if prec == "f64" else 199)
    assert mr.edge_grid("log", prec)["split"].shape[0] == n_e == mr.edge_grid("log", prec)["pow2"].shape[0]
    for ex in (mr._exps_in(lo, hi)[1], -1, 0, 1, mr._exps_in(lo, hi)[-2]):
        assert has(e["split"], math.sqrt(0.5) * 2.0 ** ex) and has(e["pow2"], 2.0 ** ex) and has(e["sqrt2"], math.sqrt(2) * 2.0 ** ex)
    assert has(e["split"], 0.7071067811865476) and has(e["split"], np.nextafter(dt(math.sqrt(0.5)), dt(0)))
    for j in (1, 2, mant - 1, mant):
        assert has(e["near1"], 1 + 2.0 ** -j) and has(e["near1"], 1 - 2.0 ** -j)
    assert has(e["one"], 1.0) and mr.edge_grid("log", prec)["near1"].shape[0] == 2 * mant
    # sqrt, rcp: every exponent (even and odd), every j, the largest float below the next power, both ends
    for op in ("sqrt", "rcp"):
        e = mr.edge_points(op, prec)
        assert mr.edge_grid(op, prec)["pow2"].shape[0] == n_e
        for ex in (mr._exps_in(lo, hi)[1], -3, -2, -1, 0, 1, 2, 3, mr._exps_in(lo, hi)[-2]):
            assert has(e["pow2"], 2.0 ** ex) and has(e["below_pow2"], np.nextafter(dt(2.0 ** (ex + 1)), dt(0)))
        centres = mr.edge_centres(op, prec)["pow2_1pj"]
        mm, ee = np.frexp(centres)
        jj = np.round(-np.log2(2 * mm - 1)).astype(int)
        for j in range(1, mant + 1):
            par = set((ee[jj == j] % 2).tolist())
            assert par == {0, 1}, (op, j)                       # every j meets even and odd exponents
        assert has(e["ends"], lo) and has(e["ends"], hi) and e["ends"].min() == dt(lo) and e["ends"].max() == dt(hi)


def test_ulp_measure_follows_the_suites_convention():
    """|got - want| / spacing(|want rounded|), exact in the low word, zero for equal infinities and for 0 against 0."""
    want = mr.Exact(np.array([1.0, 1.0, -1.0, 0.0, np.inf, 2.0]), np.array([2.0 ** -54, 0.0, 0.0, 0.0, 0.0, -2.0 ** -53]))
    got = np.array([1.0, 1.0 + 2.0 ** -52, -1.0 + 2.0 ** -53, 0.0, np.inf, 2.0 - 2.0 ** -52])
    assert mr.ulp_err(got, want, "f64").tolist() == [0.25, 1.0, 0.5, 0.0, 0.0, 0.25]
    got32 = np.array([1.0, 1.0 + 2.0 ** -23], dtype=np.float32)
    assert mr.ulp_err(got32, np.array([1.0 + 2.0 ** -25, 1.0]), "f32").tolist() == [0.25, 1.0]
    old = np.abs(got[:3] - want.hi[:3]) / np.spacing(np.abs(want.hi[:3]))      # tests/test_engine_gpu.py's _ulp_err
    assert np.allclose(mr.ulp_err(got[:3], want.hi[:3], "f64"), old)
