"""The hand-written math of the step (fiveeq_math.hpp) at its structural edges, through fiveeq_math_probe_f64 / _f32.

Every kernel form computes through the same five routines, so "every form gives the same bits" cannot see a wrong one.
Here each is held to its documented bound against an exact reference (tests/math_reference.py: mpmath on the structured
sets, 80-bit long double on the dense ones, fp64 for fp32 results) at the places where such routines go wrong: the
Cody-Waite ties and multiples of ln 2, the mantissa split of the log, arguments next to 1 and to powers of two, the clamps,
the ends of the ranges the seed-plus-Newton reciprocal and square root are specified for.  The packed fp32 twins must
return the scalar routines' bits for every float of each routine's range, in either component of the pair.
tests/test_math_reference_cpu.py shows that NumPy's routines pass the same bounds on the same points."""
import ctypes
import functools

import numpy as np
import pytest

import math_reference as mr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ALL = [(p, op) for p in mr.PRECS for op in mr.OPS]
TDTYPE = {"f64": torch.float64, "f32": torch.float32}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from fiveeqscm_amd import _capi
    return _capi.load()


def probe_t(lib, prec, op, xd, yd=None, n=None):
    """Run probe op (an index, packed twins included) on a device tensor; returns the output tensor."""
    from fiveeqscm_amd import _capi
    yd = torch.empty_like(xd) if yd is None else yd
    fn = lib.fiveeq_math_probe_f64 if prec == "f64" else lib.fiveeq_math_probe_f32
    _capi.check(lib, fn(op, xd.numel() if n is None else n, ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(yd.data_ptr()), None))
    torch.cuda.synchronize()
    return yd


def probe(lib, prec, op, x):
    xd = torch.from_numpy(np.array(x, dtype=mr.DTYPE[prec])).cuda()          # a copy: the shared sets are read-only
    return probe_t(lib, prec, mr.PROBE_OP[op] if isinstance(op, str) else op, xd).cpu().numpy()


def _hex(v):
    return float(v).hex()


@functools.lru_cache(maxsize=None)
def _edge_reference(op, prec):
    """(x, family index, family names, Exact) of the structured set: computed once and shared."""
    ep = mr.edge_points(op, prec)
    names = [n for n in ep if n != "outside"]
    x = np.concatenate([ep[n] for n in names])
    fam = np.concatenate([np.full(ep[n].size, i) for i, n in enumerate(names)])
    return x, fam, names, mr.reference(op, x, prec)


def measure(lib, op, prec):
    """Worst ulp error per family: {family: (ulp, x, got, want)}, 'dense' included; plus the arrays for further checks."""
    xe, fam, names, we = _edge_reference(op, prec)
    xd = mr.dense_points(op, prec)
    wd = mr.reference(op, xd, prec, "longdouble" if prec == "f64" and mr.HAVE_LONGDOUBLE else None)
    x = np.concatenate([xe, xd])
    fam = np.concatenate([fam, np.full(xd.size, len(names))])
    names = names + ["dense"]
    want = mr.Exact(np.concatenate([we.hi, wd.hi]), np.concatenate([we.lo, wd.lo]))
    got = probe(lib, prec, op, x)
    u = mr.ulp_err(got, want, prec)
    if op == "log":
        u = np.where(x == 1, 0.0, u)                            # ln(1): asserted to be exactly 0 instead
    u = np.where(np.isnan(u), np.inf, u)
    worst = {}
    for i, name in enumerate(names):
        sel = np.flatnonzero(fam == i)
        k = sel[np.argmax(u[sel])]
        worst[name] = (float(u[k]), x[k], got[k], want.hi[k])
    return worst, (x, fam, names, got, want, u)


@pytest.mark.parametrize("prec,op", ALL)
def test_accuracy_on_the_structured_and_dense_sets(lib, prec, op):
    """(a) ulp error over edge_points U dense_points under the documented cap: fp64 expm1 / exp / log <= 2, sqrt / rcp <= 1;
    fp32 expm1 / exp <= 2, log <= 2.5 with mean < 0.7, sqrt / rcp <= 1.  No point is excluded except log(1), which must be
    exactly 0.  expm1 keeps RELATIVE accuracy for small arguments, the log next to 1; exp, sqrt and rcp return finite normal
    numbers for every argument of their range (what fe_rcp relies on for alpha)."""
    worst, (x, fam, names, got, want, u) = measure(lib, op, prec)
    for name, (uu, xx, gg, ww) in worst.items():
        print(f"{prec} {op:5s} {name:10s} worst {uu:.4f} ulp at x = {_hex(xx)}: got {_hex(gg)}, exact {_hex(ww)}")
    cap = mr.CAPS[prec, op]
    name, (uu, xx, gg, ww) = max(worst.items(), key=lambda kv: kv[1][0])
    assert uu <= cap, f"{prec} {op}: {uu:.4f} ulp > {cap} at x = {_hex(xx)} (family {name}): got {_hex(gg)}, exact {_hex(ww)}"
    if op == "log":
        assert np.all(got[x == 1] == 0) and np.any(x == 1), "ln(1) must be exactly 0: C = C0 gives no forcing"
        near = fam == names.index("near1")
        k = np.flatnonzero(near)[np.argmax(u[near])]
        assert u[k] <= cap, f"{prec} log next to 1: {u[k]:.4f} ulp of the RESULT at x = {_hex(x[k])}: got {_hex(got[k])}, exact {_hex(want.hi[k])}"
        if prec == "f32":
            assert u[x != 1].mean() < mr.F32_LOG_MEAN_CAP, u[x != 1].mean()
    if op == "expm1":
        lim, rel = mr.EXPM1_SMALL[prec]
        small = np.flatnonzero((np.abs(x) < lim) & (x != 0))
        err = np.abs((got[small].astype(np.float64) - want.hi[small]) - want.lo[small]) / np.abs(want.hi[small])
        k = small[np.argmax(err)]
        print(f"{prec} expm1 small arguments: worst relative error {err.max():.3e} at x = {_hex(x[k])}")
        assert err.max() < rel, f"{prec} expm1 for |x| < {lim}: relative error {err.max():.3e} >= {rel} at x = {_hex(x[k])}: got {_hex(got[k])}, exact {_hex(want.hi[k])} (family {names[fam[k]]})"
        assert np.all(got[x == 0] == 0)
    if op in ("exp", "sqrt", "rcp"):
        bad = np.flatnonzero(~(np.isfinite(got) & (np.abs(got) >= np.finfo(mr.DTYPE[prec]).tiny)))
        assert bad.size == 0, f"{prec} {op}: not a finite normal result at x = {_hex(x[bad[0]])}: got {_hex(got[bad[0]])} (family {names[fam[bad[0]]]})"


def _bits(a):
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


@pytest.mark.parametrize("prec", mr.PRECS)
def test_special_values_on_bits(lib, prec):
    """(b) expm1: -inf and every argument below the clamp give -1, +-0 a zero.  exp beyond the clamp equals exp at the clamp.
    rcp and sqrt are exact on powers of two (and sqrt on their squares).  NaN: the fmax / fmin clamps of expm1 and exp return
    their other operand (fiveeq_math.hpp), so expm1(NaN) = expm1(clamp) = -1 and exp(NaN) = exp(-clamp); log, sqrt and rcp
    propagate the NaN."""
    dt = mr.DTYPE[prec]
    fi = np.finfo(dt)
    clamp = dt(mr.EXPM1_CLAMP[prec])
    g = mr.edge_grid("expm1", prec)
    below = np.concatenate([g["clamp"].ravel(), g["pow2"].ravel(), g["tie"].ravel(), np.array([-1e3, -1e30, -fi.max, -np.inf], dtype=dt)])
    below = below[below <= clamp]                               # the clamp itself: exp(-800) = 0, exp(-87) < 2^-25
    got = probe(lib, prec, "expm1", below)
    assert below.size > 1000 and np.array_equal(_bits(got), _bits(np.full(below.size, -1, dtype=dt))), _hex(below[np.argmax(got != -1)])
    z = probe(lib, prec, "expm1", np.array([0.0, -0.0], dtype=dt))
    assert np.all(z == 0)
    # exp beyond the clamp
    c = dt(mr.EXP_CLAMP[prec])
    out = mr.edge_points("exp", prec)["outside"]
    out = np.concatenate([out, np.array([fi.max, -fi.max, np.inf, -np.inf], dtype=dt)])
    at = probe(lib, prec, "exp", np.array([c, -c], dtype=dt))
    got = probe(lib, prec, "exp", out)
    assert np.array_equal(_bits(got), _bits(np.where(out > 0, at[0], at[1])))
    assert np.isfinite(at).all() and np.all(at >= fi.tiny)
    # exact powers of two
    lo, hi = mr.POS_RANGE[prec]
    e = mr._exps_in(lo, hi)
    p2 = np.ldexp(1.0, e).astype(dt)
    assert np.array_equal(_bits(probe(lib, prec, "rcp", p2)), _bits(np.ldexp(1.0, -e).astype(dt)))
    even = e[e % 2 == 0]
    assert np.array_equal(_bits(probe(lib, prec, "sqrt", np.ldexp(1.0, even).astype(dt))), _bits(np.ldexp(1.0, even // 2).astype(dt)))
    m = np.arange(e[0] // 2 + 1, e[-1] // 2)
    sq = (np.ldexp(1.0, m) * np.ldexp(1.0, m)).astype(dt)       # squares of powers of two
    assert np.array_equal(_bits(probe(lib, prec, "sqrt", sq)), _bits(np.ldexp(1.0, m).astype(dt)))
    assert np.array_equal(_bits(probe(lib, prec, "rcp", sq)), _bits(np.ldexp(1.0, -2 * m).astype(dt)))
    # NaN, as the source reads
    nan = np.array([np.nan, -np.nan], dtype=dt)
    assert np.array_equal(_bits(probe(lib, prec, "expm1", nan)), _bits(np.array([-1, -1], dtype=dt)))
    assert np.array_equal(_bits(probe(lib, prec, "exp", nan)), _bits(np.array([at[1], at[1]], dtype=dt)))
    for op in ("log", "sqrt", "rcp"):
        assert np.isnan(probe(lib, prec, op, nan)).all(), op


def _patterns(first, last, device):
    """Float32 tensors of the bit patterns first..last (inclusive, as unsigned), in chunks of 2^26, each of even length."""
    chunk = 1 << 26
    for a in range(first, last + 1, chunk):
        b = min(a + chunk, last + 1)
        p = torch.arange(a, b, dtype=torch.int64, device=device)
        if p.numel() & 1:
            p = torch.cat([p, p[:1]])
        p = torch.where(p >= 1 << 31, p - (1 << 32), p).to(torch.int32)
        yield p.view(torch.float32)


def _f32_bits(v):
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


# every float of each routine's argument range: (first, last) unsigned bit patterns
def _pattern_ranges(op):
    if op == "expm1":
        return [(0x80000000, 0xFF800000), (0, 0)]              # -0 .. -inf, and +0
    if op == "exp":
        c = _f32_bits(mr.EXP_CLAMP["f32"])
        return [(0, c), (0x80000000, 0x80000000 | c)]
    lo, hi = mr.POS_RANGE["f32"]
    return [(_f32_bits(lo), _f32_bits(hi))]


MID = {"expm1": -0.75, "exp": 0.75, "log": 1.75, "sqrt": 1.75, "rcp": 1.75}


def _packed_equals_scalar(lib, op_index, x, mid):
    """The three pairings on one even-length device tensor; all comparisons on the device, on bits."""
    bits = lambda t: t.view(torch.int32)                        # noqa: E731
    ys = probe_t(lib, "f32", op_index, x)
    assert torch.equal(bits(probe_t(lib, "f32", op_index + 8, x)), bits(ys)), "pairs of consecutive floats"
    xs = x.view(-1, 2).flip(1).contiguous().view(-1)
    yp = probe_t(lib, "f32", op_index + 8, xs)
    assert torch.equal(bits(yp.view(-1, 2).flip(1).contiguous().view(-1)), bits(ys)), "the same pairs swapped"
    del xs, yp
    pair = torch.empty(x.numel(), 2, dtype=torch.float32, device=x.device)
    ymid = probe_t(lib, "f32", op_index, torch.full((2,), mid, dtype=torch.float32, device=x.device))[0]
    for slot in (0, 1):
        pair[:, slot] = x
        pair[:, 1 - slot] = mid
        yp = probe_t(lib, "f32", op_index + 8, pair.view(-1)).view(-1, 2)
        assert torch.equal(bits(yp[:, slot].contiguous()), bits(ys)), f"each value in slot {slot} beside a constant"
        assert bool((bits(yp[:, 1 - slot].contiguous()) == bits(ymid)).all()), f"the constant in slot {1 - slot}"


@pytest.mark.parametrize("op", mr.OPS)
def test_packed_equals_scalar_for_every_float_of_the_range(lib, op):
    """(c) every fp32 bit pattern of the routine's argument range through op and op + 8: pairs of consecutive floats, the
    same pairs swapped, and each value beside one fixed constant in either slot — an error confined to one component of
    float2v (the shape of the hipcc 7.2 miscompile of fe_exp2_from_magic) cannot hide.  No host reference is involved."""
    dev = torch.device("cuda:0")
    n = 0
    for first, last in _pattern_ranges(op):
        for x in _patterns(first, last, dev):
            n += x.numel()
            _packed_equals_scalar(lib, mr.PROBE_OP[op], x, MID[op])
    print(f"{op}: {n} arguments")
    assert n >= (last - first + 1)


@pytest.mark.parametrize("prec", mr.PRECS)
def test_launch_shapes_sentinels_and_an_unaligned_input(lib, prec):
    """(d) scalar ops at n = 1, 63, 64, 65, 255, 257 and packed ops at n = 2, 126, 128, 130: the results are those of one
    large aligned launch, nothing is written beyond n, and the input starts one element off a 16-byte boundary."""
    dt, td = mr.DTYPE[prec], TDTYPE[prec]
    size = dt().itemsize
    sentinel = -12345.0
    shapes = [(0, n) for n in (1, 63, 64, 65, 255, 257)] + ([(8, n) for n in (2, 126, 128, 130)] if prec == "f32" else [])
    for op in mr.OPS:
        x = mr.dense_points(op, prec, np.random.default_rng(3), 512)
        whole = probe(lib, prec, op, x)
        for plus, n in shapes:
            buf = torch.zeros(n + 8, dtype=td, device="cuda:0")
            xd = buf[1:1 + n]
            assert buf.data_ptr() % 16 == 0 and xd.data_ptr() % 16 == size
            xd.copy_(torch.from_numpy(x[:n]))
            yd = torch.full((n + 64,), sentinel, dtype=td, device="cuda:0")
            probe_t(lib, prec, mr.PROBE_OP[op] + plus, xd, yd, n)
            y = yd.cpu().numpy()
            assert np.array_equal(_bits(y[:n]), _bits(whole[:n])), (op, plus, n)
            assert np.all(y[n:] == sentinel), (op, plus, n)


@pytest.mark.parametrize("prec,op", ALL)
def test_monotone_across_every_reduction_boundary(lib, prec, op):
    """(e) over the +-32 neighbours of every tie, multiple, split, power of two and clamp: the device result never steps
    against the function's direction (non-decreasing; non-increasing for rcp).  A wrong k on one side of a tie shows here as a
    jump of the wrong sign even where both sides pass (a)."""
    sign = -1.0 if op == "rcp" else 1.0
    for name, g in mr.edge_grid(op, prec).items():
        got = probe(lib, prec, op, g.ravel()).reshape(g.shape).astype(np.float64)
        ok = mr.in_range(op, g, prec)
        if op == "exp":
            ok = np.ones_like(ok)                               # clamped outside: constant, still monotone
        both = ok[:, 1:] & ok[:, :-1]
        step = sign * np.diff(got, axis=1)
        back = both & ~(step >= 0)
        if back.any():
            r, c = np.argwhere(back)[0]
            ulps = abs(step[r, c]) / np.spacing(abs(got[r, c]))
            raise AssertionError(f"{prec} {op} (family {name}): f({_hex(g[r, c])}) = {_hex(got[r, c])} but f({_hex(g[r, c + 1])}) = "
                                 f"{_hex(got[r, c + 1])}: {ulps:.1f} ulp against the function's direction; {int(back.sum())} such steps")
