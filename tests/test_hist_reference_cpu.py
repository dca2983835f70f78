"""The exact reference of THE BIN RULE (oracle/summary_passes.bin_rule, include/fiveeq.h), proved on the CPU: its fp32 FMA
(product exact in fp64, TwoSum, round to odd, one rounding to fp32) against fractions.Fraction arithmetic on random
operands, operands that overflow, results in the subnormal range and on 128 triples, found by search, on which the earlier
restatement (fp64 sum, rounded twice) gives another float; make_rule's clamped constants; the order of NaN, clamp and
truncation.  And the TEETH of tests/test_hist_exact_gpu.py: every deliberately wrong rule of tests/hist_exact_rows.py moves
members on the rows those tests hand the device."""
from fractions import Fraction

import numpy as np
import pytest

import hist_exact_rows as hx
from oracle.summary_passes import bin_rule, fma_f32, rule_constants_f32

F32, F64 = np.float32, np.float64


def _same_floats(got, want):
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    return np.array_equal(got, want)                     # (+0 == -0: the rule clamps both to bin 0)


def _exact(xs, as_, cs):
    return np.array([hx.fma_exact(x, a, c) for x, a, c in zip(xs, as_, cs)], dtype=F64).astype(F32)


def _random_f32(rng, n, e_lo, e_hi):
    m = rng.integers(2 ** 23, 2 ** 24, size=n).astype(F64)
    return (np.ldexp(m, rng.integers(e_lo, e_hi, size=n) - 23) * rng.choice([-1.0, 1.0], size=n)).astype(F32)


def test_round_to_f32_is_numpy_rounding_of_exact_doubles():
    """The rational rounding itself: on doubles (exact rationals) it must be NumPy's correctly rounded float64 -> float32 cast,
    ties, subnormals, the overflow threshold included."""
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.normal(size=2000) * 10.0 ** rng.integers(-50, 40, size=2000),
                        [2.0 ** -149, 2.0 ** -150, 1.5 * 2.0 ** -150, 2.0 ** -151, 2.0 ** -126, 2.0 ** -126 - 2.0 ** -150,
                         (2 - 2.0 ** -24) * 2.0 ** 127, np.nextafter((2 - 2.0 ** -24) * 2.0 ** 127, 0), 3.5e38, 1 + 2.0 ** -24,
                         1 + 3 * 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -52]])
    with np.errstate(over="ignore"):
        assert _same_floats([hx.round_to_f32(Fraction(float(x))) for x in v], v.astype(F32))
        assert _same_floats([hx.round_to_f32(Fraction(float(-x))) for x in v], (-v).astype(F32))


def test_fma_on_random_operands():
    rng = np.random.default_rng(1)
    n = 4000
    for ex, ea, ec in (((-8, 8), (-8, 8), (-8, 8)), ((-8, 8), (-8, 8), (-40, -8)), ((-30, 3), (0, 30), (-3, 13)),
                       ((-60, 60), (-60, 60), (-120, 120))):
        x, a, c = _random_f32(rng, n, *ex), _random_f32(rng, n, *ea), _random_f32(rng, n, *ec)
        assert _same_floats(fma_f32(x, a, c), _exact(x, a, c))
    # sums that cancel to a few bits, and exactly to zero
    x, a = _random_f32(rng, n, -4, 4), _random_f32(rng, n, -4, 4)
    c = (-(x.astype(F64) * a.astype(F64))).astype(F32)
    assert _same_floats(fma_f32(x, a, c), _exact(x, a, c))
    assert fma_f32(F32(3.0), F32(0.5), F32(-1.5)) == 0.0


def test_fma_that_overflows_and_operands_that_are_not_finite():
    rng = np.random.default_rng(2)
    n = 2000
    x, a, c = _random_f32(rng, n, 60, 127), _random_f32(rng, n, 60, 127), _random_f32(rng, n, 100, 127)
    got = fma_f32(x, a, c)
    assert _same_floats(got, _exact(x, a, c)) and np.isinf(got).sum() > n // 2
    # right at the threshold: max + half an ulp rounds to inf, just below it to max
    mx = np.finfo(F32).max
    assert fma_f32(mx, F32(1.0), F32(2.0 ** 103)) == np.inf and hx.fma_exact(mx, 1.0, 2.0 ** 103) == np.inf
    assert fma_f32(mx, F32(1.0), np.nextafter(F32(2.0 ** 103), F32(0))) == mx
    with np.errstate(invalid="ignore"):
        got = fma_f32(np.array([np.inf, -np.inf, np.inf, np.nan, 1.0], dtype=F32), np.array([2.0, 2.0, 0.0, 1.0, 1.0], dtype=F32),
                      np.array([-3e38, 3e38, 1.0, 1.0, np.inf], dtype=F32))
    assert got[0] == np.inf and got[1] == -np.inf and np.isnan(got[2]) and np.isnan(got[3]) and got[4] == np.inf


def test_fma_with_results_in_the_subnormal_range():
    rng = np.random.default_rng(3)
    n = 4000
    x, a, c = _random_f32(rng, n, -80, -60), _random_f32(rng, n, -75, -60), _random_f32(rng, n, -149, -130)
    got = fma_f32(x, a, c)
    assert _same_floats(got, _exact(x, a, c))
    assert (np.abs(got) < np.finfo(F32).tiny).sum() > n // 2
    tiny = np.nextafter(F32(0), F32(1))
    assert fma_f32(tiny, F32(0.5), F32(0)) == 0.0 and fma_f32(tiny, F32(0.75), F32(0)) == tiny      # tie to even; above the tie
    assert fma_f32(tiny, F32(0.5), tiny) == tiny * 2                                                  # 1.5 tiny: tie to even


def test_fma_where_the_double_rounded_restatement_is_wrong():
    """128 triples found by search (hx.double_rounding_triples): the exact result is pred(k), the fp64 restatement gives k.
    This is the only place the old and the new reference differ — and each of them moves a member by one bin."""
    tr = hx.double_rounding_triples()
    assert len(tr) >= 100
    x, a, c, k = (np.array(v) for v in zip(*tr))
    exact = _exact(x, a, c)
    assert _same_floats(fma_f32(x, a, c), exact)
    assert (hx.fma_double_rounded(x, a, c) != exact).all()
    assert np.array_equal(exact.astype(F64), np.nextafter(k.astype(F32), F32(0)).astype(F64))
    for xi, s, o, ki in tr:
        rg = hx.triple_range(s, o, 4096)
        assert rg is not None
        xs = np.array([xi], dtype=F32)
        assert bin_rule(xs, *rg, 4096, F32)[0] == ki - 1 and hx.wrong_double_rounded(xs, *rg, 4096, F32)[0] == ki


def test_rule_constants_and_the_order_of_nan_clamp_and_truncation():
    big = F32(3.0e38)
    assert rule_constants_f32(0.0, 4096 / 1e-40) == (big, F32(0.0))                   # hi - lo = 1e-40: scale clamped
    assert rule_constants_f32(1.0, 4096 / 1e-40) == (big, -big) and rule_constants_f32(-1.0, 4096 / 1e-40) == (big, big)
    assert rule_constants_f32(-0.3, 4096 / 7.4) == (F32(4096 / 7.4), F32(0.3 * (4096 / 7.4)))
    for dt in (F32, F64):
        x = np.array([np.nan, -np.inf, np.inf, -1.0, 0.0, -0.0, 0.999, 1.0, 2.5, 3.0, 1e30], dtype=dt)
        assert bin_rule(x, 0.0, 3.0, 3, dt).tolist() == [-1, 0, 2, 0, 0, 0, 0, 1, 2, 2, 2]
        # hi <= lo (the ranged entry points): inv_w = 0, every non-NaN member — inf * 0 = NaN pos included — in bin 0
        for lo, hi in ((2.0, 2.0), (2.0, -1.0)):
            assert bin_rule(x, lo, hi, 7, dt).tolist() == [-1] + [0] * 10
        # a range too narrow for fp32 constants still bins every member (fp64 rows: plain arithmetic)
        assert bin_rule(np.array([-1.0, 0.0, 1e-41, 1.0, np.inf], dtype=dt), 0.0, 1e-40, 4096, dt).tolist()[::4] == [0, 4095]
    # the fp64 branch is the formula, nothing else
    rng = np.random.default_rng(4)
    x = rng.uniform(-1.0, 8.0, size=10_000)
    want = np.trunc(np.clip((x - (-0.3)) * (4096 / (7.1 - (-0.3))), 0, 4095)).astype(np.int64)
    assert np.array_equal(bin_rule(x, -0.3, 7.1, 4096, F64), want)


def test_the_rule_against_rational_arithmetic_on_edge_rows():
    """bin_rule for fp32 rows, end to end, against Fractions on a sample of every section-2 row (finite members)."""
    rng = np.random.default_rng(5)
    for name, (x, lo, hi, nb) in hx.section2_rows_f32().items():
        if name.startswith("triple"):
            continue
        xs = x[np.isfinite(x)]
        xs = xs[rng.integers(0, len(xs), size=60)]
        _, s, o = hx._consts(lo, hi, nb)
        pos = _exact(xs, np.full(len(xs), s), np.full(len(xs), o)).astype(F64)
        want = np.trunc(np.clip(pos, 0, nb - 1)).astype(np.int64)
        assert np.array_equal(bin_rule(xs, lo, hi, nb, F32), want), name


@pytest.mark.parametrize("wrong", list(hx.WRONG_RULES))
def test_every_wrong_rule_moves_members_on_the_rows_the_device_gets(wrong):
    """The teeth of tests/test_hist_exact_gpu.py, without a GPU: each wrong rule changes the histogram of at least one
    section-2 row (the figures are in that module's docstring)."""
    rows = hx.section2_rows_f32()
    mv = {name: hx.moved(x, lo, hi, nb, F32, hx.WRONG_RULES[wrong]) for name, (x, lo, hi, nb) in rows.items()}
    print(wrong, "rows:", sum(v > 0 for v in mv.values()), "of", len(mv), "members:", sum(mv.values()))
    assert sum(v > 0 for v in mv.values()) >= 1
    if wrong == "double-rounded FMA":                     # only the searched triples tell it from the exact FMA
        assert all(v == 0 for k, v in mv.items() if not k.startswith("triple"))
        assert sum(v for k, v in mv.items() if k.startswith("triple")) >= 100
