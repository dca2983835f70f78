"""The three fold orders of fiveeq_stats.hpp restated in NumPy fp64 and held to tests/stats_reference.py — the place where the
bound gamma(20) is shown to hold for the arithmetic alone, without a GPU:

    ladder          wave_reduce_to_lane63 as a prefix scan: row_shr 1 / 2 / 4 / 8 inside each row of 16 lanes, row_bcast 15
                    into rows 1 and 3, row_bcast 31 into rows 2 and 3; a lane without a DPP source takes the neutral element;
                    the packed form adds the lane's two members first, stops before row_bcast 31 and reads lanes 31 and 63;
    flush           wave_stats_flush: lane (j, p) folds members 8 p .. 8 p + 7 of step j serially (the square through an FMA),
                    the eight partials meet over xor 8 / 16 / 32;
    packed flush    lane (j, p) folds members 16 p .. 16 p + 15, x then y of each packed lane, xor 8 / 16; p = 0 and p = 4
                    hold the wave's two records.

Inputs: the pattern of stats_reference.pattern() over 19 decaying steps (sizes with full, 63-member, 2- and 1-member records),
and rows whose sum cancels to nearly nothing.  Each route prints its worst error-to-bound ratio (expected well below 1; the
assertion is <= 1, the derived bound).  Two deliberately wrong emulations — a member moved across the lane-31/32 boundary of
the packed ladder, a flush row written at j + 1 — must FAIL the comparison: the inputs do their job.
"""
from fractions import Fraction

import numpy as np
import pytest

import stats_reference as sr

N_STEPS = 19
SIZES = (1, 63, 64, 65, 127, 128, 129, 193, 321, 330)


def _rows(N):
    """The pattern as T rows: step t holds pattern x 0.9958^(t + 1) (a slow box relaxing) plus a small common drift."""
    p = sr.pattern(N)
    return np.stack([p * 0.9958 ** (t + 1) + 1e-3 * t for t in range(N_STEPS)])


def _cancelling_rows(N, seed):
    """Pairs (a, -a (1 + 2^-40)): each record's sum is ~1e-12 of its abs1."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.5, 5.0, size=(N_STEPS, (N + 1) // 2))
    out = np.empty((N_STEPS, 2 * a.shape[1]))
    out[:, 0::2], out[:, 1::2] = a, -a * (1.0 + 2.0 ** -40)
    return out[:, :N]


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))      # one rounding


# ---- the routes ------------------------------------------------------------------------------------------------------------------
def _ladder(v, op, neutral, to_lane63=True):
    v = np.array(v, dtype=np.float64)
    lane = np.arange(64)
    for k in (1, 2, 4, 8):                                     # row_shr:k — lanes k .. 15 of a row read lane - k
        src = np.full(64, neutral)
        ok = lane % 16 >= k
        src[ok] = v[lane[ok] - k]
        v = op(v, src)
    src = np.full(64, neutral)                                 # row_bcast:15, row mask 0xa
    src[16:32], src[48:64] = v[15], v[47]
    v = op(v, src)
    if to_lane63:
        src = np.full(64, neutral)                             # row_bcast:31, row mask 0xc
        src[32:64] = v[31]
        v = op(v, src)
    return v


def _pad(x, n, fill):
    out = np.full(n, fill, dtype=np.float64)
    out[:len(x)] = x
    return out


def route_ladder(T, shift=0):
    """Per-step kernel, one member per lane: [R, n, 4]."""
    n_steps, N = T.shape
    R = (N + 63) // 64
    out = np.zeros((R, n_steps, 4))
    for r in range(R):
        for t in range(n_steps):
            v = T[t, 64 * r:64 * (r + 1)]
            out[r, t] = (_ladder(_pad(v, 64, 0.0), np.add, 0.0)[63], _ladder(_pad(v * v, 64, 0.0), np.add, 0.0)[63],
                         _ladder(_pad(v, 64, np.inf), np.fmin, np.inf)[63], _ladder(_pad(v, 64, -np.inf), np.fmax, -np.inf)[63])
    return out


def route_packed_ladder(T, wrong=False):
    """Per-step kernel, packed fp32 lanes: lane l of a wave holds members 2 l, 2 l + 1 of its 128; lanes 31 / 63 write.
    wrong=True: the member pair of lane 32 is folded with lanes 0 .. 31 (the split one lane too far)."""
    n_steps, N = T.shape
    R = (N + 63) // 64
    out = np.zeros((R, n_steps, 4))
    for w in range((N + 127) // 128):
        for t in range(n_steps):
            v = T[t, 128 * w:128 * (w + 1)]
            x, y = v[0::2], v[1::2]
            cols = []
            for vals, op, neutral in ((lambda a: a, np.add, 0.0), (lambda a: a * a, np.add, 0.0),
                                      (lambda a: a, np.fmin, np.inf), (lambda a: a, np.fmax, -np.inf)):
                lanes = op(_pad(vals(x), 64, neutral), _pad(vals(y), 64, neutral))
                if wrong:                                      # lane 32's pair joins the first record
                    lanes[31], lanes[32] = op(lanes[31], lanes[32]), neutral
                cols.append(_ladder(lanes, op, neutral, to_lane63=False))
            out[2 * w, t] = [c[31] for c in cols]
            if 2 * w + 1 < R:
                out[2 * w + 1, t] = [c[63] for c in cols]
    return out


def _flush_partials(vals):
    """Serial fold of a lane's values from (0, 0, +inf, -inf): (s1, s2, mn, mx)."""
    s1, s2, mn, mx = 0.0, 0.0, np.inf, -np.inf
    for v in vals:
        s1 = s1 + v
        s2 = _fma(v, v, s2)
        mn, mx = min(mn, v), max(mx, v)
    return [s1, s2, mn, mx]


def _xor_combine(parts, steps):
    """parts [P][4]; lane p takes lane p ^ s for each s: every lane ends with the total of its group."""
    parts = [list(p) for p in parts]
    for s in steps:
        other = [parts[p ^ s] for p in range(len(parts))]
        parts = [[a[0] + b[0], a[1] + b[1], min(a[2], b[2]), max(a[3], b[3])] for a, b in zip(parts, other)]
    return parts


def route_flush(T, wrong=False):
    """Time-fused and small-ensemble kernels, one member per lane: batches of 8 steps from the first, the last one ragged.
    wrong=True: row j of a batch is written at step slot j + 1."""
    n_steps, N = T.shape
    R = (N + 63) // 64
    out = np.zeros((R, n_steps, 4))
    for r in range(R):
        for t in range(n_steps):
            v = T[t, 64 * r:64 * (r + 1)]
            parts = [_flush_partials(v[8 * p:8 * p + 8]) for p in range(8)]
            slot = min(t + 1, n_steps - 1) if wrong else t
            out[r, slot] = _xor_combine(parts, (1, 2, 4))[0]       # xor 8 / 16 / 32 of the lane index = 1 / 2 / 4 of p
    return out


def route_packed_flush(T):
    n_steps, N = T.shape
    R = (N + 63) // 64
    out = np.zeros((R, n_steps, 4))
    for w in range((N + 127) // 128):
        for t in range(n_steps):
            v = T[t, 128 * w:128 * (w + 1)]
            parts = _xor_combine([_flush_partials(v[16 * p:16 * p + 16]) for p in range(8)], (1, 2))
            out[2 * w, t] = parts[0]
            if 2 * w + 1 < R:
                out[2 * w + 1, t] = parts[4]
    return out


ROUTES = {"ladder": route_ladder, "packed ladder": route_packed_ladder, "flush": route_flush, "packed flush": route_packed_flush}


# ---- tests -----------------------------------------------------------------------------------------------------------------------
def test_the_inputs_have_the_properties_the_record_tests_rely_on():
    for N in SIZES:
        margin = sr.check_inputs(_rows(N))
        assert margin > 1e10
    # a sub-range that starts on a record boundary sees the same records
    full = _rows(330)
    sr.check_inputs(full[:, 64:194], first=64)
    sr.check_inputs(full[:, 128:321], first=128)


def test_reference_on_hand_computed_records():
    T = np.array([[1.0, -2.0, np.nan, 4.0], [2.0 ** 60, 1.0, -2.0 ** 60, 1.0]])
    ref = sr.records(T)
    assert ref["count"].tolist() == [[4, 4]] and ref["nan"].tolist() == [[1, 0]]
    assert ref["min"][0, 0] == -2.0 and ref["max"][0, 0] == 4.0 and np.isnan(ref["s1"][0, 0])
    assert ref["s1"][0, 1] == 2.0 and ref["abs1"][0, 1] == 2.0 ** 61 + 2.0 and ref["s2"][0, 1] == 2.0 ** 121 + 2.0
    only_nan = sr.records(np.full((1, 65), np.nan))
    assert only_nan["min"].tolist() == [[np.inf], [np.inf]] and only_nan["max"].tolist() == [[-np.inf], [-np.inf]]
    assert only_nan["count"].tolist() == [[64], [1]] and only_nan["nan"].tolist() == [[64], [1]]
    wide = sr.records(np.array([[0.1, 0.2]], dtype=np.float32))          # fp32 rows widen exactly
    assert wide["s1"][0, 0] == float(np.float32(0.1)) + float(np.float32(0.2))


@pytest.mark.parametrize("route", list(ROUTES))
def test_every_fold_order_is_within_gamma_20_of_the_reference(route):
    worst = [0.0, 0.0]
    for N in SIZES:
        for rows in (_rows(N), _cancelling_rows(N, seed=N)):
            e1, e2 = sr.compare(ROUTES[route](rows), sr.records(rows))
            assert e1 <= 1.0 and e2 <= 1.0, (route, N, e1, e2)
            worst = [max(worst[0], e1), max(worst[1], e2)]
    print(f"{route}: worst |s1 - ref| / (gamma(20) abs1) = {worst[0]:.4f}, worst |s2 - ref| / (gamma(20) s2) = {worst[1]:.4f}")


def test_fp32_rows_widen_exactly_and_stay_within_the_bound():
    rows = _rows(321).astype(np.float32)
    ref = sr.records(rows)
    for route in ("packed ladder", "packed flush"):
        e1, e2 = sr.compare(ROUTES[route](rows.astype(np.float64)), ref)
        assert e1 <= 1.0 and e2 <= 1.0, (route, e1, e2)


def test_a_member_across_the_lane_31_32_boundary_fails_the_comparison():
    rows = _rows(321)
    with pytest.raises(AssertionError):
        e1, e2 = sr.compare(route_packed_ladder(rows, wrong=True), sr.records(rows))
        assert e1 <= 1.0 and e2 <= 1.0, (e1, e2)
    # ... by the sums alone, too: the moved pair holds neither extremum in the first wave's records, yet s1 and s2 miss
    got, ref = route_packed_ladder(rows, wrong=True), sr.records(rows)
    e1 = np.abs(got[..., 0] - ref["s1"]) / (sr.gamma(20) * ref["abs1"])
    e2 = np.abs(got[..., 1] - ref["s2"]) / (sr.gamma(20) * ref["s2"])
    assert e1[:2].min() > 1e9 and e2[:2].min() > 1e9, (e1[:2].min(), e2[:2].min())


def test_a_flush_row_written_at_the_next_step_fails_the_comparison():
    rows = _rows(129)
    with pytest.raises(AssertionError):
        e1, e2 = sr.compare(route_flush(rows, wrong=True), sr.records(rows))
        assert e1 <= 1.0 and e2 <= 1.0, (e1, e2)
