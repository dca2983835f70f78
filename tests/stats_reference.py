"""The exact reference of the per-wave statistics records, and the inputs that make a misplaced member visible.

TEST INFRASTRUCTURE.  Shares no code with fiveeqscm_amd: plain Python on the stored T rows.

THE RECORDS.  With collect_stats=True the stepping kernels write, for every 64 consecutive members (record r = m // 64) and
every step t, the four fp64 words (sum, sum of squares, min, max) of T.  records() computes for the same members, from the
stored rows [n_steps, N] (fp32 rows widen exactly):

    count   the members of the record;
    s1      math.fsum(v): the exact sum, rounded once;
    s2      the exact sum of the exact squares (fractions.Fraction), rounded once;
    abs1    math.fsum(|v|);
    min/max exact, NaN members left out (+inf / -inf when none remain);
    nan     the number of NaN members (s1, s2, abs1 are then NaN, as a kernel's sums are).

THE BOUND is derived from the code of fiveeq_stats.hpp, not measured.  u = 2^-53, gamma(k) = k u / (1 - k u).  A sum of
fp64 terms in which every term passes through at most k rounded additions differs from the exact sum by at most
gamma(k) sum |terms| (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: any order, k the longest chain).
The longest chain of rounded operations a term can pass through, by route:

    DPP ladder (wave_reduce_to_lane63)            6 adds: row_shr 1 / 2 / 4 / 8, row_bcast 15, row_bcast 31
    shortened ladder (packed fp32, lanes 31 / 63) 1 add (x + y of the lane) + 5 adds
    wave_stats_flush, one member per lane         8 serial adds from 0.0 (the first is exact: 7 rounded) + 3 xor-shuffle adds
    wave_stats_flush, packed                      16 serial adds from 0.0 (15 rounded) + 2 xor-shuffle adds
    the small-ensemble kernels                    wave_stats_flush on a tile that one or four waves filled: the same chain
    s2, per-step kernels                          one more: the product v * v is rounded before the ladder
    s2, every flush                               no more: the square enters through an FMA
    the reference itself                          one rounding of the exact result

The longest is the packed flush, 17, with the reference's own rounding 18; k = 20 is taken for EVERY route:

    |s1 - s1_ref| <= gamma(20) abs1          |s2 - s2_ref| <= gamma(20) s2_ref

The extrema are selections, not arithmetic: min and max must equal the reference bit for bit, and so must every count.  No form
the tests run has a longer chain than the packed flush, so k is 20 everywhere.

THE HOST FOLDS add the R records of a step (R - 1 further additions on any term, in whatever order the device sum takes) and
divide by N: mean within gamma(20 + R) fsum|v| / N.  var = s2 / N - mean^2 inherits err(s2) / N, 2 |mean| err(mean) +
err(mean)^2, and the roundings of its own four operations (a division, a product, a subtraction on numbers of size s2 / N, and
the reference's own rounding): gamma(5) s2_ref / N.

THE INPUTS (pattern()).  A value per member, meant for the slow thermal box of S0, so that T differs from member to member
from the first step: the sign alternates with the member index, the magnitudes of a record lie within a factor of 10 of each
other, and every record of four or more members has its maximum (+5.0, an even lane) and its minimum (-4.5, an odd lane) at
lanes known from the record's index alone (extreme_lanes()), never the first or the last lane, on either side of the
lane-31/32 split and in every row of 16 lanes as the record index grows.  Every member then carries at least 1 / 6400 of
abs1 — 7e10 times gamma(20) abs1 — so a member that is lost, counted twice or folded into a neighbouring record fails s1, s2 or
an extremum.  check_inputs() asserts these properties of the rows a test actually got back.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
K_ROUTE = 20


def gamma(k):
    return k * U / (1.0 - k * U)


def extreme_lanes(r, n_valid=64):
    """(lane of the minimum, lane of the maximum) of record r, or None for a record of fewer than four members."""
    if n_valid < 4:
        return None
    k = max(1, (n_valid - 3) // 2)                             # 30 for 63 and 64 members: odd lanes 1 .. 59, even lanes 2 .. 60
    lo, hi = 2 * ((11 * r + 3) % k) + 1, 2 * ((7 * r + 5) % k) + 2
    assert 0 < lo < n_valid - 1 and 0 < hi < n_valid - 1
    return lo, hi


def pattern(N, first=0):
    """The value of members first .. first + N - 1 (absolute member indices decide record and lane)."""
    out = np.empty(N, dtype=np.float64)
    total = first + N
    for i in range(N):
        m = first + i
        r, lane = divmod(m, 64)
        mag = 0.5 + 3.5 * ((lane * 29 + r * 13) % 64) / 63.0
        ext = extreme_lanes(r, min(64, total - 64 * r))
        if ext is not None and lane == ext[1]:
            mag = 5.0
        elif ext is not None and lane == ext[0]:
            mag = 4.5
        out[i] = mag if m % 2 == 0 else -mag
    return out


def _widen(T):
    T = np.asarray(T)
    assert T.ndim == 2 and T.dtype in (np.float32, np.float64), (T.shape, T.dtype)
    return T.astype(np.float64)                                # exact for fp32


def records(T):
    """dict of [R, n_steps] arrays (R = ceil(N / 64)) for rows T [n_steps, N]: count, nan (int64), s1, s2, abs1, min, max."""
    T = _widen(T)
    n_steps, N = T.shape
    R = (N + 63) // 64
    out = {k: np.zeros((R, n_steps), dtype=np.int64) for k in ("count", "nan")}
    out.update({k: np.zeros((R, n_steps), dtype=np.float64) for k in ("s1", "s2", "abs1", "min", "max")})
    for r in range(R):
        for t in range(n_steps):
            v = [float(x) for x in T[t, 64 * r:64 * (r + 1)]]
            kept = [x for x in v if x == x]
            out["count"][r, t] = len(v)
            out["nan"][r, t] = len(v) - len(kept)
            out["min"][r, t] = min(kept) if kept else math.inf
            out["max"][r, t] = max(kept) if kept else -math.inf
            if len(kept) == len(v) and all(math.isfinite(x) for x in v):
                out["s1"][r, t] = math.fsum(v)
                out["abs1"][r, t] = math.fsum(abs(x) for x in v)
                out["s2"][r, t] = float(sum(Fraction(x) * Fraction(x) for x in v))
            else:                                              # a non-finite member: the sums are what IEEE arithmetic makes of them
                with np.errstate(all="ignore"):
                    a = np.array(v)
                    out["s1"][r, t], out["abs1"][r, t], out["s2"][r, t] = a.sum(), np.abs(a).sum(), (a * a).sum()
    return out


def exact_moments(T):
    """Per step over ALL members, exactly: dict of [n_steps] arrays mean, var (population), s1, abs1, s2 (each rounded once),
    and min, max."""
    T = _widen(T)
    n_steps, N = T.shape
    out = {k: np.zeros(n_steps) for k in ("mean", "var", "s1", "abs1", "s2", "min", "max")}
    for t in range(n_steps):
        v = [Fraction(float(x)) for x in T[t]]
        s1, s2 = sum(v), sum(x * x for x in v)
        out["mean"][t] = float(s1 / N)
        out["var"][t] = float(s2 / N - (s1 / N) ** 2)
        out["abs1"][t] = math.fsum(abs(float(x)) for x in T[t])
        out["s1"][t], out["s2"][t] = float(s1), float(s2)
        out["min"][t], out["max"][t] = T[t].min(), T[t].max()
    return out


def check_inputs(T, first=0):
    """The properties of section THE INPUTS, asserted on rows [n_steps, N] of members first .. (first a multiple of 64).
    Returns the smallest |v| / (gamma(20) abs1) found: how far above the bound a single member stands."""
    T = _widen(T)
    assert first % 64 == 0 and np.isfinite(T).all()
    n_steps, N = T.shape
    m = first + np.arange(N)
    assert np.all((T > 0) == (m % 2 == 0)[None, :]) and np.all(T != 0), "the signs do not alternate"
    margin = math.inf
    for r0 in range(0, N, 64):
        v = T[:, r0:r0 + 64]
        mag = np.abs(v)
        assert np.all(mag.max(1) <= 100.0 * mag.min(1)), "magnitudes further than a factor of 100 apart"
        abs1 = np.array([math.fsum(row) for row in mag])
        assert np.all(mag.min(1) >= abs1 / 6400.0)
        margin = min(margin, float((mag.min(1) / (gamma(K_ROUTE) * abs1)).min()))
        ext = extreme_lanes((first + r0) // 64, v.shape[1])
        if ext is not None:
            assert np.all(v.argmin(1) == ext[0]) and np.all(v.argmax(1) == ext[1]), ((first + r0) // 64, ext)
            assert 0 < ext[0] < v.shape[1] - 1 and 0 < ext[1] < v.shape[1] - 1
    assert margin > 1e10
    return margin


def compare(stats, ref):
    """stats [R, n, 4] (sum, sum of squares, min, max) against records() of the same rows: asserts the extrema bit for bit
    and returns the worst (|s1 - ref| / (gamma(20) abs1), |s2 - ref| / (gamma(20) s2_ref)); the caller asserts <= 1."""
    stats = np.asarray(stats, dtype=np.float64)
    assert stats.shape == ref["s1"].shape + (4,), (stats.shape, ref["s1"].shape)
    for k, name in ((2, "min"), (3, "max")):
        same = stats[..., k].view(np.int64) == ref[name].view(np.int64)
        assert same.all(), (name, np.argwhere(~same)[:4].tolist(), stats[..., k][~same][:4], ref[name][~same][:4])
    assert np.isfinite(stats[..., :2]).all()
    e1 = np.abs(stats[..., 0] - ref["s1"]) / (gamma(K_ROUTE) * ref["abs1"])
    e2 = np.abs(stats[..., 1] - ref["s2"]) / (gamma(K_ROUTE) * ref["s2"])
    return float(e1.max()), float(e2.max())
