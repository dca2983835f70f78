"""The references of tests/first_kernels_reference.py hold on the CPU, without a GPU: the wrapping-uint64 Latin hypercube
against its statement in Python integers, against the NumPy twin (params.lhs_rows) and against the library's host twin
(fiveeq_lhs_rows_host_f64, the kernel's own C++ functions on the calling thread), bit for bit at every design size and window
tests/test_first_kernels_gpu.py uses; the bijection; that a wrong half_bits, a wrong end of the cycle-walk or an ignored dim0
gives other numbers AT THOSE windows; the C oracle's and NumPy's exp(-t) within the bound the device is held to; the refusals
of both entry points, made before any launch."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

import first_kernels_reference as ref
from fiveeqscm_amd import _capi
from fiveeqscm_amd import params as prm
from oracle import c_oracle

SENT = -777.25
SMALL = 70_000                                                   # designs up to here are looked at whole


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _host_twin(seed, n_total, m0, n, dim0, n_dim, pad):
    """fiveeq_lhs_rows_host_f64 into a sentinel-filled [n_dim + 2, n + pad] block with a guard row on either side."""
    lib = _capi.load()
    ld = n + pad
    buf = np.full((n_dim + 2, ld), SENT)
    rc = lib.fiveeq_lhs_rows_host_f64(seed, n_total, m0, n, dim0, n_dim, ld, ctypes.c_void_p(buf.ctypes.data + 8 * ld))
    assert rc == _capi.OK, (n_total, m0, n, (lib.fiveeq_last_error() or b"").decode())
    assert np.all(buf[0] == SENT) and np.all(buf[-1] == SENT) and np.all(buf[:, n:] == SENT), "guard rows and padding columns"
    return buf[1:-1, :n]


def test_the_reference_statements_of_the_special_cases():
    t = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, 800.0, -800.0, 745.0, 746.0, 1.0])
    d = ref.hfc_decay_mp(t)
    assert _bits(d.rounded[[0, 1, 3, 4, 5, 6]]).tolist() == _bits([0.0, np.inf, 1.0, 1.0, 0.0, np.inf]).tolist()
    assert math.isnan(d.rounded[2])
    assert d.rounded[7] == 5e-324 and d.rounded[8] == 0.0 and d.rounded[9] == 0.36787944117144233
    assert 0 < d.exact[5] < Fraction(1, 2 ** 1100) and d.exact[6] > 2 ** 1100          # the exact values stay rationals
    # ulp_err: units of 2^-1074 below the normal range, the value's own last place above it; a special is met or missed
    sub = ref.Decay([Fraction(5, 2 ** 1075)], np.array([ref._round_fraction(Fraction(5, 2 ** 1075))]))   # 2.5 units
    assert ref.ulp_err([5e-324 * 3], sub)[0] == 0.5 and ref.ulp_err([0.0], sub)[0] == 2.5
    one = ref.Decay([Fraction(1) + Fraction(1, 2 ** 54)], np.array([1.0]))
    assert ref.ulp_err([1.0], one)[0] == 0.25 and ref.ulp_err([1.0 + 2.0 ** -52], one)[0] == 0.75
    assert ref.ulp_err(d.rounded, d).max() <= 0.5
    wrong = d.rounded.copy()
    wrong[0], wrong[3], wrong[6] = -0.0, np.nextafter(1.0, 2.0), ref.DBL_MAX
    e = ref.ulp_err(wrong, d)
    assert np.isinf(e[0]) and np.isinf(e[3]) and e[6] > 1e10 and np.all(e[[1, 2, 4]] == 0.0) and 0 < e[5] < 1e-20


@pytest.mark.parametrize("seed", ref.LHS_SEEDS)
def test_uint64_rows_equal_the_python_integers(seed):
    """lhs_rows_ref against lhs_ints at 19 designs x 11 dimensions x the two ends of the design and two members inside."""
    pairs = 0
    for n_total in ref.LHS_TOTALS:
        members = sorted({0, n_total // 3, (2 * n_total) // 3, n_total - 1})
        for dim in ref.LHS_DIMS:
            stratum, jbits = ref.lhs_strata_ref(seed, n_total, dim, members)
            for i, m in enumerate(members):
                s, j, u = ref.lhs_ints(seed, n_total, dim, m)
                assert (s, j) == (int(stratum[i]), int(jbits[i])) and 0 <= s < n_total and 0 <= j < 1 << 24, (n_total, dim, m)
                got = ref.lhs_rows_ref(seed, n_total, [dim], m, m + 1)[0, 0]
                assert got.hex() == u.hex() and s < u * n_total < s + 1, (n_total, dim, m)
                pairs += 1
    assert pairs > 600
    assert [ref.half_bits_of(n) for n in ref.LHS_TOTALS] == [1, 1, 1, 1, 2, 2, 2, 3, 4, 4, 5, 6, 6, 7, 8, 8, 9, 14, 14]


@pytest.mark.parametrize("n_total", ref.LHS_TOTALS)
def test_reference_equals_the_numpy_twin_and_the_host_twin(n_total):
    seed = ref.LHS_SEEDS[0]
    assert seed == prm.LHS_SEED and ref.LHS_MAX_TOTAL == _capi.LHS_MAX_TOTAL
    windows = [(0, n_total)] if n_total <= SMALL else ref.lhs_windows(n_total)
    for m0, n in windows:
        want = ref.lhs_rows_ref(seed, n_total, ref.LHS_DIMS, m0, m0 + n)
        assert np.all((want > 0.0) & (want < 1.0))
        assert np.array_equal(_bits(prm.lhs_rows(n_total, ref.LHS_DIMS, m0, m0 + n)), _bits(want)), (n_total, m0, n)
        for pad in (0, 3):
            assert np.array_equal(_bits(_host_twin(seed, n_total, m0, n, 0, 11, pad)), _bits(want)), (n_total, m0, n, pad)
    m0, n = ref.lhs_windows(n_total)[-1]
    other = ref.LHS_SEEDS[1]
    want = ref.lhs_rows_ref(other, n_total, ref.LHS_DIMS, m0, m0 + n)
    assert np.array_equal(_bits(prm.lhs_rows(n_total, ref.LHS_DIMS, m0, m0 + n, seed=other)), _bits(want))
    assert np.array_equal(_bits(_host_twin(other, n_total, m0, n, 4, 3, 3)), _bits(want[4:7])), "dim0 = 4, n_dim = 3"


@pytest.mark.parametrize("n_total", [n for n in ref.LHS_TOTALS if n <= SMALL])
def test_the_stratum_is_a_permutation_in_every_dimension(n_total):
    members = np.arange(n_total)
    for seed in ref.LHS_SEEDS:
        for dim in ref.LHS_DIMS:
            stratum, _ = ref.lhs_strata_ref(seed, n_total, dim, members)
            assert np.array_equal(np.sort(stratum.astype(np.int64)), members), (seed, n_total, dim)


def test_wrong_designs_differ_at_the_windows_the_device_is_tested_at():
    """The sizes are sharp.  Restating the design with half_bits one off, with a cycle-walk that also stops at x == n_total, or
    with dim0 ignored gives other numbers where the device is compared — so a kernel with that defect cannot equal lhs_rows_ref
    there.  The walk's end can only show where 4^half_bits > n_total (not at 4, 16, 256, 4096, 65536, 2^28), and only at the
    members whose walk passes x == n_total: every whole design up to 70 000 has some in every dimension looked at; of the
    2^28 - 1 design exactly ONE member per dimension has, and lhs_windows() puts a window over dimension 0's."""
    seed = ref.LHS_SEEDS[0]
    for n_total in ref.LHS_TOTALS:
        h = ref.half_bits_of(n_total)
        up = down = 0
        for m0, n in ref.lhs_windows(n_total):
            for m in range(m0, m0 + n, max(1, n // 16)):
                for dim in (0, 10):
                    good = ref.lhs_ints(seed, n_total, dim, m)
                    up += ref.lhs_ints(seed, n_total, dim, m, half_bits=h + 1) != good
                    if h > 1 and m < 4 ** (h - 1):              # a narrower network is a bijection of fewer members only
                        down += ref.lhs_ints(seed, n_total, dim, m, half_bits=h - 1) != good
        assert (up > 0 or n_total == 1) and (h == 1 or down > 0), (n_total, up, down)   # one member: one stratum, whatever the network
    walked = [n for n in ref.LHS_TOTALS if 4 ** ref.half_bits_of(n) > n]
    assert walked == [1, 2, 3, 5, 15, 17, 255, 257, 4095, 4097, 65_535, 65_537, (1 << 28) - 1]
    for n_total in walked[:-1]:
        members = np.arange(n_total)
        hit = [int((ref.lhs_strata_ref(seed, n_total, dim, members, stop_at_n_total=True)[0] == n_total).sum()) for dim in ref.LHS_DIMS]
        assert max(hit) == 1 and sum(hit) >= 1, (n_total, hit)    # at most one member per dimension: the network is a bijection
    n_total = walked[-1]
    m0, n = ref.lhs_windows(n_total)[2]
    star = ref.lhs_preimage(seed, n_total, 0, n_total)
    assert m0 % 2 == 1 and m0 <= star < m0 + n
    assert ref.lhs_ints(seed, n_total, 0, star, accept=lambda x, nt: x <= nt)[0] == n_total > ref.lhs_ints(seed, n_total, 0, star)[0]
    # dim0 ignored: rows 4..6 are not rows 0..2
    a = ref.lhs_rows_ref(seed, 257, [4, 5, 6], 0, 257)
    b = ref.lhs_rows_ref(seed, 257, [0, 1, 2], 0, 257)
    assert (a != b).mean() > 0.99


def test_glibc_and_numpy_meet_the_bound_the_device_is_held_to():
    """c_oracle.hfc_conc (glibc's exp) and np.exp on the three time sets, against the 50-digit values, under the bound of
    tests/test_first_kernels_gpu.py — the reference alone meets the condition.  Measured here (glibc 2.35, NumPy 2.2.6,
    2026-10-21), worst error in ulp for (normal, subnormal-or-zero) results:
                 uniform           integers            logspaced
        glibc    (0.4723, none)    (0.4997, 0.4924)    (0.5003, 0.4287)
        NumPy    (0.6148, none)    (0.5720, 0.4924)    (0.6222, 0.4287)"""
    e0 = np.array([1.0, 10.0])
    for name, t in ref.hfc_time_sets().items():
        want = ref.hfc_time_refs()[name]
        with np.errstate(over="ignore", under="ignore"):
            out = c_oracle.hfc_conc(e0, t)
            npy = np.exp(-t)
        assert np.array_equal(_bits(out[:, 1]), _bits(10.0 * out[:, 0]))
        for who, d in (("glibc", out[:, 0]), ("numpy", npy)):
            worst_n, worst_s, at = ref.worst_errors(d, want)
            print(f"{who} {name}: worst {worst_n:.4f} ulp (normal) {worst_s:.4f} ulp (subnormal or zero) at t = {t[at]!r}")
            assert max(worst_n, worst_s) <= ref.EXP_ULP_BOUND, (who, name, worst_n, worst_s, float(t[at]))
    assert ref.EXP_ULP_BOUND in (1.0, 2.0)
    sub = ref.is_subnormal_or_zero(ref.hfc_time_refs()["integers"].rounded)
    assert sub[709:].all() and not sub[:709].any()               # config 1 does walk the subnormal range: t = 709 .. 745


def test_both_entry_points_refuse_before_any_launch():
    lib = _capi.load()
    out = np.full((4, 8), SENT)
    ptr = out.ctypes.data_as(ctypes.c_void_p)
    top = ref.LHS_MAX_TOTAL
    device = lambda *a: lib.fiveeq_lhs_rows_f64(*a, ptr, None)   # noqa: E731  (refused, or empty: nothing is ever launched)
    host = lambda *a: lib.fiveeq_lhs_rows_host_f64(*a, ptr)      # noqa: E731
    for fn in (device, host):
        assert fn(1, top, top - 1, 0, 0, 1, 8) == _capi.OK                       # 2^28 is a design; an empty window of it
        assert fn(1, top + 1, top - 1, 0, 0, 1, 8) == _capi.E_INVALID            # 2^28 + 1 is not, even for no members
        assert fn(1, 0, 0, 0, 0, 1, 8) == _capi.E_INVALID
        assert fn(1, 10, 0, 4, 0, 1, 3) == _capi.E_INVALID                       # ld < n
        assert fn(1, 10, 8, 4, 0, 1, 8) == _capi.E_INVALID                       # [8, 12) outside [0, 10)
        assert fn(1, 10, -1, 4, 0, 1, 8) == _capi.E_INVALID
        assert fn(1, 10, 11, 0, 0, 1, 8) == _capi.E_INVALID                      # an empty window past the design
        assert fn(1, 10, 0, 4, -1, 1, 8) == _capi.E_INVALID
        assert (lib.fiveeq_last_error() or b"").decode()
    assert host(1, top, top - 4, 4, 0, 1, 8) == _capi.OK and np.all(out[0, :4] != SENT)      # the host twin does compute there
    assert np.array_equal(_bits(out[0, :4]), _bits(ref.lhs_rows_ref(1, top, [0], top - 4, top)[0]))
    assert np.all(out[0, 4:] == SENT) and np.all(out[1:] == SENT)
    # fiveeq_hfc_conc_f64 checks its shape before it launches too
    for args in ((0, 8, 4), (4, 3, 4), (4, 8, -1)):
        assert lib.fiveeq_hfc_conc_f64(*args, ptr, ptr, ptr, None) == _capi.E_INVALID, args
    assert lib.fiveeq_hfc_conc_f64(4, 8, 0, ptr, ptr, ptr, None) == _capi.OK and np.all(out[1:] == SENT)    # no time points: nothing to do
