"""The two oldest device kernels through the C ABI, against tests/first_kernels_reference.py (which shares nothing with the
package and is itself held to exact integers, the NumPy twin and the host twin in tests/test_first_kernels_cpu.py):

  hfc_conc_kernel (fiveeq_hfc_conc_f64)   out[k][m] = e0[m] exp(-time[k]): every size around its 256-point LDS tile and its
      256-member workgroup, ld = N and N + 3, aligned and one element off, guard rows before and after; the staged factor the
      same bits in every workgroup, every element ONE rounded product of it; the factor against a 50-digit exp with no absolute
      floor (subnormal results in units of 2^-1074); BASELINE config 1 on the device; special times at the tile edge; streams,
      split calls and repeated calls.
  lhs_kernel (fiveeq_lhs_rows_f64)        every bit of the design at and around the powers of four up to 2^28, in windows at both
      ends and in the middle, ld = n and n + 3, guard rows, dim0 > 0, ragged and empty windows, the permutation, a stream.

Raw device pointers throughout, so that ld, offsets and guards are the test's."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import first_kernels_reference as ref
from fiveeqscm_amd import _capi
from utility_reference import strata

pytestmark = pytest.mark.gpu

SENT = 0x7FF85EA71E55C0DE      # a NaN with a payload no kernel here produces
BLOCK = 256                    # FIVEEQ_BLOCK: members per workgroup and time points per LDS tile
PAD = 3
SEED = ref.LHS_SEEDS[0]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _ptr(t, elements=0):
    return ctypes.c_void_p(t.data_ptr() + 8 * elements)


def _stream_arg(stream):
    return None if stream is None else ctypes.c_void_p(stream.cuda_stream)


def _embedded(values, off):
    """fp64 values at element `off` of a sentinel-filled, 16-byte aligned device buffer with one sentinel after them."""
    host = np.full(off + values.size + 1, SENT, dtype=np.int64)
    host[off:off + values.size] = _bits(values)
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 16 == 0
    return host, dev


def _same_bits(a, b):
    """Equal bit patterns; where one side is a NaN the other must be one too (the payload is not compared)."""
    na, nb = np.isnan(a.view(np.float64)), np.isnan(b.view(np.float64))
    return np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb])


# ---- fiveeq_hfc_conc_f64 -----------------------------------------------------------------------------------------------------
class HfcCall:
    """One layout of a call: e0 [N] and time [K] at element `off` of their buffers, out [K][ld] behind one guard row, with one
    guard row after it, inside a sentinel-filled buffer that starts `off` elements before the guard row."""

    def __init__(self, e0, time, pad, off):
        self.N, self.K, self.ld, self.off = e0.size, time.size, e0.size + pad, off
        self.e0_host, self.e0 = _embedded(e0, off)
        self.t_host, self.time = _embedded(time, off)
        self.out = torch.full((off + (self.K + 2) * self.ld,), SENT, dtype=torch.int64, device="cuda")
        assert self.out.data_ptr() % 16 == 0 and (self.e0.data_ptr() + 8 * off) % 16 == 8 * off
        self.wait_for_all = False
        torch.cuda.synchronize()                               # the buffers are ready whichever stream the call runs on

    def launch(self, a=0, b=None, stream=None):
        lib = _capi.load()
        b = self.K if b is None else b
        rc = lib.fiveeq_hfc_conc_f64(self.N, self.ld, b - a, _ptr(self.e0, self.off), _ptr(self.time, self.off + a),
                                     _ptr(self.out, self.off + (1 + a) * self.ld), _stream_arg(stream))
        assert rc == _capi.OK, (self.N, self.K, self.ld, (lib.fiveeq_last_error() or b"").decode())
        if stream is None:
            self.wait_for_all = True
        else:
            stream.synchronize()                               # ONLY the stream it was handed
        return self

    def read(self):
        """[K, N] bit patterns, after the guards, the padding and the inputs have been found untouched."""
        if self.wait_for_all:
            torch.cuda.synchronize()
        h = self.out.cpu().numpy()
        first = self.off + self.ld
        assert np.all(h[:first] == SENT), "the guard row before out"
        assert np.all(h[first + self.K * self.ld:] == SENT), "the guard row after out (a row past the last)"
        body = h[first:first + self.K * self.ld].reshape(self.K, self.ld)
        assert np.all(body[:, self.N:] == SENT), "padding columns [N, ld)"
        assert np.array_equal(self.e0.cpu().numpy(), self.e0_host) and np.array_equal(self.time.cpu().numpy(), self.t_host), "inputs"
        return body[:, :self.N].copy()


ONES = (0, BLOCK, 2 * BLOCK)                                     # e0 == 1.0 at one member of every workgroup
SPECIAL_E0 = (0.0, -0.0, 12345 * 5e-324, np.inf, np.nan, -3.0, -np.inf, 1e300)


def _e0(N, seed):
    """Random members of both signs; 1.0 at columns 0, 256, 512; zeros, a subnormal, infinities and a NaN behind columns 0 and 256."""
    e = np.random.default_rng(seed).normal(size=N) * 10.0
    for start in (1, BLOCK + 1):
        for i, s in enumerate(SPECIAL_E0, start=start):
            if i < N:
                e[i] = s
    for c in ONES:
        if c < N:
            e[c] = 1.0
    return e


def _times(K, seed):
    """Uniform on [-2, 30]; from K = 255 on also a factor deep in the subnormal range, one just inside it and one near 1e306."""
    t = np.random.default_rng(seed).uniform(-2.0, 30.0, K)
    if K >= 255:
        t[K - 1], t[K - 2], t[K // 2] = 730.0, -705.0, 708.5
    return t


def _check_structure(got, e0, what):
    """d[k] = the column of the first e0 == 1: the same bits at every other such column (the workgroups agree on the staged
    factor), and every element the one IEEE product e0[m] * d[k].  Returns d."""
    val = got.view(np.float64)
    ones = [c for c in ONES if c < e0.size]
    d = val[:, ones[0]].copy()
    for c in ones[1:]:
        assert _same_bits(got[:, c], _bits(d)), (what, "workgroups disagree on exp(-time)", c)
    with np.errstate(all="ignore"):
        want = _bits(e0[None, :] * d[:, None])
    nan = np.isnan(want.view(np.float64))
    assert np.array_equal(np.isnan(val), nan), (what, "NaN positions")
    bad = np.argwhere((got != want) & ~nan)
    assert bad.size == 0, (what, "first element that is not e0[m] * d[k]: (k, m)", bad[0].tolist(), len(bad))
    return d


@pytest.mark.parametrize("K", [1, 255, 256, 257, 512, 513])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 513])
def test_hfc_conc_structure_at_every_tile_and_workgroup_edge(N, K):
    """One or two time tiles plus a ragged third x one to three workgroups with a ragged last; ld = N and N + 3; e0 and time
    both 16-byte aligned and both one element off.  Exact: the staged factor, the products, the guard rows, the padding, the
    inputs.  (An `nk` replaced by the tile size writes rows past K into the guard row; an `ld` replaced by `n` moves every row
    of the ld = N + 3 layouts; a tile read before it is complete, or after the next one has begun, is another factor.)"""
    e0, time = _e0(N, 100 * N + K), _times(K, 100 * K + N)
    for pad in (0, PAD):
        for off in (0, 1):
            got = HfcCall(e0, time, pad, off).launch().read()
            d = _check_structure(got, e0, (N, K, pad, off))
            assert np.all(d[:min(K, 250)] > 0) and (K < 255 or (0 < d[K - 1] < 2.3e-308 and d[K - 2] > 1e306))


def test_the_exponential_against_fifty_digits():
    """d[k] = exp(-time[k]) against the 50-digit value on the three time sets, in units of the spacing of the correctly rounded
    result — 2^-1074 for subnormal results — with no absolute floor.  The bound follows the rule stated at
    first_kernels_reference.EXP_ULP_BOUND: the worst measured is within 1 ulp, so 1 ulp is asserted.  Worst error measured on an MI355X (gfx950), ROCm 7.2.0, 2026-10-21, in ulp, for normal /
    subnormal-or-zero results:
        uniform on [-2, 30] (64 points)           0.7199 / none
        the integers 0..749 (config 1)            0.6610 / 0.4924
        513 log-spaced points, both signs, +-745  0.6752 / 0.4287
    A flush-to-zero exp fails here on the integers from t = 709 on: exp(-740) is 80 units of 2^-1074."""
    sets, refs = ref.hfc_time_sets(), ref.hfc_time_refs()
    e0 = _e0(257, 1)
    for name, t in sets.items():
        got = HfcCall(e0, t, PAD, 1).launch().read()
        d = _check_structure(got, e0, name)
        worst_n, worst_s, at = ref.worst_errors(d, refs[name])
        print(f"device exp {name}: worst {worst_n:.4f} ulp (normal) {worst_s:.4f} ulp (subnormal or zero) at t = {t[at]!r}: "
              f"got {d[at].hex()} want {refs[name].rounded[at].hex()}")
        assert max(worst_n, worst_s) <= ref.EXP_ULP_BOUND, (name, worst_n, worst_s, float(t[at]))


def test_config_1_on_the_device():
    """BASELINE config 1, e0 = 10 over t = 0..749: through the subnormal range to zero.  Observed on an MI355X (gfx950), ROCm 7,
    2026-10-21: the last non-zero output is at t = 745; out[744..746] = 0x0.0000000000014p-1022, 0x0.000000000000ap-1022, 0x0.0p+0
    (d[744..746] = 2, 1 and 0 units of 2^-1074) — the bits NumPy gives.
    Asserted: every value is the one product 10 * d[k] and d[k] meets the bound of the exponential test — which makes the value
    at t = 744 (1.55 units of 2^-1074 before rounding) non-zero and leaves the rows behind it to the bound.  NumPy's own tail is
    pinned on the CPU in tests/test_hfc_conc.py."""
    t = ref.hfc_time_sets()["integers"]
    e0 = np.array([1.0, 10.0, -10.0])
    got = HfcCall(e0, t, 0, 0).launch().read()
    d = _check_structure(got, e0, "config 1")
    out = got.view(np.float64)[:, 1]
    last = int(np.flatnonzero(out)[-1])
    print(f"config 1 on the device: last non-zero output at t = {last}; out[744..746] = {[v.hex() for v in out[744:747]]}; "
          f"d[744..746] = {[v.hex() for v in d[744:747]]}")
    worst_n, worst_s, at = ref.worst_errors(d, ref.hfc_time_refs()["integers"])
    assert max(worst_n, worst_s) <= ref.EXP_ULP_BOUND, (worst_n, worst_s, at)
    assert out[0] == 10.0 and last >= 744 and np.array_equal(got[:, 2], _bits(-out))


SPECIAL_TIMES = (np.inf, -np.inf, np.nan, 0.0, -0.0, 800.0, -800.0)
SPECIAL_DECAY = (0.0, np.inf, np.nan, 1.0, 1.0, 0.0, np.inf)


def test_special_times_on_both_sides_of_the_tile_edge():
    """t in {+inf, -inf, NaN, +0, -0, 800, -800} gives d = {+0, +inf, NaN, 1, 1, +0, +inf} exactly, at each of the indices
    254..257 of a K = 513 call (seven calls, the specials rotated through the four slots); the products follow IEEE: 0 x inf
    and inf x 0 are NaN, -3 x +0 is -0."""
    K, N = 513, 257
    e0 = _e0(N, 2)
    zero, minus3, inf = 1, 6, 4
    assert (e0[zero], e0[minus3], e0[inf]) == (0.0, -3.0, np.inf) and not np.signbit(e0[zero])
    for r in range(len(SPECIAL_TIMES)):
        time = _times(K, 50 + r)
        slots = {254 + j: (r + j) % len(SPECIAL_TIMES) for j in range(4)}
        for k, s in slots.items():
            time[k] = SPECIAL_TIMES[s]
        got = HfcCall(e0, time, PAD, 1).launch().read()
        d = _check_structure(got, e0, ("special times", r))
        for k, s in slots.items():
            want = SPECIAL_DECAY[s]
            assert (np.isnan(d[k]) if np.isnan(want) else _bits(d[k]) == _bits(want)), (r, k, SPECIAL_TIMES[s], d[k].hex())
            row = got[k].view(np.float64)
            if want == 0.0:
                assert _bits(row[minus3]) == _bits(-0.0) and np.isnan(row[inf]) and _bits(row[zero]) == _bits(0.0), (r, k)
            elif want == np.inf:
                assert row[minus3] == -np.inf and np.isnan(row[zero]) and row[inf] == np.inf, (r, k)
            elif want == 1.0:
                assert np.array_equal(got[k][~np.isnan(e0)], _bits(e0)[~np.isnan(e0)]), (r, k)
            else:
                assert np.isnan(row).all(), (r, k)


def test_hfc_conc_does_not_depend_on_how_it_is_launched():
    """The bits of one call on the default stream are also those of the same call on a stream of its own (synchronised alone),
    of two calls over [0, 300) and [300, K) into one buffer (the second call's tiles start at 300), and of the call made twice."""
    N, K = 513, 513
    e0, time = _e0(N, 3), _times(K, 4)
    base = HfcCall(e0, time, PAD, 1).launch().read()
    _check_structure(base, e0, "base")
    assert np.array_equal(HfcCall(e0, time, PAD, 1).launch(stream=torch.cuda.Stream()).read(), base), "a non-default stream"
    assert np.array_equal(HfcCall(e0, time, PAD, 1).launch(0, 300).launch(300, K).read(), base), "two calls"
    assert np.array_equal(HfcCall(e0, time, PAD, 1).launch(300, K).launch(0, 300).read(), base), "two calls, the later rows first"
    assert np.array_equal(HfcCall(e0, time, PAD, 1).launch().launch().read(), base), "a second identical call"


# ---- fiveeq_lhs_rows_f64 -----------------------------------------------------------------------------------------------------
N_DIM = len(ref.LHS_DIMS)


def _lhs(n_total, m0, n, *, seed=SEED, dim0=0, n_dim=N_DIM, pad=0, stream=None):
    """Members [m0, m0 + n) into rows ld = n + pad apart behind one guard row, one guard row after: [n_dim, n] bit patterns."""
    lib = _capi.load()
    ld = n + pad
    out = torch.full(((n_dim + 2) * ld,), SENT, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc = lib.fiveeq_lhs_rows_f64(seed, n_total, m0, n, dim0, n_dim, ld, _ptr(out, ld), _stream_arg(stream))
    assert rc == _capi.OK, (n_total, m0, n, (lib.fiveeq_last_error() or b"").decode())
    if stream is None:
        torch.cuda.synchronize()
    else:
        stream.synchronize()
    h = out.cpu().numpy().reshape(n_dim + 2, ld)
    assert np.all(h[0] == SENT) and np.all(h[-1] == SENT), "guard rows"
    assert np.all(h[:, n:] == SENT), "padding columns [n, ld)"
    return h[1:-1, :n].copy()


@functools.lru_cache(maxsize=None)
def _want(n_total, m0, n, seed=SEED):
    w = _bits(ref.lhs_rows_ref(seed, n_total, ref.LHS_DIMS, m0, m0 + n))
    w.setflags(write=False)
    return w


@pytest.mark.parametrize("n_total", ref.LHS_TOTALS)
def test_lhs_kernel_gives_the_reference_bits(n_total):
    """Every window of first_kernels_reference.lhs_windows (n of {1, 255, 256, 257, 513}, both ends of the design, odd starts in
    the middle), 11 dimensions, ld = n and n + 3, a guard row on either side — and one window under a seed with the top bit set.
    half_bits one off, or a walk that stops at x == n_total, gives other numbers in these very windows
    (tests/test_first_kernels_cpu.py::test_wrong_designs_differ_at_the_windows_the_device_is_tested_at)."""
    for m0, n in ref.lhs_windows(n_total):
        for pad in (0, PAD):
            got = _lhs(n_total, m0, n, pad=pad)
            bad = np.argwhere(got != _want(n_total, m0, n))
            assert bad.size == 0, (n_total, m0, n, pad, "first (dimension, member) that differs", bad[0].tolist(), len(bad))
    m0, n = ref.lhs_windows(n_total)[0]
    other = ref.LHS_SEEDS[1]
    assert np.array_equal(_lhs(n_total, m0, n, seed=other, pad=PAD), _want(n_total, m0, n, other)), (n_total, "seed 2")


@pytest.mark.parametrize("n_total", [257, 65_537, (1 << 28) - 1])
def test_lhs_dim0_selects_the_rows(n_total):
    """dim0 = 4, n_dim = 3 gives rows 4..6 of the 11-row call (a kernel that ignores dim0 gives rows 0..2)."""
    m0, n = ref.lhs_windows(n_total)[2 if n_total > 513 else 0]
    got = _lhs(n_total, m0, n, dim0=4, n_dim=3, pad=PAD)
    assert np.array_equal(got, _lhs(n_total, m0, n, pad=PAD)[4:7]) and np.array_equal(got, _want(n_total, m0, n)[4:7])
    assert not np.array_equal(got, _want(n_total, m0, n)[0:3])


def test_lhs_ragged_windows_join_and_an_empty_one_writes_nothing():
    lib = _capi.load()
    n_total, m0, n = 65_537, 1001, 513
    whole = _lhs(n_total, m0, n, pad=PAD)
    assert np.array_equal(whole, _want(n_total, m0, n))
    cuts = [(m0, 200), (m0 + 200, 0), (m0 + 200, n - 200)]
    parts = [_lhs(n_total, a, k, pad=PAD) for a, k in cuts if k]
    assert np.array_equal(np.concatenate(parts, axis=1), whole)
    out = torch.full((64,), SENT, dtype=torch.int64, device="cuda")
    a, k = cuts[1]
    for ld in (0, 5):
        assert lib.fiveeq_lhs_rows_f64(SEED, n_total, a, k, 0, N_DIM, ld, _ptr(out, 8), None) == _capi.OK
    assert lib.fiveeq_lhs_rows_f64(SEED, n_total, n_total, 0, 0, N_DIM, 0, _ptr(out, 8), None) == _capi.OK      # empty, at the very end
    assert lib.fiveeq_lhs_rows_f64(SEED, n_total, a, 5, 4, 0, 5, _ptr(out, 8), None) == _capi.OK                # no dimensions
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


@pytest.mark.parametrize("n_total", [n for n in ref.LHS_TOTALS if n <= 70_000])
def test_lhs_whole_design_is_one_member_per_stratum(n_total):
    """All members, in windows of 513: the bits of the reference, 0 < u < 1, and floor(u * n_total) — in exact integers from the
    bits of u — a permutation in every dimension."""
    cols = []
    for m0 in range(0, n_total, ref.WINDOW):
        cols.append(_lhs(n_total, m0, min(ref.WINDOW, n_total - m0)))
    got = np.concatenate(cols, axis=1)
    assert np.array_equal(got, _want(n_total, 0, n_total))
    u = got.view(np.float64)
    assert np.all((u > 0.0) & (u < 1.0))
    members = np.arange(n_total)
    for k in range(N_DIM):
        assert np.array_equal(np.sort(strata(u[k], n_total)), members), (n_total, k)


def test_lhs_on_a_stream_of_its_own():
    n_total = 1 << 28
    m0, n = ref.lhs_windows(n_total)[1]
    got = _lhs(n_total, m0, n, pad=PAD, stream=torch.cuda.Stream())
    assert np.array_equal(got, _want(n_total, m0, n)) and np.array_equal(got, _lhs(n_total, m0, n, pad=PAD))
