"""Running means and trends without a GPU: the C ABI (exported, bound, additive, validated on the host), the NumPy twin of the
kernels against the independent reference (tests/smooth_reference.py) on the layouts the GPU test holds the kernels to, and the
host side of smooth.running_mean / window_trends under host_passes()."""
import ctypes
import os

import numpy as np
import pytest
import torch

import smooth_reference as ref
from fiveeqscm_amd import _capi, _smooth_host
from fiveeqscm_amd.smooth import SmoothedRows, WindowTrends, running_mean, window_trends

NEW = ["fiveeq_max_smooth_window", "fiveeq_smooth_tile", "fiveeq_smooth_unroll", "fiveeq_running_mean_f64", "fiveeq_running_mean_f32",
       "fiveeq_window_trends_f64", "fiveeq_window_trends_f32"]


def test_new_symbols_are_exported_and_the_abi_is_additive():
    lib = _capi.load()
    for name in NEW:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    assert lib.fiveeq_abi_version() == _capi.ABI_VERSION == 13
    assert lib.fiveeq_sizeof_model() == ctypes.sizeof(_capi.Model) == 448
    assert lib.fiveeq_max_smooth_window() == _capi.MAX_SMOOTH_WINDOW == 32
    assert any(os.path.basename(p) == "fiveeq_smooth.hpp" for p in _capi.SOURCES), "the new header is not under the stamped source hash"
    # the kernel's shape comes from the library: a lane owns 16 bytes of a row, a workgroup whole waves of them
    t8, t4 = lib.fiveeq_smooth_tile(8), lib.fiveeq_smooth_tile(4)
    assert t8 > 0 and t8 % 128 == 0 and t4 == 2 * t8 and lib.fiveeq_smooth_tile(2) == 0
    assert lib.fiveeq_smooth_unroll(1) >= 1 and lib.fiveeq_smooth_unroll(0) >= 1
    assert len(_capi.SIGNATURES["fiveeq_running_mean_f64"][1]) == 13 and len(_capi.SIGNATURES["fiveeq_window_trends_f64"][1]) == 12


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_the_running_mean_validates_on_the_host(sfx):
    """Every call returns on the host with an error code and a message: the fake pointers are never dereferenced."""
    lib = _capi.load()
    fn = getattr(lib, f"fiveeq_running_mean_{sfx}")
    w = 8 if sfx == "f64" else 4
    p = ctypes.c_void_p(0x1000)
    E = _capi.E_INVALID
    err = lambda: lib.fiveeq_last_error().decode()   # noqa: E731
    odd = lambda k: ctypes.c_void_p(0x1000 + k)      # noqa: E731

    def call(n_scen=1, n_rows=6, n=8, ld=8, rows=p, scen_stride=48, window=3, n_tail=2, tail=p, tail_stride=16, out=p, out_stride=48):
        return fn(n_scen, n_rows, n, ld, rows, scen_stride, window, n_tail, tail, tail_stride, out, out_stride, None)

    for n_scen in (0, -1, lib.fiveeq_max_scenarios() + 1):
        assert call(n_scen=n_scen) == E and "n_scen" in err()
    assert call(n_rows=-1) == E and "n_rows" in err()
    assert call(n=0) == E and "n_members" in err()
    assert call(n=2 ** 31, ld=2 ** 31) == E and "n_members" in err()
    assert call(n=8, ld=7) == E and "ld=" in err()
    assert call(n_scen=2, scen_stride=47) == E and "scen_stride" in err()
    assert call(n_scen=2, tail_stride=15) == E and "tail_scen_stride" in err()
    assert call(n_scen=2, out_stride=47) == E and "out_scen_stride" in err()          # n_out = 2 + 6 - 3 + 1 = 6 rows of 8
    for window in (0, -1, 33):
        assert call(window=window, n_tail=0) == E and "window" in err()
    for n_tail in (-1, 3):
        assert call(n_tail=n_tail) == E and "n_tail" in err()
    for kw, needle in [(dict(rows=None), "rows"), (dict(tail=None), "tail"), (dict(out=None), "out")]:
        assert call(**kw) == E and needle in err() and "NULL" in err(), kw
    for kw, needle in [(dict(rows=odd(w // 2)), "rows"), (dict(tail=odd(w // 2)), "tail"), (dict(out=odd(4)), "out")]:
        assert call(**kw) == E and needle in err() and "aligned" in err(), kw
    # what need not be there: rows with no rows, the tail with none, out with no output — validated, nothing launched
    assert call(n_rows=0, rows=None, out=None) == _capi.OK                             # 2 + 0 < 3: no output
    assert call(n_rows=0, n_tail=0, rows=None, tail=None, out=None) == _capi.OK
    assert call(n_rows=2, n_tail=0, tail=None, out=None) == _capi.OK                   # fewer rows than a window
    assert call(n_rows=3, n_tail=0, tail=None, out=None) == E and "out" in err()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_the_window_trends_validate_on_the_host(sfx):
    lib = _capi.load()
    fn = getattr(lib, f"fiveeq_window_trends_{sfx}")
    w = 8 if sfx == "f64" else 4
    p = ctypes.c_void_p(0x1000)
    wn = (ctypes.c_int32 * 8)(0, 5, 5, 5, 2, 9, 0, 1)
    E = _capi.E_INVALID
    err = lambda: lib.fiveeq_last_error().decode()   # noqa: E731
    odd = lambda k: ctypes.c_void_p(0x1000 + k)      # noqa: E731

    def call(n_scen=1, n_rows=4, n=8, ld=8, rows=p, scen_stride=32, steps=p, W=2, windows=wn, tsum=p, first=1):
        return fn(n_scen, n_rows, n, ld, rows, scen_stride, steps, W, ctypes.cast(windows, ctypes.c_void_p) if windows else None, tsum, first,
                  None)

    for n_scen in (0, -1, lib.fiveeq_max_scenarios() + 1):
        assert call(n_scen=n_scen) == E and "n_scen" in err()
    assert call(n_rows=-1) == E and "n_rows" in err()
    assert call(n=0) == E and "n_members" in err()
    assert call(n=2 ** 31, ld=2 ** 31) == E and "n_members" in err()
    assert call(n=8, ld=7) == E and "ld=" in err()
    assert call(n_scen=2, scen_stride=31) == E and "scen_stride" in err()
    for W in (-1, 5):
        assert call(W=W) == E and "n_windows" in err()
    assert call(windows=(ctypes.c_int32 * 8)(0, 5, 6, 5, 0, 0, 0, 0)) == E and "windows[1]" in err()
    assert call(windows=(ctypes.c_int32 * 8)(-1, 5, 0, 0, 0, 0, 0, 0), W=1) == E and "windows[0]" in err()
    for kw, needle in [(dict(rows=None), "rows"), (dict(steps=None), "steps"), (dict(tsum=None), "tsum"), (dict(windows=None), "windows")]:
        assert call(**kw) == E and needle in err() and "NULL" in err(), kw
    for kw, needle in [(dict(rows=odd(w // 2)), "rows"), (dict(steps=odd(2)), "steps"), (dict(tsum=odd(4)), "tsum")]:
        assert call(**kw) == E and needle in err() and "aligned" in err(), kw
    assert call(n_rows=0, rows=None, steps=None, first=0) == _capi.OK
    assert call(n_rows=0, rows=None, steps=None, first=0, tsum=None) == E
    assert call(W=0, windows=None, tsum=None) == _capi.OK                              # no window: no state, nothing to do


# ---- the NumPy twin against the reference, on the GPU test's layouts -----------------------------------------------------------
TWIN = ref.HostBackend(_smooth_host.SmoothPasses())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_host_twin_equals_the_reference(dtype):
    itemsize = np.dtype(dtype).itemsize
    seed = 0
    for n in (1, 5, 67):
        for window in (1, 2, 3, 7, 20, 32):
            for k in ref.rows_of(window, (2, 8)):
                for ld, off, gap, S in ref.layouts_of(n, itemsize):
                    seed += 1
                    xs = [ref.make_rows(k, n, dtype, 31 * seed + s) for s in range(S)]
                    ref.check_mean(TWIN, xs, window, ld=ld, off=off, gap=gap)
                    if window == 7 and k > 2:
                        ref.check_mean(TWIN, xs, window, ld=ld, off=off, gap=gap, cuts=(1, k // 2, k - 1))
    for n in (1, 5, 67):
        for k in (0, 1, 2, 9, 17):
            steps = ref.steps_of(k, first=3, stride=2)
            for windows in ((), ((0, 100),), ((5, 20), (20, 20), (0, 4), (4, 36))):
                for ld, off, gap, S in ref.layouts_of(n, itemsize):
                    xs = [ref.make_rows(k, n, dtype, 7 * k + n + s) for s in range(S)]
                    ref.check_trend(TWIN, xs, steps, windows, ld=ld, off=off, gap=gap, poison=True)
                    if k > 2:
                        ref.check_trend(TWIN, xs, steps, windows, ld=ld, off=off, gap=gap, cuts=(1, k // 2, k - 1))


def test_the_inputs_tell_the_excluded_implementations_apart():
    """On the test inputs a sliding add / subtract update and a multiply by the reciprocal each differ from the definition in
    at least one bit, in members that hold no NaN and no infinity: a test that passes on them holds the kernel to the
    definition and to nothing close to it."""
    for dtype in (np.float64, np.float32):
        x = ref.make_rows(43, 67, dtype, 5)
        ok = ref.finite_members(x)
        for window in (3, 7, 20):
            want = ref.running_mean(x, window)[:, ok]
            assert np.isfinite(want).all()
            assert (ref.bits(ref.sliding_mean(x, window)[:, ok]) != ref.bits(want)).any(), (dtype, window, "sliding")
            assert (ref.bits(ref.reciprocal_mean(x, window)[:, ok]) != ref.bits(want)).any(), (dtype, window, "reciprocal")


# ---- smooth.running_mean / window_trends on host tensors, through the twin ------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int64)


def test_running_mean_host_side():
    K, N, window = 23, 37, 7
    x = ref.make_rows(K, N, np.float64, 3)
    rows = torch.from_numpy(x)
    steps = ref.steps_of(K, first=10, stride=2)
    with pytest.raises(TypeError, match="no CPU fallback"):
        running_mean(rows, steps, window)                      # host rows outside the context
    with _smooth_host.host_passes():
        want = ref.running_mean(x, window)
        one = running_mean(rows, steps, window)
        assert isinstance(one, SmoothedRows) and one.rows.dtype == torch.float64 and one.rows.shape == (K - window + 1, N)
        assert np.array_equal(ref.bits(one.rows.numpy()), ref.bits(want))
        assert (one.window, one.align) == (window, "centre") and one.seen_steps.tolist() == steps.tolist()
        assert torch.equal(_bits(one.tail), _bits(rows[K - (window - 1):])) and one.tail.dtype == rows.dtype
        # the dating of the outputs, for an odd and an even window: the window's step number window // 2, or its last
        for w_, align, first_step in ((7, "centre", steps[3]), (7, "trailing", steps[6]), (4, "centre", steps[2]), (4, "trailing", steps[3]),
                                      (1, "centre", steps[0]), (1, "trailing", steps[0])):
            sm = running_mean(rows, steps, w_, align=align)
            assert sm.steps.tolist() == (int(first_step) + 2 * np.arange(K - w_ + 1)).tolist(), (w_, align)
        assert running_mean(rows, steps, 20).steps[0] == steps[10]                   # the first year of the second decade
        # window 1: the rows widened, bit for bit; fp32 rows give fp64 outputs
        r32 = torch.from_numpy(ref.make_rows(K, N, np.float32, 4))
        assert torch.equal(_bits(running_mean(r32, steps, 1).rows), _bits(r32.double()))
        # continuation at every cut: the outputs of the two calls, concatenated, are those of one call
        for cut in range(K + 1):
            head = running_mean(rows[:cut], steps[:cut], window)
            rest = running_mean(rows[cut:], steps[cut:], window, state=head)
            assert head.tail.shape[0] == min(window - 1, cut) and rest.tail.shape[0] == window - 1
            assert np.array_equal(ref.bits(torch.cat([head.rows, rest.rows]).numpy()), ref.bits(want)), cut
            assert np.concatenate([head.steps, rest.steps]).tolist() == one.steps.tolist(), cut
            assert rest.seen_steps.tolist() == steps.tolist()
        # row by row
        st = None
        got = []
        for k in range(K):
            st = running_mean(rows[k:k + 1], steps[k:k + 1], window, state=st)
            got.append(st.rows)
        assert np.array_equal(ref.bits(torch.cat(got).numpy()), ref.bits(want))
        # a column-sliced view of a wider buffer (read in place, ld > N) and the scenario axis
        wide = torch.from_numpy(np.ascontiguousarray(np.stack([np.pad(x, ((0, 2), (0, 9))), np.pad(x[::-1], ((0, 2), (0, 9)))])))
        two = running_mean(wide[:, :K, :N], steps, window)
        assert two.rows.shape == (2, K - window + 1, N) and two.tail.shape == (2, window - 1, N)
        assert np.array_equal(ref.bits(two.rows[0].numpy()), ref.bits(want))
        assert np.array_equal(ref.bits(two.rows[1].numpy()), ref.bits(ref.running_mean(x[::-1], window)))
        head = running_mean(wide[:, :9, :N], steps[:9], window)
        rest = running_mean(wide[:, 9:K, :N], steps[9:], window, state=head)
        assert torch.equal(_bits(torch.cat([head.rows, rest.rows], dim=1)), _bits(two.rows))
        # fewer rows than a window: no output, the rows kept as the tail
        few = running_mean(rows[:4], steps[:4], window)
        assert few.rows.shape == (0, N) and few.steps.size == 0 and few.tail.shape == (4, N)
        # refusals
        with pytest.raises(ValueError, match="evenly spaced"):
            running_mean(rows[:4], [1, 2, 4, 5], 2)
        with pytest.raises(ValueError, match="strictly increasing"):
            running_mean(rows[:3], [3, 3, 3], 2)
        with pytest.raises(ValueError, match="evenly spaced"):
            running_mean(rows[4:], steps[4:] + 1, window, state=few)               # not the next evenly spaced step
        with pytest.raises(ValueError, match="does not lie after"):
            running_mean(rows[3:], steps[3:], window, state=few)
        with pytest.raises(ValueError, match="window and align"):
            running_mean(rows[4:], steps[4:], window + 1, state=few)
        with pytest.raises(ValueError, match="window and align"):
            running_mean(rows[4:], steps[4:], window, align="trailing", state=few)
        with pytest.raises(ValueError, match="other rows"):
            running_mean(rows[4:, :N - 1], steps[4:], window, state=few)
        with pytest.raises(ValueError, match="other rows"):
            running_mean(rows[4:].float(), steps[4:], window, state=few)
        for bad in (0, 33, -1, 2.0, True):
            with pytest.raises(ValueError, match="window"):
                running_mean(rows, steps, bad)
        with pytest.raises(ValueError, match="align"):
            running_mean(rows, steps, window, align="middle")
        assert running_mean(rows, steps[:K], 32 if K >= 32 else K).rows.shape[0] == 1


def test_window_trends_host_side():
    K, N = 19, 37
    x = ref.make_rows(K, N, np.float64, 8)
    rows = torch.from_numpy(x)
    steps = ref.steps_of(K, first=3, stride=2)                 # 3, 5, .., 39
    windows = ((5, 20), (20, 20), (39, 60), (0, 100))          # 8 steps; none; one; all
    with pytest.raises(TypeError, match="no CPU fallback"):
        window_trends(rows, steps, windows)
    with _smooth_host.host_passes():
        sx, stx = ref.trend_sums(x, steps, windows)
        one = window_trends(rows, steps, windows, dt=0.5)
        assert isinstance(one, WindowTrends) and one.count == (8, 0, 1, K) and one.windows == windows and one.dt == 0.5
        assert np.array_equal(ref.bits(one.sx.numpy()), ref.bits(sx)) and np.array_equal(ref.bits(one.stx.numpy()), ref.bits(stx))
        assert np.array_equal(ref.bits(one.slope.numpy()), ref.bits(ref.slope_of(sx, stx, steps, windows, 0.5)))
        assert np.isnan(one.slope.numpy()[1]).all() and np.isnan(one.slope.numpy()[2]).all()      # fewer than 2 stored steps
        assert np.isnan(one.mean.numpy()[1]).all()
        ok = ref.finite_members(x)
        assert np.array_equal(one.mean.numpy()[3][ok], (sx[3] / K)[ok]) and np.isfinite(one.slope.numpy()[0][ok]).all()
        # a straight line has its slope: T = 0.25 t + 1 over steps two apart, half a year each
        line = torch.from_numpy(np.repeat((0.25 * steps + 1.0)[:, None], 3, axis=1))
        assert np.array_equal(window_trends(line, steps, ((0, 100),), dt=0.5).slope.numpy(), np.full((1, 3), 0.5))
        # continuation at every cut: the bits of one call, the counts accumulated
        for cut in range(K + 1):
            head = window_trends(rows[:cut], steps[:cut], windows, dt=0.5)
            both = window_trends(rows[cut:], steps[cut:], windows, dt=0.5, state=head)
            for name in ("sx", "stx", "mean", "slope"):
                assert torch.equal(_bits(getattr(both, name)), _bits(getattr(one, name))), (cut, name)
            assert both.count == one.count and both.steps.tolist() == steps.tolist()
        # the scenario axis over a column-sliced view
        wide = torch.from_numpy(np.ascontiguousarray(np.stack([np.pad(x, ((0, 2), (0, 9))), np.pad(x[::-1], ((0, 2), (0, 9)))])))
        two = window_trends(wide[:, :K, :N], steps, windows)
        assert two.sx.shape == (2, 4, N) and torch.equal(_bits(two.sx[0]), _bits(one.sx))
        assert np.array_equal(ref.bits(two.stx[1].numpy()), ref.bits(ref.trend_sums(x[::-1], steps, windows)[1]))
        # no window
        none = window_trends(rows, steps, ())
        assert none.sx.shape == (0, N) and none.slope.shape == (0, N) and none.count == ()
        # refusals
        with pytest.raises(ValueError, match="at most 4"):
            window_trends(rows, steps, [(0, 1)] * 5)
        with pytest.raises(ValueError, match="windows"):
            window_trends(rows, steps, [(5, 4)])
        with pytest.raises(ValueError, match="strictly increasing"):
            window_trends(rows[:3], [3, 9, 9], windows)
        with pytest.raises(ValueError, match="dt"):
            window_trends(rows, steps, windows, dt=0.0)
        head = window_trends(rows[:5], steps[:5], windows)
        with pytest.raises(ValueError, match="windows and dt"):
            window_trends(rows[5:], steps[5:], windows[:3], state=head)
        with pytest.raises(ValueError, match="windows and dt"):
            window_trends(rows[5:], steps[5:], windows, dt=2.0, state=head)
        with pytest.raises(ValueError, match="does not lie after"):
            window_trends(rows[4:], steps[4:], windows, state=head)
        with pytest.raises(ValueError, match="other rows"):
            window_trends(rows[5:, :N - 1], steps[5:], windows, state=head)
        with pytest.raises(ValueError, match="2\\^53"):
            window_trends(rows[:2], [0, 2 ** 27], ((0, 2 ** 31 - 1),))
