"""Running means and trends on the GPU: running_mean_kernel and window_trend_kernel through the C ABI against the independent
reference (tests/smooth_reference.py) at every size where they take another path — fp64 bits, compared exactly, the guards
around the outputs included —, row splits at every cut, NaN containment, the slope, and EnsembleEngine.running_mean /
window_trends end to end on a run with internal variability."""
import numpy as np
import pytest
import torch

import smooth_reference as ref
from fiveeqscm_amd import _capi

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
WINDOWS = [1, 2, 3, 7, 20, 32]


class GpuBackend:
    """smooth_reference.check_mean / check_trend on device buffers through the library."""

    def __init__(self):
        self.lib = _capi.load()

    def put(self, a):
        t = torch.from_numpy(a).cuda()
        assert t.data_ptr() % 16 == 0
        return t

    def addr(self, h):
        return h.data_ptr()

    def get(self, h):
        torch.cuda.synchronize()
        return h.cpu().numpy()

    def check(self, rc):
        _capi.check(self.lib, rc)


def _shape(dtype):
    lib = _capi.load()
    itemsize = np.dtype(dtype).itemsize
    return lib.fiveeq_smooth_tile(itemsize), 16 // itemsize, (lib.fiveeq_smooth_unroll(1), lib.fiveeq_smooth_unroll(0))


def _bits(t):
    return t.contiguous().view(torch.int64)


def test_the_inputs_tell_the_excluded_implementations_apart():
    """A sliding add / subtract update and a multiply by the reciprocal each differ from the definition in at least one bit on
    the inputs below, in members without NaN or infinity, at the windows that are no power of two."""
    for dtype in DTYPES:
        tile, _, _ = _shape(dtype)
        x = ref.make_rows(2 * 20 + 3, tile + 1, dtype, 5)
        ok = ref.finite_members(x)
        for window in (3, 7, 20):
            want = ref.running_mean(x, window)[:, ok]
            assert (ref.bits(ref.sliding_mean(x, window)[:, ok]) != ref.bits(want)).any(), (dtype, window, "sliding")
            assert (ref.bits(ref.reciprocal_mean(x, window)[:, ok]) != ref.bits(want)).any(), (dtype, window, "reciprocal")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("window", WINDOWS)
def test_running_mean_kernel_equals_the_reference(dtype, window):
    """n_members at the edges of a lane and of a workgroup's tile x n_rows at the edges of the window and of both row loops, each
    in two layouts: 16-byte rows with guard columns (the 16-byte path, the ragged members in a launch of their own), and rows
    one element off, ld = n + 5, three scenarios further apart than their rows (the element path).  Guard rows before and after
    out, guard columns and the gaps between scenario blocks must come back untouched."""
    gpu = GpuBackend()
    tile, lane, unrolls = _shape(dtype)
    sizes = ref.sizes_of(tile, lane)
    assert len(sizes) >= 7 and sizes[-1] == 2 * tile + 3
    for i, n in enumerate(sizes):
        for k in ref.rows_of(window, unrolls):
            for j, (ld, off, gap, S) in enumerate(ref.layouts_of(n, np.dtype(dtype).itemsize)):
                xs = [ref.make_rows(k, n, dtype, 1000 * window + 100 * i + 10 * j + s + k) for s in range(S)]
                ref.check_mean(gpu, xs, window, ld=ld, off=off, gap=gap)


@pytest.mark.parametrize("dtype", DTYPES)
def test_running_mean_row_splits_at_every_cut(dtype):
    """Rows [0, cut) in one call, rows [cut, n) with the rows before them as the tail in a second: the bits of one call, in both
    layouts; then the same through smooth.running_mean(state=)."""
    from fiveeqscm_amd.smooth import running_mean
    gpu = GpuBackend()
    tile, lane, _ = _shape(dtype)
    n, window, k = tile + lane + 1, 7, 2 * 7 + 3
    x = ref.make_rows(k, n, dtype, 77)
    want = ref.running_mean(x, window)
    for ld, off, gap, S in ref.layouts_of(n, np.dtype(dtype).itemsize):
        for cut in range(k + 1):
            ref.check_mean(gpu, [x] * S, window, ld=ld, off=off, gap=gap, cuts=(cut,), want=[want] * S)
    ref.check_mean(gpu, [x], window, ld=n, off=0, gap=0, cuts=tuple(range(1, k)), want=[want])          # row by row
    rows, steps = torch.from_numpy(x).cuda(), ref.steps_of(k, first=4, stride=3)
    one = running_mean(rows, steps, window)
    assert torch.equal(_bits(one.rows), _bits(torch.from_numpy(want).cuda()))
    for cut in range(k + 1):
        head = running_mean(rows[:cut], steps[:cut], window)
        rest = running_mean(rows[cut:], steps[cut:], window, state=head)
        assert torch.equal(_bits(torch.cat([head.rows, rest.rows])), _bits(one.rows)), cut
        assert np.concatenate([head.steps, rest.steps]).tolist() == one.steps.tolist() == (steps[3:3 + k - window + 1]).tolist()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_row_touches_exactly_its_window_of_outputs(dtype):
    from fiveeqscm_amd.smooth import running_mean
    tile, lane, _ = _shape(dtype)
    n = tile + 3
    for window in (1, 3, 20):
        k, r = 3 * window + 2, window + 1
        rng = np.random.default_rng(window)
        x = (1.0 + rng.random((k, n))).astype(dtype)
        hit = [0, lane - 1, lane, tile - 1, tile, n - 1]
        x[r, hit] = np.nan
        got = running_mean(torch.from_numpy(x).cuda(), ref.steps_of(k), window).rows.cpu().numpy()
        nan = np.isnan(got)
        assert nan.sum(axis=0)[hit].tolist() == [window] * len(hit)
        assert nan[r - window + 1:r + 1][:, hit].all()
        assert nan.sum() == window * len(hit), "a neighbour turned NaN"
        assert np.array_equal(ref.bits(got), ref.bits(ref.running_mean(x, window)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_window_one_returns_the_rows_widened(dtype):
    from fiveeqscm_amd.smooth import running_mean
    tile, _, _ = _shape(dtype)
    x = torch.from_numpy(ref.make_rows(11, tile + 5, dtype, 9)).cuda()
    assert torch.equal(_bits(running_mean(x, ref.steps_of(11), 1).rows), _bits(x.double()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_window_trend_kernel_equals_the_reference(dtype):
    """sx and stx to the bit: the sizes and layouts of the running mean x the edges of both row loops x 0, 1 and 4 windows
    (one empty, overlapping ones, boundaries between stored steps); first_call over a poisoned state; rows split at 1, k // 2
    and k - 1."""
    gpu = GpuBackend()
    tile, lane, unrolls = _shape(dtype)
    rows_n = sorted({0, 1, 2 * max(unrolls) + 1} | {u + d for u in unrolls for d in (-1, 0, 1)})
    for i, n in enumerate(ref.sizes_of(tile, lane)):
        for k in rows_n:
            steps = ref.steps_of(k, first=3, stride=2)
            for windows in ((), ((0, 100),), ((6, 20), (20, 20), (0, 5), (4, 36))):
                for j, (ld, off, gap, S) in enumerate(ref.layouts_of(n, np.dtype(dtype).itemsize)):
                    xs = [ref.make_rows(k, n, dtype, 100 * i + 10 * j + s + k) for s in range(S)]
                    ref.check_trend(gpu, xs, steps, windows, ld=ld, off=off, gap=gap, poison=True)
                    if k > 2 and len(windows) == 4:
                        ref.check_trend(gpu, xs, steps, windows, ld=ld, off=off, gap=gap, cuts=(1, k // 2, k - 1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_window_trends_row_splits_and_slope(dtype):
    """first_call, then continuation, at every cut — through the C ABI and through smooth.window_trends(state=); the slope
    against NumPy's evaluation of the same expression on the downloaded sums.  The products and subtractions are correctly
    rounded on both sides, and so, measured on the MI355X (0 ulp over every value of both precisions), are the two divisions:
    the comparison is held to the bit."""
    from fiveeqscm_amd.smooth import window_trends
    gpu = GpuBackend()
    tile, lane, _ = _shape(dtype)
    n, k = tile + lane + 1, 19
    x = ref.make_rows(k, n, dtype, 21)
    steps = ref.steps_of(k, first=3, stride=2)
    windows = ((5, 20), (20, 20), (39, 60), (0, 100))
    for ld, off, gap, S in ref.layouts_of(n, np.dtype(dtype).itemsize):
        for cut in range(k + 1):
            ref.check_trend(gpu, [x] * S, steps, windows, ld=ld, off=off, gap=gap, cuts=(cut,))
    rows = torch.from_numpy(x).cuda()
    sx, stx = ref.trend_sums(x, steps, windows)
    one = window_trends(rows, steps, windows, dt=0.5)
    assert np.array_equal(ref.bits(one.sx.cpu().numpy()), ref.bits(sx)) and np.array_equal(ref.bits(one.stx.cpu().numpy()), ref.bits(stx))
    for cut in range(k + 1):
        head = window_trends(rows[:cut], steps[:cut], windows, dt=0.5)
        both = window_trends(rows[cut:], steps[cut:], windows, dt=0.5, state=head)
        for name in ("sx", "stx", "mean", "slope"):
            assert torch.equal(_bits(getattr(both, name)), _bits(getattr(one, name))), (cut, name)
    got = one.slope.cpu().numpy()
    want = ref.slope_of(one.sx.cpu().numpy(), one.stx.cpu().numpy(), steps, windows, 0.5)
    assert one.count == (8, 0, 1, k) and np.isnan(got[1]).all() and np.isnan(got[2]).all()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = np.isfinite(want)
    assert np.array_equal(got[~ok & ~np.isnan(want)], want[~ok & ~np.isnan(want)])                    # infinities, with their sign
    ulp = np.abs(ref.bits(got[ok]) - ref.bits(want[ok]))
    print(f"slope vs NumPy, {np.dtype(dtype).name}: max distance {int(ulp.max())} ulp over {int(ok.sum())} values")
    assert ulp.max() == 0


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_engine_running_mean_and_window_trends_end_to_end(dtype):
    """A 64-member, 60-step CO2 run with AR(1) internal variability: the warming-level crossing and the peak of the 10-row
    running mean, and the trend over steps 20..49, equal what the reference computes from the downloaded T rows."""
    from fiveeqscm_amd import params as prm
    from fiveeqscm_amd.emissions import rcp_like_emissions
    from fiveeqscm_amd.engine import EnsembleEngine
    from fiveeqscm_amd.forcing import ar1_noise_rows
    from fiveeqscm_amd.metrics import trajectory_metrics
    from metrics_reference import reference as metrics_reference
    N, n_steps = 64, 60
    p = prm.sample_ensemble_shard(prm.default_params("co2"), N)
    noise = ar1_noise_rows(N, n_steps, sigma=0.4, phi=0.6, seed=11, dtype=dtype, device="cuda:0")
    eng = EnsembleEngine(p, N, rcp_like_emissions(n_steps, 1), dtype=dtype, member_forcing=noise, device="cuda:0")
    eng.run()
    torch.cuda.synchronize()
    T = eng.T.cpu().numpy()
    assert T.shape == (n_steps, N) and (np.diff(T, axis=0) < 0).any(), "the rows are not noisy"
    want = ref.running_mean(T, 10)
    sm = eng.running_mean(10)
    assert torch.equal(_bits(sm.rows), _bits(torch.from_numpy(want).cuda()))
    assert sm.steps.tolist() == list(range(5, 5 + n_steps - 9)) and sm.window == 10 and sm.align == "centre"
    level = float(np.median(want.max(axis=0)))                 # half the members' means reach it, the others never do
    m = trajectory_metrics(sm.rows, sm.steps, levels=(level,))
    mw = metrics_reference(want, sm.steps, (level,))
    assert np.array_equal(m.first.cpu().numpy(), mw["first"]) and np.array_equal(ref.bits(m.peak.cpu().numpy()), ref.bits(mw["peak"]))
    assert (mw["first"] >= 0).any() and (mw["first"] < 0).any()
    raw = metrics_reference(T, eng.out_steps, (level,))
    assert (raw["first"] != mw["first"]).any(), "single rows date the level as the mean does: the case shows nothing"
    tail = eng.running_mean(10, align="trailing", rows=slice(20, None))
    assert torch.equal(_bits(tail.rows), _bits(sm.rows[20:])) and tail.steps.tolist() == list(range(29, 60))
    tr = eng.window_trends(((20, 50),))
    sx, stx = ref.trend_sums(T, eng.out_steps, ((20, 50),))
    assert tr.count == (30,)
    assert np.array_equal(ref.bits(tr.sx.cpu().numpy()), ref.bits(sx)) and np.array_equal(ref.bits(tr.stx.cpu().numpy()), ref.bits(stx))
    slope = ref.slope_of(sx, stx, eng.out_steps, ((20, 50),), eng.dt)
    assert np.array_equal(ref.bits(tr.slope.cpu().numpy()), ref.bits(slope))
    # the slope is the least-squares fit: NumPy's polyfit over the same rows agrees to rounding
    fit = np.polyfit(np.arange(20, 50) * eng.dt, T[20:50].astype(np.float64), 1)[0]
    assert np.allclose(tr.slope.cpu().numpy()[0], fit, rtol=1e-9, atol=1e-12)
    c = eng.running_mean(5, gas=0)
    assert torch.equal(_bits(c.rows), _bits(torch.from_numpy(ref.running_mean(eng.C[:, 0].cpu().numpy(), 5)).cuda()))
