"""Trajectory metrics on the GPU: traj_metrics_kernel through the C ABI against the independent reference
(tests/metrics_reference.py) at every size where it takes another path — integers and fp64 bits, compared exactly —, the guards
around the state blocks, row splits, and EnsembleEngine.trajectory_metrics end to end."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

from fiveeqscm_amd import _capi
from metrics_reference import assert_equal, case_data, case_table, lay_out, ld_of, reference, sizes_of
from weighted_reference import weighted_row

pytestmark = pytest.mark.gpu

U = _capi.METRICS_UNROLL
TILE = {np.float64: _capi.METRICS_TILE_F64, np.float32: _capi.METRICS_TILE_F32}
F_SENT, I_SENT = -777.25, -777


def _run(xs, steps, levels, windows, *, ld, off, gap, splits=(), poison=False):
    """xs: one [n_rows, n] array per scenario.  Lays them out at element offset `off` of a 16-byte aligned buffer, rows ld
    apart, scenario blocks n_rows * ld + gap apart; state blocks with sentinel padding and a guard word.  Returns per scenario
    the result dict."""
    lib = _capi.load()
    S, (K, n) = len(xs), xs[0].shape
    dtype = xs[0].dtype.type
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    host, stride = lay_out(xs, ld, off, gap)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0 and buf.dtype == tdt
    L, W = len(levels), len(windows)
    fm = torch.full((S * (1 + W) * ld + 1,), float("nan") if poison else F_SENT, dtype=torch.float64, device="cuda")
    im = torch.full((S * (2 + 2 * L) * ld + 1,), 12345 if poison else I_SENT, dtype=torch.int32, device="cuda")
    if poison:                                                 # a poisoned state, sentinels where nothing may be written
        fm[:-1].view(S, 1 + W, ld)[:, :, n:] = F_SENT
        im[:-1].view(S, 2 + 2 * L, ld)[:, :, n:] = I_SENT
        fm[-1], im[-1] = F_SENT, I_SENT
    st = torch.from_numpy(np.asarray(steps, dtype=np.int32)).cuda()
    c_lv = (ctypes.c_double * max(L, 1))(*levels)
    c_wn = (ctypes.c_int32 * max(2 * W, 1))(*[v for ab in windows for v in ab])
    fn = lib.fiveeq_traj_metrics_f64 if dtype == np.float64 else lib.fiveeq_traj_metrics_f32
    w = host.itemsize
    cuts = [0, *splits, K]
    for i in range(len(cuts) - 1):
        a, b = cuts[i], cuts[i + 1]
        _capi.check(lib, fn(S, b - a, n, ld, ctypes.c_void_p(buf.data_ptr() + (off + a * ld) * w), stride,
                            ctypes.c_void_p(st.data_ptr() + 4 * a), L, ctypes.cast(c_lv, ctypes.c_void_p), W,
                            ctypes.cast(c_wn, ctypes.c_void_p), ctypes.c_void_p(fm.data_ptr()), ctypes.c_void_p(im.data_ptr()),
                            1 if i == 0 else 0, None))
    torch.cuda.synchronize()
    fh, ih = fm.cpu().numpy(), im.cpu().numpy()
    assert fh[-1] == F_SENT and ih[-1] == I_SENT, "guard word after a state block"
    fh, ih = fh[:-1].reshape(S, 1 + W, ld), ih[:-1].reshape(S, 2 + 2 * L, ld)
    assert np.all(fh[:, :, n:] == F_SENT) and np.all(ih[:, :, n:] == I_SENT), "padding columns of the state blocks"
    return [{"peak": fh[s, 0, :n], "t_peak": ih[s, 0, :n], "n_nan": ih[s, 1, :n], "first": ih[s, 2:2 + L, :n],
             "n_above": ih[s, 2 + L:, :n], "wsum": fh[s, 1:, :n]} for s in range(S)]


def test_the_binding_holds_the_kernels_shape():
    lib = _capi.load()
    assert (lib.fiveeq_metrics_tile(8), lib.fiveeq_metrics_tile(4)) == (TILE[np.float64], TILE[np.float32])
    assert (lib.fiveeq_metrics_unroll(1), lib.fiveeq_metrics_unroll(0)) == (U, _capi.METRICS_UNROLL_NARROW)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("slot", range(8))
def test_kernel_equals_the_reference_on_the_case_table(dtype, slot):
    """THE CASE TABLE of tests/metrics_reference.py (the one the NumPy twin is held to on the CPU), one size per test: n_members
    at the tile edges x the row-loop edges x (L, W), aligned and one element off, ld = n and n + 5, one and three scenarios with
    a block stride larger than n_rows * ld.  Ties and exact hits: asserted by case_data for every case."""
    n = sizes_of(TILE[dtype])[slot]
    per16 = 16 // np.dtype(dtype).itemsize
    cases = [c for c in case_table(TILE[dtype], U, _capi.METRICS_UNROLL_NARROW) if c["n"] == n]
    assert len(cases) >= 16
    for c in cases:
        data = [case_data(c["k"], n, dtype, seed, c["L"], c["W"]) for seed in c["seeds"]]
        _, steps, levels, windows, _ = data[0]
        got = _run([d[0] for d in data], steps, levels, windows, ld=ld_of(c, np.dtype(dtype).itemsize), off=c["off"], gap=2 * per16)
        for s_, d in enumerate(data):
            assert_equal(got[s_], d[4], (c, s_))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_row_splits_and_a_poisoned_state(dtype):
    n, k = TILE[dtype] + 67, 2 * U + 1
    x, steps, levels, windows, want = case_data(k, n, dtype, 7, 8, 4)
    for off in (0, 1):
        for cut in (1, k // 2, k - 1):
            got = _run([x], steps, levels, windows, ld=n + 5 - off, off=off, gap=0, splits=(cut,))
            assert_equal(got[0], want, (off, cut))
        assert_equal(_run([x], steps, levels, windows, ld=n + 5 - off, off=off, gap=0, splits=(1, k // 2, k - 1))[0], want)
        assert_equal(_run([x], steps, levels, windows, ld=n + 5 - off, off=off, gap=0, poison=True)[0], want, "first_call ignores the state")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_wrapper_reads_a_wider_buffer_in_place_and_copies_a_strided_view(dtype):
    """metrics.trajectory_metrics on 3 rows of one 256-member tile plus three members: in a buffer N + 3 wide (read in place, the
    state blocks laid out with the buffer's ld), on every second column of a buffer 2 N wide (copied), and both under a scenario
    axis — every bit of the same call on a contiguous clone, which is the reference's."""
    from fiveeqscm_amd.metrics import trajectory_metrics
    n, k = 259, 3
    data = [case_data(k, n, dtype, seed, 2, 2) for seed in (11, 12)]
    _, steps, levels, windows, _ = data[0]
    names = ("peak", "t_peak", "n_nan", "first", "n_above", "wsum", "window_mean")
    bits = lambda t: t.view(torch.int64) if t.dtype == torch.float64 else t                  # noqa: E731  (NaN equal to NaN)

    def embed(rows, width, step):
        view = torch.full(tuple(rows.shape[:-1]) + (width,), float("nan"), dtype=rows.dtype, device=rows.device)[..., :step * n:step]
        view.copy_(rows)
        return view
    for rows in (torch.from_numpy(data[0][0].copy()).cuda(), torch.from_numpy(np.stack([d[0] for d in data])).cuda()):
        base = trajectory_metrics(rows.clone(), steps, levels, windows)
        for s_, d in enumerate(data[:1] if rows.dim() == 2 else data):
            pick = (lambda t: t) if rows.dim() == 2 else (lambda t: t[s_])                   # noqa: E731
            assert_equal({key: pick(getattr(base, key)).cpu().numpy() for key in d[4]}, d[4], (rows.dim(), s_))
        for width, step in ((n + 3, 1), (2 * n, 2)):
            view = embed(rows, width, step)
            assert view.stride(-1) == step and view.stride(-2) == width
            got = trajectory_metrics(view, steps, levels, windows)
            for name in names:
                assert torch.equal(bits(getattr(got, name)), bits(getattr(base, name))), (rows.dim(), width, name)
            assert got.peak.stride(-1) == 1 and (got.wsum.stride(-2) == width if step == 1 else got.wsum.stride(-2) == n)


def _sha(eng):
    return [hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest() for t in (eng.R, eng.S, eng.T, eng.C) if t is not None]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["scenarios", "observed_forced"])
def test_engine_trajectory_metrics_end_to_end(dtype, kind):
    from fiveeqscm_amd import params as prm
    from fiveeqscm_amd.distributed import gather_summary, gather_weighted_summary
    from fiveeqscm_amd.emissions import rcp_like_emissions
    from fiveeqscm_amd.engine import EnsembleEngine
    N, n_steps = 130, 60
    out_steps = [3, 4, 9, 10, 20, 21, 22, 35, 36, 40, 41, 50, 58, 59]
    base = prm.default_params("multigas")
    p = prm.sample_ensemble_shard(base, N)
    E = rcp_like_emissions(n_steps, 3)
    kw = {}
    if kind == "scenarios":
        E = np.stack([E, 0.6 * E])
    else:
        from fiveeqscm_amd.constrain import Observations
        from fiveeqscm_amd.forcing import ExternalForcings
        sc = prm.sample_forcing_scales(base, N, ranges=[(0.8, 1.2)] * 3 + [(0.3, 2.0), (0.5, 1.5)], seed=7)
        p["f_scale"], p["fx_scale"] = sc[:3], sc[3:]
        tt = np.arange(n_steps)
        kw["forcing"] = ExternalForcings(np.stack([-0.4 * tt / n_steps, np.where(tt % 17 == 5, -2.5, 0.0)], 1), ("aerosol", "volcanic"))
        years = 1850.0 + tt
        kw["observations"] = Observations.from_years(years, years[20:55], 0.01 * (years[20:55] - 1850.0), 0.1, baseline=(1850, 1869))
    eng = EnsembleEngine(p, N, E, dtype=dtype, output_steps=out_steps, device="cuda:0", **kw)
    eng.run()
    before = _sha(eng)
    T = eng.T.cpu().numpy()
    lo, hi = float(np.nanmin(T)), float(np.nanmax(T))
    levels = (lo + 0.5 * (hi - lo), float(T.reshape(-1, N)[5, 7]), hi + 1.0)       # a level inside, an exact hit, one nobody reaches
    windows = ((10, 41), (23, 35), (0, 60))
    m = eng.trajectory_metrics(levels=levels, windows=windows)
    torch.cuda.synchronize()
    assert _sha(eng) == before
    blocks = T if kind == "scenarios" else T[None]
    for s, block in enumerate(blocks):
        want = reference(block, eng.out_steps, levels, windows)
        pick = (lambda t: t[s]) if kind == "scenarios" else (lambda t: t)
        got = {k: pick(getattr(m, k)).cpu().numpy() for k in want}
        assert_equal(got, want, (kind, s))
        if kind == "scenarios":
            one = eng.trajectory_metrics(levels=levels, windows=windows, scenario=s)
            assert_equal({k: getattr(one, k).cpu().numpy() for k in want}, want, (kind, s, "one scenario"))
        peak = pick(m.peak).reshape(1, -1).contiguous()
        pct = gather_summary(peak, (5.0, 50.0, 95.0))["percentiles"].numpy()
        assert np.array_equal(pct[0], np.percentile(want["peak"], (5.0, 50.0, 95.0)))
        w = torch.arange(1, N + 1, dtype=torch.int64, device=peak.device) % 7
        ws = gather_weighted_summary(peak, w, (5.0, 50.0, 95.0))
        ref = weighted_row(want["peak"], w.cpu().numpy(), (5.0, 50.0, 95.0))
        assert np.array_equal(ws["percentiles"].numpy()[0], ref["percentiles"]) and ws["weight_sum"] == ref["weight_sum"]
    # continuation over the engine's own rows in two blocks == one call
    rows = eng.T
    from fiveeqscm_amd.metrics import trajectory_metrics
    head = trajectory_metrics(rows[..., :6, :], eng.out_steps[:6], levels, windows)
    both = trajectory_metrics(rows[..., 6:, :], eng.out_steps[6:], levels, windows, state=head)
    for k in ("peak", "t_peak", "n_nan", "first", "n_above", "wsum"):
        a, b = getattr(both, k).cpu().numpy(), getattr(m, k).cpu().numpy()
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), k


def test_engine_without_stored_rows_refuses():
    from fiveeqscm_amd import params as prm
    from fiveeqscm_amd.emissions import rcp_like_emissions
    from fiveeqscm_amd.engine import EnsembleEngine
    p = prm.sample_ensemble_shard(prm.default_params("multigas"), 64)
    eng = EnsembleEngine(p, 64, rcp_like_emissions(10, 3), output_steps=[], device="cuda:0")
    with pytest.raises(RuntimeError, match="no stored T rows"):
        eng.trajectory_metrics(levels=(1.5,))
