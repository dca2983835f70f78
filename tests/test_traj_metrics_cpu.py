"""Trajectory metrics without a GPU: the C ABI (exported, bound, additive, validated on the host), the NumPy twin of the
kernel against the independent reference (tests/metrics_reference.py) on the GPU test's case table, the host side of
metrics.trajectory_metrics under host_passes(), and exceedance / crossing_summary over gloo."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fiveeqscm_amd import _capi, _metrics_host, _wsummary_host
from fiveeqscm_amd.distributed import shard_bounds
from fiveeqscm_amd.metrics import TrajectoryMetrics, crossing_summary, exceedance, trajectory_metrics
from metrics_reference import assert_equal, case_data, case_table, lay_out, ld_of, make_rows, reference, spec_of, steps_of
from weighted_reference import weighted_row

NEW = ["fiveeq_traj_metrics_f64", "fiveeq_traj_metrics_f32", "fiveeq_max_levels", "fiveeq_max_windows", "fiveeq_metrics_tile",
       "fiveeq_metrics_unroll"]
U = _capi.METRICS_UNROLL


def test_new_symbols_are_exported_and_the_abi_is_additive():
    lib = _capi.load()
    for name in NEW + ["fiveeq_max_scenarios"]:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    assert lib.fiveeq_abi_version() == _capi.ABI_VERSION == 13
    assert lib.fiveeq_sizeof_model() == ctypes.sizeof(_capi.Model) == 448
    assert lib.fiveeq_max_levels() == _capi.MAX_LEVELS == 8 and lib.fiveeq_max_windows() == _capi.MAX_WINDOWS == 4
    assert any(p.endswith("fiveeq_metrics.hpp") for p in _capi.SOURCES)
    names = [os.path.basename(p) for p in _capi.SOURCES]
    assert names.index("fiveeq_metrics.hpp") == names.index("fiveeq_resample.hpp") + 1
    # the kernel's shape comes from the library: the tests pick their edge sizes from these
    assert (lib.fiveeq_metrics_tile(8), lib.fiveeq_metrics_tile(4), lib.fiveeq_metrics_tile(2)) == (_capi.METRICS_TILE_F64, _capi.METRICS_TILE_F32, 0)
    assert (lib.fiveeq_metrics_unroll(1), lib.fiveeq_metrics_unroll(0)) == (_capi.METRICS_UNROLL, _capi.METRICS_UNROLL_NARROW)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_the_entry_points_validate_on_the_host(sfx):
    """Every call returns on the host with an error code: the fake pointers are never dereferenced, nothing is launched."""
    lib = _capi.load()
    fn = getattr(lib, f"fiveeq_traj_metrics_{sfx}")
    w = 8 if sfx == "f64" else 4
    p = ctypes.c_void_p(0x1000)
    lv = (ctypes.c_double * 8)(*[0.5 * i for i in range(8)])
    wn = (ctypes.c_int32 * 8)(0, 5, 5, 5, 2, 9, 0, 1)
    E = _capi.E_INVALID
    err = lambda: lib.fiveeq_last_error().decode()   # noqa: E731

    def call(n_scen=1, n_rows=4, n=8, ld=8, rows=p, scen_stride=32, steps=p, L=2, levels=lv, W=2, windows=wn, fmet=p, imet=p,
             first=1):
        return fn(n_scen, n_rows, n, ld, rows, scen_stride, steps, L, ctypes.cast(levels, ctypes.c_void_p) if levels else None, W,
                  ctypes.cast(windows, ctypes.c_void_p) if windows else None, fmet, imet, first, None)

    for kw, needle in [(dict(rows=None), "rows"), (dict(steps=None), "steps"), (dict(fmet=None), "fmet"), (dict(imet=None), "imet"),
                       (dict(levels=None), "levels"), (dict(windows=None), "windows")]:
        assert call(**kw) == E and needle in err() and "NULL" in err(), kw
    odd = lambda k: ctypes.c_void_p(0x1000 + k)   # noqa: E731
    for kw, needle in [(dict(rows=odd(w // 2)), "rows"), (dict(steps=odd(2)), "steps"), (dict(fmet=odd(4)), "fmet"),
                       (dict(imet=odd(2)), "imet")]:
        assert call(**kw) == E and needle in err() and "aligned" in err(), kw
    for n_scen in (0, -1, lib.fiveeq_max_scenarios() + 1):
        assert call(n_scen=n_scen) == E and "n_scen" in err()
    assert call(n=0) == E and "n_members" in err()
    assert call(n=2 ** 31, ld=2 ** 31) == E and "n_members" in err()
    assert call(n=8, ld=7) == E and "ld=" in err()
    assert call(n_rows=-1) == E and "n_rows" in err()
    assert call(n_scen=2, scen_stride=31) == E and "scen_stride" in err()
    for L in (-1, 9):
        assert call(L=L) == E and "n_levels" in err()
    for W in (-1, 5):
        assert call(W=W) == E and "n_windows" in err()
    nan_lv = (ctypes.c_double * 8)(1.0, float("nan"), 0, 0, 0, 0, 0, 0)
    assert call(levels=nan_lv) == E and "levels[1]" in err() and "NaN" in err()
    assert call(windows=(ctypes.c_int32 * 8)(0, 5, 6, 5, 0, 0, 0, 0)) == E and "windows[1]" in err()
    assert call(windows=(ctypes.c_int32 * 8)(-1, 5, 0, 0, 0, 0, 0, 0), W=1) == E and "windows[0]" in err()
    # n_rows == 0 without first_call: validated, then nothing to do — rows / steps may be NULL
    assert call(n_rows=0, rows=None, steps=None, first=0) == _capi.OK
    assert call(n_rows=0, rows=None, steps=None, first=0, fmet=None) == E
    assert call(n_rows=0, L=0, levels=None, W=0, windows=None, first=0) == _capi.OK


# ---- the NumPy twin of the kernel against the reference, on THE CASE TABLE the GPU test holds the kernel to -------------------
F_SENT, I_SENT = -777.25, -777


def _twin(xs, steps, levels, windows, *, ld, off, gap, splits=()):
    """The twin through its pointer signature on the GPU test's layout (tests/metrics_reference.py lay_out): row base `off`
    elements off, rows ld apart, scenario blocks k * ld + gap apart; sentinel padding and a guard word in the state blocks.
    Returns one result dict per scenario."""
    S, (K, n) = len(xs), xs[0].shape
    dtype = xs[0].dtype.type
    host, stride = lay_out(xs, ld, off, gap)
    L, W = len(levels), len(windows)
    fm = np.full(S * (1 + W) * ld + 1, F_SENT)
    im = np.full(S * (2 + 2 * L) * ld + 1, I_SENT, dtype=np.int32)
    st = np.asarray(steps, dtype=np.int32)
    lv = np.asarray(levels, dtype=np.float64).reshape(-1)
    wn = np.asarray(windows, dtype=np.int32).reshape(-1)
    fn = getattr(_metrics_host.MetricsPasses(), "fiveeq_traj_metrics_f64" if dtype == np.float64 else "fiveeq_traj_metrics_f32")
    cuts = [0, *splits, K]
    for i in range(len(cuts) - 1):
        a, b = cuts[i], cuts[i + 1]
        assert fn(S, b - a, n, ld, host.ctypes.data + (off + a * ld) * host.itemsize, stride, st.ctypes.data + 4 * a, L,
                  lv.ctypes.data if L else 0, W, wn.ctypes.data if W else 0, fm.ctypes.data, im.ctypes.data, 1 if i == 0 else 0,
                  None) == 0
    assert fm[-1] == F_SENT and im[-1] == I_SENT
    fh, ih = fm[:-1].reshape(S, 1 + W, ld), im[:-1].reshape(S, 2 + 2 * L, ld)
    assert np.all(fh[:, :, n:] == F_SENT) and np.all(ih[:, :, n:] == I_SENT)
    return [{"peak": fh[s, 0, :n], "t_peak": ih[s, 0, :n], "n_nan": ih[s, 1, :n], "first": ih[s, 2:2 + L, :n],
             "n_above": ih[s, 2 + L:, :n], "wsum": fh[s, 1:, :n]} for s in range(S)]


@pytest.mark.parametrize("dtype,tile", [(np.float64, _capi.METRICS_TILE_F64), (np.float32, _capi.METRICS_TILE_F32)])
def test_the_host_twin_equals_the_reference_on_the_case_table(dtype, tile):
    """Every case of the table, in its layout; and every case with more than two rows again with the rows split at 1, k // 2
    and k - 1 (first_call = 1, then 0)."""
    itemsize = np.dtype(dtype).itemsize
    table = case_table(tile, _capi.METRICS_UNROLL, _capi.METRICS_UNROLL_NARROW)
    assert {c["k"] for c in table} >= {1, U - 1, U, U + 1, 2 * U + 1} and {(c["L"], c["W"]) for c in table} == {(0, 0), (1, 0), (0, 1), (8, 4)}
    assert {c["n"] for c in table} == {1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 3}
    assert {(c["off"], c["S"]) for c in table} == {(0, 1), (1, 3), (0, 3)}
    for c in table:
        data = [case_data(c["k"], c["n"], dtype, seed, c["L"], c["W"]) for seed in c["seeds"]]
        _, steps, levels, windows, _ = data[0]
        kw = dict(ld=ld_of(c, itemsize), off=c["off"], gap=2 * (16 // itemsize))
        k = c["k"]
        for splits in ((),) + (((1, k // 2, k - 1),) if k > 2 else ()):
            got = _twin([d[0] for d in data], steps, levels, windows, splits=splits, **kw)
            for s, d in enumerate(data):
                assert_equal(got[s], d[4], (c, s, splits))


# ---- metrics.trajectory_metrics on host tensors, through the twin ------------------------------------------------------------
def _as_dict(m):
    return {k: getattr(m, k).numpy() for k in ("peak", "t_peak", "n_nan", "first", "n_above", "wsum")}


def test_trajectory_metrics_host_side():
    K, N = 19, 130
    steps = steps_of(K)
    levels, windows = spec_of(3, 4, steps)
    x = make_rows(K, N, np.float64, seed=5)
    rows = torch.from_numpy(x)
    with pytest.raises(TypeError, match="no CPU fallback"):
        trajectory_metrics(rows, steps, levels, windows)            # host rows outside the context
    with _metrics_host.host_passes():
        one = trajectory_metrics(rows, steps, levels, windows)
        want = reference(x, steps, levels, windows)
        assert_equal(_as_dict(one), want)
        assert isinstance(one, TrajectoryMetrics) and one.levels == tuple(levels) and one.windows == tuple(windows)
        assert one.steps.tolist() == steps.tolist()
        # window_mean = wsum / stored steps inside; the empty window: 0 rows, sum 0, mean NaN
        counts = [int(((steps >= a) & (steps < b)).sum()) for a, b in windows]
        assert counts[1] == 0 and min(counts[0], counts[2], counts[3]) > 0
        live = one.n_nan.numpy() == 0
        assert np.all(one.wsum.numpy()[1] == 0.0) and np.all(np.isnan(one.window_mean.numpy()[1]))
        for w in (0, 2, 3):
            assert np.array_equal(one.window_mean.numpy()[w][live], (want["wsum"][w] / counts[w])[live])
        # continuation in three blocks == one call, bit for bit; window counts accumulate over the blocks
        st = None
        for a, b in ((0, 1), (1, K // 2), (K // 2, K)):
            st = trajectory_metrics(rows[a:b], steps[a:b], levels, windows, state=st)
        assert_equal(_as_dict(st), want)
        assert st.steps.tolist() == steps.tolist()
        assert np.array_equal(st.window_mean.numpy().view(np.uint64), one.window_mean.numpy().view(np.uint64))
        # a column-sliced view (ld > N) and the scenario axis with a block stride larger than n_rows * ld
        wide = torch.from_numpy(np.ascontiguousarray(np.stack([np.pad(x, ((0, 3), (0, 9))), np.pad(x[::-1], ((0, 3), (0, 9)))])))
        two = trajectory_metrics(wide[:, :K, :N], steps, levels, windows)
        assert two.peak.shape == (2, N) and two.first.shape == (2, 3, N) and two.wsum.shape == (2, 4, N)
        assert_equal({k: v[0] for k, v in _as_dict(two).items()}, want)
        assert_equal({k: v[1] for k, v in _as_dict(two).items()}, reference(x[::-1], steps, levels, windows))
        # refusals
        head = trajectory_metrics(rows[:5], steps[:5], levels, windows)
        with pytest.raises(ValueError, match="levels and windows"):
            trajectory_metrics(rows[5:], steps[5:], levels[:2], windows, state=head)
        with pytest.raises(ValueError, match="levels and windows"):
            trajectory_metrics(rows[5:], steps[5:], levels, windows[:3], state=head)
        with pytest.raises(ValueError, match="does not lie after"):
            trajectory_metrics(rows[4:], steps[4:], levels, windows, state=head)
        with pytest.raises(ValueError, match="strictly increasing"):
            trajectory_metrics(rows[:3], [3, 9, 9], levels, windows)
        with pytest.raises(ValueError, match="at most 8"):
            trajectory_metrics(rows, steps, [0.1 * i for i in range(9)])
        with pytest.raises(ValueError, match="windows"):
            trajectory_metrics(rows, steps, (), [(5, 4)])
        with pytest.raises(ValueError, match="NaN"):
            trajectory_metrics(rows, steps, [float("nan")])
        # no rows: the initial state
        none = trajectory_metrics(rows[:0], steps[:0], levels, windows)
        assert np.all(none.peak.numpy() == -np.inf) and np.all(none.t_peak.numpy() == -1) and np.all(none.first.numpy() == -1)
        assert_equal(_as_dict(trajectory_metrics(rows, steps, levels, windows, state=none)), want)


# ---- exceedance and crossing_summary: world 1 == world 2 over gloo ---------------------------------------------------------
PCT = (5.0, 50.0, 95.0)
N_GLOO = 1003


def _gloo_case():
    rng = np.random.default_rng(11)
    first = np.full((3, N_GLOO), -1, dtype=np.int32)
    hit = rng.random(N_GLOO) < 0.6
    first[0, hit] = rng.integers(0, 80, size=int(hit.sum()))
    rare = rng.random(N_GLOO) < 0.02
    first[1, rare] = rng.integers(40, 80, size=int(rare.sum()))      # row 2: a level nobody crosses
    weights = rng.integers(0, 1 << 20, size=N_GLOO).astype(np.int64)
    weights[rng.random(N_GLOO) < 0.3] = 0
    zeroing = weights.copy()
    zeroing[first[1] >= 0] = 0                                        # weights that zero out every crosser of level 1
    years = 1850.0 + 0.5 * np.arange(80)
    return first, weights, zeroing, years


def _bounds(case, world):
    if case == "balanced":
        return [shard_bounds(N_GLOO, r, world) for r in range(world)]
    return [(0, 0), (0, N_GLOO)] + [(N_GLOO, N_GLOO)] * (world - 2)   # rank 0 holds nothing


def _install_host_summaries():
    """distributed.py's summaries on host tensors: the unweighted passes of oracle/summary_passes.py and the weighted ones of
    _wsummary_host.py behind the one switch they share."""
    from fiveeqscm_amd import distributed
    from oracle.summary_passes import SummaryPasses

    class Both:
        plain, weighted = SummaryPasses(), _wsummary_host.WeightedPasses()

        def __getattr__(self, name):
            return getattr(self.weighted if name.startswith("fiveeq_w") else self.plain, name)

    passes = Both()
    distributed._lib_and_stream = lambda rows: (passes, _wsummary_host._Check, ctypes, None)
    distributed._passes_apply = lambda rows: rows.dtype in (torch.float32, torch.float64)


def _evaluate(lo, hi):
    first, weights, zeroing, years = _gloo_case()
    f, w, z = torch.from_numpy(first[:, lo:hi].copy()), torch.from_numpy(weights[lo:hi].copy()), torch.from_numpy(zeroing[lo:hi].copy())
    tolist = lambda s: None if s["percentiles"] is None else s["percentiles"].numpy().view(np.uint64).tolist()   # noqa: E731
    out = {"ex": exceedance(f), "exw": exceedance(f, weights=w)}
    for name, row, kw in (("c0", 0, {}), ("c0w", 0, dict(weights=w)), ("c1w", 1, dict(weights=w)), ("c2", 2, {}),
                          ("c2w", 2, dict(weights=w)), ("c1z", 1, dict(weights=z)),
                          ("c0a", 0, dict(accepted=torch.from_numpy((weights[lo:hi] > 0))))):
        s = crossing_summary(f[row], years, PCT, **kw)
        out[name] = (int(s["crossed"]), float(s["count"][0]), tolist(s))
    return out


def _worker(rank, world, port, case, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _install_host_summaries()
        lo, hi = _bounds(case, world)[rank]
        q.put((rank, _evaluate(lo, hi)))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _spawn(target, world, *args):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, *args, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return dict(results)


@pytest.fixture
def host_summaries():
    from fiveeqscm_amd import distributed
    saved = distributed._lib_and_stream, distributed._passes_apply
    _install_host_summaries()
    yield
    distributed._lib_and_stream, distributed._passes_apply = saved


@pytest.mark.parametrize("case", ["balanced", "empty_shard"])
def test_exceedance_and_crossing_summary_world_1_equals_world_2(case, host_summaries):
    first, weights, zeroing, years = _gloo_case()
    one = _evaluate(0, N_GLOO)
    # world 1 against plain NumPy / the weighted reference
    assert one["ex"] == [(int((first[l] >= 0).sum()), N_GLOO) for l in range(3)]
    assert one["exw"] == [(int(weights[first[l] >= 0].sum()), int(weights.sum())) for l in range(3)]
    yr0 = years[first[0][first[0] >= 0]]
    assert one["c0"][:2] == (int((first[0] >= 0).sum()), float(yr0.size))
    assert one["c0"][2] == [np.percentile(yr0, PCT).view(np.uint64).tolist()]
    acc = (first[0] >= 0) & (weights > 0)
    assert one["c0a"][2] == [np.percentile(years[first[0][acc]], PCT).view(np.uint64).tolist()]
    for name, row in (("c0w", 0), ("c1w", 1)):
        w_eff = weights * (first[row] >= 0)
        ref = weighted_row(years[np.maximum(first[row], 0)], w_eff, PCT)
        assert one[name][0] == ref["weight_sum"] and one[name][1] == ref["count"]
        assert one[name][2] == [ref["percentiles"].view(np.uint64).tolist()]
    # a level nobody crosses, and weights that zero out every crosser: crossed == 0, count 0, NaN percentiles, no raise
    for name in ("c2", "c2w", "c1z"):
        crossed, count, pct = one[name]
        assert crossed == 0 and count == 0.0 and np.all(np.isnan(np.array(pct, dtype=np.uint64).view(np.float64)))
    assert one["ex"][2] == (0, N_GLOO)
    # world 2: identical integers on every rank, identical percentiles on the root, None elsewhere
    got = _spawn(_worker, 2, case)
    for rank in (0, 1):
        for key, want in one.items():
            if key.startswith("ex"):
                assert got[rank][key] == want, (rank, key)
            else:
                assert got[rank][key][:2] == want[:2], (rank, key)
                assert got[rank][key][2] == (want[2] if rank == 0 else None), (rank, key)


def test_crossing_summary_keeps_its_keys_when_nobody_crosses(host_summaries):
    """The empty case returns the key set (and host tensors) of the summary that the non-empty case comes from."""
    first, weights, _, years = _gloo_case()
    w = torch.from_numpy(weights)
    for kw in ({}, dict(weights=w)):
        full = crossing_summary(torch.from_numpy(first[0]), years, PCT, **kw)
        empty = crossing_summary(torch.from_numpy(first[2]), years, PCT, **kw)
        assert set(empty) == set(full), (sorted(empty), sorted(full))
        for key, v in full.items():
            assert type(empty[key]) is type(v), key
            if isinstance(v, torch.Tensor):
                assert empty[key].shape == v.shape and empty[key].dtype == v.dtype and empty[key].device == v.device, key
