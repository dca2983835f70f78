"""The JOINT STATISTICS passes on the GPU: both kernels against the exact reference (tests/joint_reference.py) at the edges of
their chunks, lanes and row tiles, in fp64 and fp32, on both load paths; the same bits for every layout, repetition and tiling;
the flags; and EnsembleEngine.drivers end to end."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest
import torch

from fiveeqscm_amd import _capi, _joint_host
from joint_reference import WEIGHT_KINDS, W_ONE, Ref, case_data, case_table, finished_tol, tol

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NP = {torch.float64: np.float64, torch.float32: np.float32}


def _tile():
    lib = _capi.load()
    return [lib.fiveeq_joint_tile(k) for k in range(8)]


def _cases(dtype):
    t = _tile()
    return case_table(t[0], t[1], t[2], (t[3] if dtype == torch.float64 else t[4]) * t[7])


@functools.lru_cache(maxsize=None)
def _data(case, kind):
    """the data of a case and its exact results, computed once and shared by the dtypes and layouts"""
    n, n_x, n_y, n_bins = case
    x, y, w, piv, edges = case_data(n, n_x, n_y, n_bins, kind, _tile()[2])
    ref = Ref(x, y, w, piv, edges)
    return x, y, w, piv, edges, ref, ref.moments(), ref.cond(n_bins)


def _lay(a, dtype, ld, off):
    """rows [K, n] -> a device buffer holding them ld apart from element `off`; returns (buffer, pointer of the first row)"""
    K, n = a.shape
    buf = torch.full((off + K * ld + 8,), float("nan"), dtype=dtype, device=DEV)
    buf[off:off + K * ld].view(K, ld)[:, :n] = torch.from_numpy(a.astype(NP[dtype])).to(DEV)
    return buf, ctypes.c_void_p(buf.data_ptr() + off * buf.element_size())


def _run(x, y, w, piv, edges, n_bins, dtype, ld_pad=0, off=0):
    """both passes over one layout, poisoned workspace and outputs -> (co, margins, info, nanrows, sums, binw, xnan) host arrays"""
    lib = _capi.load()
    sfx = "f64" if dtype == torch.float64 else "f32"
    (n_x, n), n_y = x.shape, y.shape[0]
    ld = n + ld_pad
    xb, xp = _lay(x, dtype, ld, off)
    yb, yp = _lay(y, dtype, ld, off)
    wb = torch.zeros(n + 1 + off, dtype=torch.int64, device=DEV)
    wb[off:off + n] = torch.from_numpy(w).to(DEV)
    wp = ctypes.c_void_p(wb.data_ptr() + 8 * off)
    R = n_x + n_y
    chunks = int(lib.fiveeq_joint_chunks(n))
    p = lambda t, k=0: ctypes.c_void_p(t.data_ptr() + 8 * k)      # noqa: E731
    piv_d, ed_d = torch.from_numpy(piv).to(DEV), torch.from_numpy(np.ascontiguousarray(edges.reshape(-1))).to(DEV)
    work = torch.full((chunks * max(int(lib.fiveeq_joint_moments_words(n_x, n_y)), int(lib.fiveeq_cond_sums_words(n_x, n_y, n_bins))),),
                      float("nan"), dtype=torch.float64, device=DEV)
    oa = torch.full((n_x * n_y + 2 * R + 4 + R,), float("nan"), dtype=torch.float64, device=DEV)
    o = [0, n_x * n_y, n_x * n_y + 2 * R, n_x * n_y + 2 * R + 4]
    _capi.check(lib, getattr(lib, f"fiveeq_joint_moments_{sfx}")(n, n_x, ld, xp, n_y, ld, yp, wp, p(piv_d), p(work), p(oa, o[0]), p(oa, o[1]),
                                                                 p(oa, o[2]), p(oa, o[3]), None))
    work.fill_(float("nan"))
    ob = torch.full((n_x * n_bins * (n_y + 1) + n_x,), float("nan"), dtype=torch.float64, device=DEV)
    _capi.check(lib, getattr(lib, f"fiveeq_cond_sums_{sfx}")(n, n_x, ld, xp, n_y, ld, yp, wp, n_bins, p(ed_d) if n_bins > 1 else None,
                                                             p(piv_d, n_x), p(work), p(ob), p(ob, n_x * n_bins * n_y),
                                                             p(ob, n_x * n_bins * (n_y + 1)), None))
    torch.cuda.synchronize()
    a, b = oa.cpu().numpy(), ob.cpu().numpy()
    return (a[:o[1]].reshape(n_x, n_y), a[o[1]:o[2]].reshape(R, 2), a[o[2]:o[3]].view(np.int64), a[o[3]:].view(np.int64),
            b[:n_x * n_bins * n_y].reshape(n_x, n_bins, n_y), b[n_x * n_bins * n_y:n_x * n_bins * (n_y + 1)].view(np.int64).reshape(n_x, n_bins),
            b[n_x * n_bins * (n_y + 1):].view(np.int64))


def _same(a, b, what):
    for u, v, name in zip(a, b, ("co", "margins", "info", "nanrows", "sums", "binw", "xnan")):
        assert u.tobytes() == v.tobytes() or np.array_equal(u, v, equal_nan=True), (what, name)


def _twin(x, y, w, piv, edges, n_bins, dtype):
    """the NumPy twin over the same arrays: its integer outputs are the kernel's"""
    tw = _joint_host.JointPasses()
    npd = NP[dtype]
    xs, ys, ws = np.ascontiguousarray(x.astype(npd)), np.ascontiguousarray(y.astype(npd)), np.ascontiguousarray(w.astype(np.uint64))
    (n_x, n), n_y = x.shape, y.shape[0]
    R = n_x + n_y
    co, mar, info, nanr = np.zeros(n_x * n_y), np.zeros(2 * R), np.zeros(4, dtype=np.uint64), np.zeros(R, dtype=np.uint64)
    sums, binw, xnan = np.zeros(n_x * n_bins * n_y), np.zeros(n_x * n_bins, dtype=np.uint64), np.zeros(n_x, dtype=np.uint64)
    ed = np.ascontiguousarray(edges.reshape(-1))
    a = lambda t: t.ctypes.data      # noqa: E731
    getattr(tw, f"fiveeq_joint_moments_{'f64' if npd == np.float64 else 'f32'}")(n, n_x, n, a(xs), n_y, n, a(ys), a(ws), a(piv), 0, a(co), a(mar),
                                                                                 a(info), a(nanr), None)
    getattr(tw, f"fiveeq_cond_sums_{'f64' if npd == np.float64 else 'f32'}")(n, n_x, n, a(xs), n_y, n, a(ys), a(ws), n_bins, a(ed) if n_bins > 1 else 0,
                                                                             a(piv[n_x:]), 0, a(sums), a(binw), a(xnan), None)
    return info.astype(np.int64), nanr.astype(np.int64), binw.astype(np.int64).reshape(n_x, n_bins), xnan.astype(np.int64)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", WEIGHT_KINDS)
@pytest.mark.parametrize("k", range(10))
def test_both_passes_against_the_exact_reference_on_every_layout(k, kind, dtype):
    case = _cases(dtype)[k]
    n, n_x, n_y, n_bins = case
    x, y, w, piv, edges, ref, (co, co_abs, mar, mar_abs), (sums, sabs, cnt, binw, xnan) = _data(case, kind)
    first = None
    for ld_pad in (0, 3):
        for off in (0, 1):
            got = _run(x, y, w, piv, edges, n_bins, dtype, ld_pad, off)
            if first is None:
                first = got
                g_co, g_mar, g_info, g_nan, g_sums, g_binw, g_xnan = got
                assert np.all(np.abs(g_co - co) <= tol(ref.n, co_abs)), np.max(np.abs(g_co - co) - tol(ref.n, co_abs))
                assert np.all(np.abs(g_mar - mar) <= tol(ref.n, mar_abs))
                assert np.all(np.abs(g_sums - sums) <= tol(cnt[:, :, None], sabs))
                assert g_info.tolist() == [ref.W, ref.n, 0, 0] and not g_nan.any()
                assert np.array_equal(g_binw, binw) and np.array_equal(g_xnan, xnan)
                t_info, t_nan, t_binw, t_xnan = _twin(x, y, w, piv, edges, n_bins, dtype)
                assert np.array_equal(t_info, g_info) and np.array_equal(t_nan, g_nan) and np.array_equal(t_binw, g_binw)
                assert np.array_equal(t_xnan, g_xnan)
                _same(_run(x, y, w, piv, edges, n_bins, dtype, ld_pad, off), first, "the same call twice")
            else:
                _same(got, first, f"ld + {ld_pad}, offset {off}")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_a_32_by_32_call_is_the_concatenation_of_its_tile_sized_calls(dtype):
    t = _tile()
    n = t[2] + 1
    x, y, w, piv, edges = case_data(n, 32, 32, 32, "mix", t[2])
    full = _run(x, y, w, piv, edges, 32, dtype)
    for i0 in range(0, 32, t[0]):                              # the tiles of the co-moment pass ...
        for j0 in range(0, 32, t[1]):
            i, j = slice(i0, i0 + t[0]), slice(j0, j0 + t[1])
            got = _run(x[i], y[j], w, np.concatenate([piv[i], piv[32:][j]]), edges[i], 32, dtype)
            assert got[0].tobytes() == full[0][i, j].tobytes(), (i0, j0)
            assert got[1].tobytes() == np.concatenate([full[1][i], full[1][32:][j]]).tobytes(), (i0, j0)
            assert got[4].tobytes() == np.ascontiguousarray(full[4][i, :, j]).tobytes(), (i0, j0)
    for i0 in (0, 13, 31):                                     # ... and those of the conditional sums: one x row, COND_TILE_Y y rows
        for j0 in range(0, 32, t[6]):
            j = slice(j0, j0 + t[6])
            got = _run(x[i0:i0 + 1], y[j], w, np.concatenate([piv[i0:i0 + 1], piv[32:][j]]), edges[i0:i0 + 1], 32, dtype)
            assert got[4].tobytes() == np.ascontiguousarray(full[4][i0:i0 + 1, :, j]).tobytes(), (i0, j0)
            assert np.array_equal(got[5], full[5][i0:i0 + 1])


def test_flags_nan_rows_and_the_python_layer():
    from fiveeqscm_amd.joint import joint_moments, sensitivity
    t = _tile()
    n = 700
    x, y, w, piv, edges = case_data(n, 5, 3, 8, "mix", t[2])
    live = np.nonzero(w > 0)[0]
    w2 = w.copy()
    w2[live[0]] = W_ONE + 1                                     # above 2^32: flag bit 1
    assert _run(x, y, w2, piv, edges, 8, torch.float64)[2][2] == 2
    xn, yn = x.copy(), y.copy()
    xn[2, live[3]], yn[1, live[5]] = np.nan, np.nan             # NaNs under positive weight
    got = _run(xn, yn, w, piv, edges, 8, torch.float64)
    assert got[2][2] == 1 and got[3].tolist() == [0, 0, int(w[live[3]]), 0, 0, 0, int(w[live[5]]), 0]
    assert np.isnan(got[0][2]).all() and np.isnan(got[0][:, 1]).all() and not np.isnan(np.delete(np.delete(got[0], 2, 0), 1, 1)).any()
    assert got[6].tolist() == [0, 0, int(w[live[3]]), 0, 0] and int(got[5][2].sum()) == int(w.sum()) - int(w[live[3]])
    assert np.isnan(got[4][:, :, 1]).any() and not np.isnan(got[4][:, :, [0, 2]]).any()
    xd, yd = torch.from_numpy(xn).to(DEV), torch.from_numpy(yn).to(DEV)
    with pytest.raises(ValueError, match="outside"):
        joint_moments(xd, yd, weights=torch.from_numpy(w2).to(DEV))
    with pytest.raises(TypeError):
        joint_moments(xd.cpu(), yd.cpu())
    s = sensitivity(xd, yd.to(torch.float32), bins=8, weights=torch.from_numpy(w).to(DEV))       # a mix of dtypes is widened
    nan_pair = torch.isnan(s.moments.cov)
    assert nan_pair[2].all() and nan_pair[:, 1].all() and int(nan_pair.sum()) == 3 + 5 - 1
    assert torch.isnan(s.eta2[2]).all() and torch.isnan(s.eta2[:, 1]).all() and int(torch.isnan(s.eta2).sum()) == 7


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_the_python_layer_reads_a_wider_buffer_in_place_and_copies_a_strided_view(dtype):
    """joint.sensitivity on x [3, N], y [2, N] of one 256-member tile plus three members: rows in buffers N + 3 wide (read in
    place: ld_x = ld_y = N + 3) and on every second column of buffers 2 N wide (copied) — every bit of the same call on
    contiguous clones."""
    from fiveeqscm_amd.joint import sensitivity
    n = 259
    x, y, w, _, _ = case_data(n, 3, 2, 8, "mix", _tile()[2])
    xd, yd = (torch.from_numpy(a.astype(NP[dtype])).to(DEV) for a in (x, y))
    wd = torch.from_numpy(w.astype(np.int64)).to(DEV)
    base = sensitivity(xd.clone(), yd.clone(), bins=8, weights=wd)
    assert not bool(torch.isnan(base.eta2).any()) and base.moments.weight_sum == int(w.sum())
    bits = lambda t: t.contiguous().view(torch.int64)                                        # noqa: E731  (NaN equal to NaN)

    def embed(rows, width, step):
        view = torch.full((rows.shape[0], width), float("nan"), dtype=dtype, device=DEV)[:, :step * n:step]
        view.copy_(rows)
        return view
    for width, step in ((n + 3, 1), (2 * n, 2)):
        xv, yv = embed(xd, width, step), embed(yd, width, step)
        assert xv.stride() == (width, step) and yv.stride() == (width, step)
        got = sensitivity(xv, yv, bins=8, weights=wd)
        for name in ("eta2", "cond_mean", "bin_weight", "edges"):
            assert torch.equal(bits(getattr(got, name)), bits(getattr(base, name))), (width, name)
        for name in ("mean_x", "mean_y", "var_x", "var_y", "cov", "corr", "slope"):
            assert torch.equal(bits(getattr(got.moments, name)), bits(getattr(base.moments, name))), (width, name)
        assert (got.moments.weight_sum, got.moments.count, got.moments.ess) == (base.moments.weight_sum, base.moments.count, base.moments.ess)


def _sha(eng):
    return [hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()
            for t in (eng.R, eng.S, eng.T, eng.C, eng.r, eng.q, eng.fscale, eng.misfit) if t is not None]


def test_engine_drivers_end_to_end():
    from fiveeqscm_amd import params as prm
    from fiveeqscm_amd.constrain import Observations, importance_weights
    from fiveeqscm_amd.emissions import rcp_like_emissions
    from fiveeqscm_amd.engine import EnsembleEngine
    from fiveeqscm_amd.forcing import ExternalForcings
    N, n_steps = 4096, 60
    base = prm.default_params("multigas")
    p = prm.sample_ensemble_shard(base, N, device=DEV)
    sc = prm.sample_forcing_scales(base, N, ranges=[(0.8, 1.2)] * 3 + [(0.3, 2.0), (0.5, 1.5)], seed=7, device=DEV)
    p["f_scale"], p["fx_scale"] = sc[:3], sc[3:]
    tt = np.arange(n_steps)
    years = 1850.0 + tt
    eng = EnsembleEngine(p, N, rcp_like_emissions(n_steps, 3), dtype=torch.float64, output_steps=[20, 40, 59], device=DEV,
                         forcing=ExternalForcings(np.stack([-0.4 * tt / n_steps, np.where(tt % 17 == 5, -2.5, 0.0)], 1), ("aerosol", "volcanic")),
                         observations=Observations.from_years(years, years[20:55], 0.01 * (years[20:55] - 1850.0), 0.1, baseline=(1850, 1869)))
    eng.run()
    before = _sha(eng)
    names, rows = eng.parameter_rows()
    assert names == [f"{k}[{g}]" for g in range(3) for k in ("r0", "rC", "rT")] + ["q[0]", "q[1]", "ECS", "TCR"] + \
        [f"f_scale[{g}]" for g in range(3)] + ["fx_scale[0]", "fx_scale[1]"]
    assert rows.shape == (18, N) and rows.dtype == torch.float64 and rows.is_cuda
    for name in ("ECS", "TCR"):                                # the round trip q -> (ECS, TCR): tests/test_joint_cpu.py derives the bound
        want = torch.as_tensor(p[name], device=DEV).to(torch.float64)
        assert float(((rows[names.index(name)] - want).abs() / want).max()) <= 1e-13, name
    pick = ["ECS", "TCR", "rT[0]", "fx_scale[0]", "f_scale[1]"]
    assert eng.parameter_rows(pick)[0] == pick and torch.equal(eng.parameter_rows(pick)[1], rows[[names.index(v) for v in pick]])
    with pytest.raises(ValueError, match="no rows"):
        eng.parameter_rows(["ECS", "nope"])
    w = importance_weights(eng.chi2())
    xh, yh = rows[[names.index(v) for v in pick]].cpu().numpy(), eng.T[-1:].cpu().numpy()
    for weights in (None, w):
        s = eng.drivers(eng.T[-1:], names=pick, bins=16, weights=weights)
        wh = np.ones(N, dtype=np.int64) if weights is None else weights.cpu().numpy()
        piv = np.concatenate([s.moments.mean_x.numpy(), s.moments.mean_y.numpy()])
        ref = Ref(xh, yh, wh, piv, s.edges.numpy())
        want = ref.finished(16)
        assert s.moments.weight_sum == ref.W and s.moments.count == ref.n
        assert np.array_equal(s.bin_weight.numpy(), want["bin_weight"])
        scale = np.sqrt(want["var"][:5, None] * want["var"][None, 5:])
        t_cov, t_unit = finished_tol(ref.n)
        assert np.all(np.abs(s.moments.cov.numpy() - want["cov"]) <= t_cov * scale)
        assert np.all(np.abs(s.moments.corr.numpy() - want["corr"]) <= t_unit)
        assert np.all(np.abs(s.eta2.numpy() - want["eta2"]) <= t_unit)
        if weights is None:                                    # (the posterior of this toy record has an ess below the bin count)
            assert float(s.eta2[0, 0]) > 5 * s.noise_floor     # ECS drives warming
    assert _sha(eng) == before
