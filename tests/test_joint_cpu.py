"""Joint statistics without a GPU: the C ABI (exported, bound, additive, validated on the host), the NumPy twin of the two
passes against the exact reference (tests/joint_reference.py) on the GPU test's case table, joint.joint_moments / sensitivity
under host_passes(), known answers, and the collectives over gloo."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fiveeqscm_amd import _capi, _joint_host
from fiveeqscm_amd.distributed import shard_bounds
from fiveeqscm_amd.joint import joint_moments, sensitivity
from fiveeqscm_amd.params import ecs_tcr, k_q
from joint_reference import WEIGHT_KINDS, Ref, case_data, case_table, finished_tol, tol

NEW = ["fiveeq_joint_moments_f64", "fiveeq_joint_moments_f32", "fiveeq_cond_sums_f64", "fiveeq_cond_sums_f32", "fiveeq_joint_tile",
       "fiveeq_joint_chunks", "fiveeq_max_joint_rows", "fiveeq_max_cond_bins", "fiveeq_joint_moments_words", "fiveeq_cond_sums_words"]
T = _capi.JOINT_TILE


def test_new_symbols_are_exported_and_the_abi_is_additive():
    lib = _capi.load()
    for name in NEW:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    assert lib.fiveeq_abi_version() == _capi.ABI_VERSION == 13
    assert lib.fiveeq_sizeof_model() == ctypes.sizeof(_capi.Model) == 448
    names = [os.path.basename(p) for p in _capi.SOURCES]
    assert names.index("fiveeq_joint.hpp") == names.index("fiveeq_metrics.hpp") + 1 == names.index("fiveeq_diag.hpp") - 1
    assert lib.fiveeq_max_joint_rows() == _capi.MAX_JOINT_ROWS == 32 and lib.fiveeq_max_cond_bins() == _capi.MAX_COND_BINS == 32
    assert tuple(lib.fiveeq_joint_tile(k) for k in range(9)) == _capi.JOINT_TILE + (0,)
    assert _capi.JOINT_CHUNK % (4 * _capi.JOINT_BLOCK) == 0
    assert [lib.fiveeq_joint_chunks(n) for n in (0, 1, _capi.JOINT_CHUNK, _capi.JOINT_CHUNK + 1)] == [0, 1, 1, 2]
    tw = _joint_host.JointPasses()
    assert lib.fiveeq_joint_moments_words(5, 7) == tw.fiveeq_joint_moments_words(5, 7) == 35 + 36 + 3
    assert lib.fiveeq_cond_sums_words(5, 7, 9) == tw.fiveeq_cond_sums_words(5, 7, 9) == 5 * 9 * 8 + 5


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_the_entry_points_validate_on_the_host(sfx):
    """Every call returns on the host with an error code: the fake pointers are never dereferenced, nothing is launched."""
    lib = _capi.load()
    el = 8 if sfx == "f64" else 4
    p = ctypes.c_void_p(0x1000)
    odd = lambda k: ctypes.c_void_p(0x1000 + k)   # noqa: E731
    E = _capi.E_INVALID
    err = lambda: lib.fiveeq_last_error().decode()   # noqa: E731

    def mom(n=8, n_x=2, ld_x=8, x=p, n_y=3, ld_y=8, y=p, weights=p, pivots=p, partial=p, co=p, margins=p, info=p, nanrows=p):
        return getattr(lib, f"fiveeq_joint_moments_{sfx}")(n, n_x, ld_x, x, n_y, ld_y, y, weights, pivots, partial, co, margins, info, nanrows, None)

    def cond(n=8, n_x=2, ld_x=8, x=p, n_y=3, ld_y=8, y=p, weights=p, n_bins=4, edges=p, pivots=p, partial=p, sums=p, binw=p, xnan=p):
        return getattr(lib, f"fiveeq_cond_sums_{sfx}")(n, n_x, ld_x, x, n_y, ld_y, y, weights, n_bins, edges, pivots, partial, sums, binw, xnan, None)

    for fn, outs in ((mom, ("co", "margins", "info", "nanrows")), (cond, ("edges", "sums", "binw", "xnan"))):
        for name in ("x", "y", "weights", "pivots", "partial") + outs:
            assert fn(**{name: None}) == E and name in err() and "NULL" in err(), name
            k = el // 2 if name in ("x", "y") else 4
            assert fn(**{name: odd(k)}) == E and name in err() and "aligned" in err(), name
        for n in (0, -1, 2 ** 31):
            assert fn(n=n, ld_x=2 ** 31, ld_y=2 ** 31) == E and "n_members" in err()
        assert fn(ld_x=7) == E and "ld_x" in err()
        assert fn(ld_y=7) == E and "ld_y" in err()
        for k in (0, -1, 33):
            assert fn(n_x=k) == E and "n_x" in err()
            assert fn(n_y=k) == E and "n_y" in err()
    for b in (0, -1, 33):
        assert cond(n_bins=b) == E and "n_bins" in err()


def _twin_run(x, y, w, piv, edges, n_bins, npd):
    tw = _joint_host.JointPasses()
    xs, ys, ws = np.ascontiguousarray(x.astype(npd)), np.ascontiguousarray(y.astype(npd)), np.ascontiguousarray(w.astype(np.uint64))
    (n_x, n), n_y = x.shape, y.shape[0]
    R = n_x + n_y
    co, mar, info, nanr = np.zeros(n_x * n_y), np.zeros(2 * R), np.zeros(4, dtype=np.uint64), np.zeros(R, dtype=np.uint64)
    sums, binw, xnan = np.zeros(n_x * n_bins * n_y), np.zeros(n_x * n_bins, dtype=np.uint64), np.zeros(n_x, dtype=np.uint64)
    ed = np.ascontiguousarray(edges.reshape(-1))
    a = lambda t: t.ctypes.data      # noqa: E731
    sfx = "f64" if npd == np.float64 else "f32"
    assert getattr(tw, f"fiveeq_joint_moments_{sfx}")(n, n_x, n, a(xs), n_y, n, a(ys), a(ws), a(piv), 0, a(co), a(mar), a(info), a(nanr), None) == 0
    assert getattr(tw, f"fiveeq_cond_sums_{sfx}")(n, n_x, n, a(xs), n_y, n, a(ys), a(ws), n_bins, a(ed) if n_bins > 1 else 0, a(piv[n_x:]), 0,
                                                  a(sums), a(binw), a(xnan), None) == 0
    return (co.reshape(n_x, n_y), mar.reshape(R, 2), info.astype(np.int64), nanr.astype(np.int64), sums.reshape(n_x, n_bins, n_y),
            binw.astype(np.int64).reshape(n_x, n_bins), xnan.astype(np.int64))


@pytest.mark.parametrize("kind", WEIGHT_KINDS)
@pytest.mark.parametrize("k", range(10))
def test_the_numpy_twin_against_the_exact_reference(k, kind):
    n, n_x, n_y, n_bins = case_table(T[0], T[1], T[2], T[3] * T[7])[k]
    x, y, w, piv, edges = case_data(n, n_x, n_y, n_bins, kind, T[2])
    ref = Ref(x, y, w, piv, edges)
    co, co_abs, mar, mar_abs = ref.moments()
    sums, sabs, cnt, binw, xnan = ref.cond(n_bins)
    for npd in (np.float64, np.float32):
        g_co, g_mar, g_info, g_nan, g_sums, g_binw, g_xnan = _twin_run(x, y, w, piv, edges, n_bins, npd)
        assert np.all(np.abs(g_co - co) <= tol(ref.n, co_abs)) and np.all(np.abs(g_mar - mar) <= tol(ref.n, mar_abs))
        assert np.all(np.abs(g_sums - sums) <= tol(cnt[:, :, None], sabs))
        assert g_info.tolist() == [ref.W, ref.n, 0, 0] and not g_nan.any()
        assert np.array_equal(g_binw, binw) and np.array_equal(g_xnan, xnan)


def _rows(n=600, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(3, n))
    y = np.stack([2.0 * x[0] - x[1] + 0.3 * rng.normal(size=n), np.sin(3 * x[2]) + 0.1 * rng.normal(size=n)])
    w = rng.choice(np.array([0, 1, 5, 1 << 32], dtype=np.int64), size=n)
    return x, y, w


def test_python_layer_under_host_passes():
    x, y, w = _rows()
    tx, ty, tw = torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(w)
    with pytest.raises(TypeError):
        joint_moments(tx, ty)                                  # host rows, no twin installed: refused
    with _joint_host.host_passes():
        s = sensitivity(tx, ty, bins=8, weights=tw)
        ref = Ref(x, y, w, np.concatenate([s.moments.mean_x.numpy(), s.moments.mean_y.numpy()]), s.edges.numpy())
        want = ref.finished(8)
        t_cov, t_unit = finished_tol(ref.n)
        scale = np.sqrt(want["var"][:3, None] * want["var"][None, 3:])
        assert np.all(np.abs(s.moments.cov.numpy() - want["cov"]) <= t_cov * scale)
        assert np.all(np.abs(s.moments.corr.numpy() - want["corr"]) <= t_unit) and np.all(np.abs(s.eta2.numpy() - want["eta2"]) <= t_unit)
        assert np.array_equal(s.bin_weight.numpy(), want["bin_weight"]) and s.moments.weight_sum == ref.W and s.moments.count == ref.n
        assert s.noise_floor == 7 / (s.moments.ess - 1) and s.cond_mean.shape == (3, 8, 2) and s.bin_weight.dtype == torch.int64
        assert float(s.eta2[2, 1]) > 0.5 > float(s.moments.corr[2, 1]) ** 2       # the non-linear dependence eta2 sees and corr does not
        # mixed dtypes: widened to fp64 on the rows' device — the answer of the widened rows
        y32 = ty.to(torch.float32)
        a, b = sensitivity(tx, y32, bins=8, weights=tw), sensitivity(tx, y32.to(torch.float64), bins=8, weights=tw)
        assert torch.equal(a.eta2, b.eta2) and torch.equal(a.moments.cov, b.moments.cov)
        # accepted against 0 / 1 weights; both given
        mask = tw > 0
        a, b = sensitivity(tx, ty, bins=8, accepted=mask), sensitivity(tx, ty, bins=8, weights=mask.to(torch.int64))
        for f in ("eta2", "cond_mean", "bin_weight", "edges"):
            assert torch.equal(getattr(a, f).nan_to_num(-7.0), getattr(b, f).nan_to_num(-7.0)), f
        assert torch.equal(a.moments.cov, b.moments.cov) and a.moments.weight_sum == int(mask.sum())
        with pytest.raises(ValueError, match="exclude"):
            joint_moments(tx, ty, weights=tw, accepted=mask)
        with pytest.raises(ValueError, match="sum to 0"):
            joint_moments(tx, ty, weights=torch.zeros_like(tw))
        with pytest.raises(ValueError, match="outside"):
            joint_moments(tx, ty, weights=tw + (1 << 32))
        with pytest.raises(ValueError, match="bins"):
            sensitivity(tx, ty, bins=33)
        # a constant x row: eta2 0, corr NaN; a constant y row: eta2 NaN; bins = 1: eta2 0
        xc, yc = tx.clone(), ty.clone()
        xc[1], yc[0] = 0.1, -2.5
        s = sensitivity(xc, yc, bins=8, weights=tw)
        assert s.eta2[1, 1] == 0 and torch.isnan(s.moments.corr[1]).all() and s.moments.var_x[1] == 0
        assert torch.isnan(s.eta2[:, 0]).all() and torch.isnan(s.moments.corr[:, 0]).all() and not torch.isnan(s.eta2[[0, 2], 1]).any()
        assert int((s.bin_weight[1] > 0).sum()) == 1           # every member of the constant row sits in one bin: the rest are empty
        s1 = sensitivity(tx, ty, bins=1, weights=tw)
        assert torch.equal(s1.eta2, torch.zeros(3, 2, dtype=torch.float64)) and s1.edges.shape == (3, 0) and s1.noise_floor == 0
        # a NaN under weight 0 is ignored; under positive weight it makes exactly its row's pairs NaN
        xn, yn = tx.clone(), ty.clone()
        zero, live = int(torch.nonzero(tw == 0)[0]), int(torch.nonzero(tw > 0)[0])
        xn[0, zero], yn[1, zero] = float("nan"), float("inf")
        a, b = sensitivity(xn, yn, bins=8, weights=tw), sensitivity(tx, ty, bins=8, weights=tw)
        assert torch.equal(a.eta2, b.eta2) and torch.equal(a.moments.cov, b.moments.cov)
        xn[0, live] = float("nan")
        s = sensitivity(xn, yn, bins=8, weights=tw)
        for f in (s.eta2, s.moments.cov, s.moments.corr):
            assert torch.isnan(f[0]).all() and not torch.isnan(f[1:]).any()
        # ties sitting on an edge belong to the lower bin, and a bin nobody falls into stays empty
        xt = torch.tensor([[1.0] * 6 + [2.0] * 2])
        s = sensitivity(xt, torch.arange(8.0)[None], bins=4)
        assert s.edges.tolist() == [[1.0, 1.0, 1.0]] and s.bin_weight.tolist() == [[6, 0, 0, 2]]
        assert torch.isnan(s.cond_mean[0, 1:3]).all() and s.cond_mean[0, :, 0][[0, 3]].tolist() == [2.5, 6.5]


def test_known_answers():
    with _joint_host.host_passes():
        rng = np.random.default_rng(5)
        x = torch.from_numpy(rng.normal(size=(1, 500)))
        for a in (2.5, -0.75):
            jm = joint_moments(x, a * x + 1.25)
            assert abs(float(jm.corr[0, 0]) - np.sign(a)) <= 1e-12 and abs(float(jm.slope[0, 0]) - a) <= 1e-12 * abs(a)
        N, B = 4096, 16
        xk = ((torch.arange(N, dtype=torch.float64) + 0.5) / N)[None]
        s = sensitivity(xk, xk.clone(), bins=B)
        assert s.bin_weight.tolist() == [[N // B] * B]
        assert abs(float(s.eta2[0, 0]) - (1 - ((N / B) ** 2 - 1) / (N ** 2 - 1))) <= 1e-12


def test_ecs_tcr_inverts_k_q():
    """The bound: in np.longdouble the round trip of these rows returns TCR and ECS to 1e-13 relative with d = [239, 4.1] (the
    test prints what it finds); the fp64 round trip is held to 1e-13."""
    rng = np.random.default_rng(9)
    d, F2x = np.array([239.0, 4.1]), 3.74
    TCR = rng.uniform(1.0, 2.5, 2000)
    ECS = TCR * rng.uniform(1.1, 2.5, 2000)
    ecs, tcr = ecs_tcr(k_q(TCR, ECS, d, F2x), d, F2x)
    worst = max(np.max(np.abs(ecs - ECS) / ECS), np.max(np.abs(tcr - TCR) / TCR))
    ld = np.longdouble
    k = 1 - (d.astype(ld) / 70) * (-np.expm1(-70 / d.astype(ld)))
    q = k_q(TCR, ECS, d, F2x).astype(ld)
    worst_ld = max(np.max(np.abs(F2x * (q[0] + q[1]) - ECS) / ECS), np.max(np.abs(F2x * (q[0] * k[0] + q[1] * k[1]) - TCR) / TCR))
    print(f"round trip: fp64 {worst:.3e}, evaluated in longdouble from the fp64 q {float(worst_ld):.3e}")
    assert worst <= 1e-13
    eq, et = ecs_tcr(torch.from_numpy(k_q(TCR, ECS, d, F2x)), d, F2x)
    assert isinstance(eq, torch.Tensor) and np.array_equal(eq.numpy(), ecs) and np.array_equal(et.numpy(), tcr)


# ---- gloo: world 2 and 3 against world 1 --------------------------------------------------------------------------------------
N_GLOO = 1000


def _gloo_rows():
    x, y, w = _rows(N_GLOO, seed=21)
    lo, hi = shard_bounds(N_GLOO, 1, 3)
    w[lo:hi] = 0                                               # the members of rank 1 of world 3 all weigh 0
    return x, y, w


def _evaluate(lo, hi):
    x, y, w = _gloo_rows()
    s = sensitivity(torch.from_numpy(x[:, lo:hi].copy()), torch.from_numpy(y[:, lo:hi].copy()), bins=8, weights=torch.from_numpy(w[lo:hi].copy()))
    m = s.moments
    return {"ints": (m.weight_sum, m.count, s.bin_weight.tolist(), s.edges.numpy().view(np.int64).tolist()),
            "cov": m.cov.numpy(), "corr": m.corr.numpy(), "eta2": s.eta2.numpy(), "var": np.concatenate([m.var_x.numpy(), m.var_y.numpy()])}


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _joint_host.install()
        q.put((rank, _evaluate(*shard_bounds(N_GLOO, rank, world))))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _spawn(world):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return dict(results)


@pytest.mark.parametrize("world", [2, 3])
def test_world_1_equals_world_2_and_3_over_gloo(world):
    with _joint_host.host_passes():
        one = _evaluate(0, N_GLOO)
    x, y, w = _gloo_rows()
    t_cov, t_unit = finished_tol(int((w > 0).sum()))
    scale = np.sqrt(one["var"][:3, None] * one["var"][None, 3:])
    got = _spawn(world)
    for rank in range(world):
        g = got[rank]
        assert g["ints"] == one["ints"], rank                  # weight_sum, count, bin_weight, edges: bit for bit
        assert np.all(np.abs(g["cov"] - one["cov"]) <= 2 * t_cov * scale)        # each side within the bound of the exact value
        assert np.all(np.abs(g["corr"] - one["corr"]) <= 2 * t_unit) and np.all(np.abs(g["eta2"] - one["eta2"]) <= 2 * t_unit)
        assert g["cov"].tobytes() == got[0]["cov"].tobytes() and g["eta2"].tobytes() == got[0]["eta2"].tobytes()      # every rank holds the same bits
