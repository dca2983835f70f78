"""The weighted summary without a GPU: the integer weights, the rank arithmetic, the NumPy restatement of the four passes
against the independent reference (tests/weighted_reference.py), the host logic over gloo, and the C ABI's validation."""
import ctypes
import os
import socket
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fiveeqscm_amd import _capi, _wsummary_host
from fiveeqscm_amd.constrain import W_ONE, importance_weights
from fiveeqscm_amd.distributed import gather_weighted_summary, shard_bounds, weighted_rank
from weighted_reference import rank_of, weighted_rows

PCT = (0.0, 5.0, 50.0, 95.0, 100.0)
U = 2.0 ** -53


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): the relative error bound of k successive fp64 roundings."""
    return k * U / (1.0 - k * U)


# ---- importance_weights ----------------------------------------------------------------------------------------------------
def test_importance_weights_follow_the_formula_exactly():
    rng = np.random.default_rng(11)
    chi2 = rng.gamma(3.0, 4.0, size=4001)
    chi2[[5, 77]] = np.nan
    chi2[100] = chi2[np.nanargmin(chi2)] + 200.0                      # far tail: floor(2^32 e^-100) = 0
    w = importance_weights(chi2)
    assert w.dtype == np.int64 and w.shape == chi2.shape
    cmin = np.nanmin(chi2)
    for m in range(chi2.size):
        want = 0 if np.isnan(chi2[m]) else int(np.floor(float(W_ONE) * np.exp(-(chi2[m] - cmin) / 2.0)))
        assert int(w[m]) == want, m
    assert w[5] == 0 and w[77] == 0 and w[100] == 0
    assert int(w[np.nanargmin(chi2)]) == W_ONE == 2 ** 32 and w.max() == W_ONE and w.min() >= 0
    t = importance_weights(torch.from_numpy(chi2))
    assert t.dtype == torch.int64 and np.array_equal(t.numpy(), w)


def _worker_weights(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        chi2 = _scores()
        lo, hi = shard_bounds(chi2.size, rank, world)
        q.put((rank, importance_weights(chi2[lo:hi]).tolist()))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _scores():
    chi2 = np.random.default_rng(5).gamma(2.0, 3.0, size=1003)
    chi2[17] = np.nan
    return chi2


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
    return results


@pytest.mark.parametrize("world", [2, 3])
def test_importance_weights_are_the_same_for_any_split(world):
    whole = importance_weights(_scores())
    parts = dict(_spawn(_worker_weights, world))
    assert np.array_equal(np.concatenate([parts[r] for r in range(world)]), whole)


def test_importance_weights_refuse_2_to_31_members():
    huge = np.broadcast_to(np.float64(1.0), (2 ** 31,))                # a view of one number: nothing of that size is allocated
    with pytest.raises(ValueError, match="2\\^31"):
        importance_weights(huge)


# ---- k_p ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 3, 2 ** 62])
@pytest.mark.parametrize("p", [0, 0.1, 2.5, 50, 100])
def test_rank_arithmetic_is_exact(p, W):
    want = Fraction(p) / 100 * W
    k = weighted_rank(p, W)
    assert isinstance(k, int) and 1 <= k <= W
    assert k == max(1, -((-want.numerator) // want.denominator)) == rank_of(p, W)
    assert k >= want and (k == 1 or k - 1 < want)                      # the ceiling, in rationals
    if p == 100:
        assert k == W
    if p == 0:
        assert k == 1


def test_rank_arithmetic_refuses_percentiles_outside_0_100():
    for p in (-0.1, 100.5, float("nan")):
        with pytest.raises(ValueError):
            weighted_rank(p, 10)


# ---- the NumPy restatement of the passes, through the product's host logic, against the reference --------------------------
def _rows_and_weights(n, seed=3):
    rng = np.random.default_rng(seed)
    rows = np.stack([rng.normal(1.5, 0.7, size=n), np.full(n, 2.5), rng.choice([-1.0, 0.5, 0.75, 2.0, 9.0], size=n),
                     rng.standard_cauchy(size=n), rng.normal(size=n)])
    w = rng.integers(0, W_ONE + 1, size=n, dtype=np.int64)
    w[rng.uniform(size=n) < 0.5] = 0
    if not w.any():
        w[0] = W_ONE
    zero = np.nonzero(w == 0)[0]
    if zero.size >= 3:
        rows[0, zero[0]], rows[0, zero[1]], rows[3, zero[2]] = np.nan, np.inf, -np.inf     # ignored: weight 0
    if n > 1:
        rows[4, np.nonzero(w)[0][0]] = np.nan                                            # a NaN that carries weight: a NaN row
    return rows, w


def _check_against_reference(s, rows, w, pct):
    ref = weighted_rows(rows, w, pct)
    got = s["percentiles"].numpy()
    for k, r in enumerate(ref):
        assert np.array_equal(got[k], r["percentiles"], equal_nan=True), (k, got[k], r["percentiles"])
        assert int(s["count"][k]) == r["count"] and s["weight_sum"] == r["weight_sum"]
        assert float(s["min"][k]) == r["min"] and float(s["max"][k]) == r["max"]
        n = max(r["count"], 1)
        if np.isnan(r["mean"]):
            assert np.isnan(float(s["mean"][k])) and np.isnan(float(s["std"][k]))
        else:
            # sum w x: n products rounded once (u each) summed in fp64 (at most n - 1 roundings per term), and the reference's
            # own rounded products and fsum: gamma(n + 2) sum |w x|; then float(W) and the division: 3 more roundings
            assert abs(float(s["mean"][k]) - r["mean"]) <= gamma(n + 2) * r["sum_abs_wx"] / r["weight_sum"] + gamma(4) * abs(r["mean"])
        # sum w^2 likewise (positive terms: the bound is relative), float(W) twice, a product, a division, the reference's rounding
        assert abs(s["ess"] - r["ess"]) <= gamma(n + 6) * r["ess"]
    assert s["method"] == "weighted_inverted_cdf"


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [1, 2, 65, 1000, 4097])
def test_host_passes_equal_the_reference(n, dtype):
    rows, w = _rows_and_weights(n)
    rows = rows.astype(dtype)
    with _wsummary_host.host_passes():
        s = gather_weighted_summary(torch.from_numpy(rows), torch.from_numpy(w), PCT)
    _check_against_reference(s, rows, w, PCT)


def test_host_passes_special_weight_patterns():
    rng = np.random.default_rng(8)
    n = 777
    rows = np.stack([rng.normal(size=n), rng.standard_cauchy(size=n)])
    patterns = {"equal": np.full(n, 7, dtype=np.int64), "one": np.zeros(n, dtype=np.int64), "at_min": np.zeros(n, dtype=np.int64),
                "at_max": np.zeros(n, dtype=np.int64), "all_one": np.full(n, W_ONE, dtype=np.int64)}
    patterns["one"][123] = 5
    patterns["at_min"][np.argmin(rows[0])] = W_ONE
    patterns["at_max"][np.argmax(rows[0])] = 1
    with _wsummary_host.host_passes():
        for name, w in patterns.items():
            s = gather_weighted_summary(torch.from_numpy(rows), torch.from_numpy(w), (0, 0.1, 2.5, 50, 100))
            _check_against_reference(s, rows, w, (0, 0.1, 2.5, 50, 100))
        with pytest.raises(ValueError, match="sum to 0"):
            gather_weighted_summary(torch.from_numpy(rows), torch.zeros(n, dtype=torch.int64), PCT)
        with pytest.raises(ValueError, match="outside"):
            gather_weighted_summary(torch.from_numpy(rows), torch.full((n,), W_ONE + 1, dtype=torch.int64), PCT)
        with pytest.raises(ValueError, match="outside"):
            gather_weighted_summary(torch.from_numpy(rows), torch.full((n,), -1, dtype=torch.int64), PCT)
        with pytest.raises(ValueError, match="int64"):
            gather_weighted_summary(torch.from_numpy(rows), torch.ones(n, dtype=torch.float64), PCT)


def test_host_rows_are_refused_without_the_switch():
    with pytest.raises(TypeError, match="no CPU fallback"):
        gather_weighted_summary(torch.zeros((1, 4), dtype=torch.float64), torch.ones(4, dtype=torch.int64), PCT)


# ---- the host logic over gloo: world 2 and 3, a rank whose weights are all zero, an empty shard ---------------------------
def _worker_summary(rank, world, port, case, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    _wsummary_host.install()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rows, w, bounds = _gloo_case(case, world)
        lo, hi = bounds[rank]
        out = []
        for dt in (np.float64, np.float32):
            s = gather_weighted_summary(torch.from_numpy(np.ascontiguousarray(rows[:, lo:hi].astype(dt))),
                                        torch.from_numpy(np.ascontiguousarray(w[lo:hi])), PCT)
            out.append({k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in s.items()})
        zero_raised = False
        try:
            gather_weighted_summary(torch.from_numpy(np.ascontiguousarray(rows[:, lo:hi])),
                                    torch.zeros(hi - lo, dtype=torch.int64), PCT)
        except ValueError:
            zero_raised = True                                         # W == 0: on EVERY rank
        q.put((rank, out, zero_raised))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _gloo_case(case, world):
    if case == "zero_rank":                                            # the last rank's members all weigh 0
        rows, w = _rows_and_weights(1001, seed=21)
        bounds = [shard_bounds(1001, r, world) for r in range(world)]
        w = w.copy()
        w[bounds[-1][0]:] = 0
        rows[4] = np.random.default_rng(1).normal(size=1001)           # (the NaN row's NaN may have lost its weight: plain row)
        return rows, w, bounds
    rows, w = _rows_and_weights(2, seed=22)                            # two members on three ranks: an empty shard
    return rows, w, [shard_bounds(2, r, world) for r in range(world)]


@pytest.mark.parametrize("world,case", [(2, "zero_rank"), (3, "zero_rank"), (3, "empty_shard")])
def test_gloo_rehearsal_gives_the_one_rank_percentiles(world, case):
    rows, w, _ = _gloo_case(case, world)
    results = {r: (out, z) for r, out, z in _spawn(_worker_summary, world, case)}
    assert all(z for _, z in results.values())
    for i, dt in enumerate((np.float64, np.float32)):
        x = rows.astype(dt)
        with _wsummary_host.host_passes():
            one = gather_weighted_summary(torch.from_numpy(x), torch.from_numpy(w), PCT)
        root = results[0][0][i]
        assert np.array_equal(root["percentiles"], one["percentiles"].numpy(), equal_nan=True)      # bit for bit
        _check_against_reference({k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in root.items()}, x, w, PCT)
        for r in range(1, world):
            other = results[r][0][i]
            assert other["percentiles"] is None and other["weight_sum"] == one["weight_sum"]
            assert np.array_equal(other["count"], one["count"].numpy()) and np.array_equal(other["min"], root["min"])


# ---- the C ABI: exported, bound, additive, and validated on the host ------------------------------------------------------
NEW = [f"fiveeq_{n}_{s}" for n in ("wrow_moments", "whist_rows_ranged", "wselect_bins", "wselect_pick") for s in ("f64", "f32")] \
    + ["fiveeq_wrow_moments_chunks"]


def test_new_symbols_are_exported_and_the_abi_is_additive():
    lib = _capi.load()
    for name in NEW:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    assert lib.fiveeq_abi_version() == _capi.ABI_VERSION == 13
    assert lib.fiveeq_sizeof_model() == ctypes.sizeof(_capi.Model) == 448
    assert [lib.fiveeq_wrow_moments_chunks(k, n) for k, n in ((0, 8), (3, 0), (1, 1), (3, 1000))] == [0, 0, 1, 1]
    assert lib.fiveeq_wrow_moments_chunks(3, 10 ** 8) == lib.fiveeq_row_moments_chunks(3, 10 ** 8) > 1


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_new_entry_points_validate_on_the_host(sfx):
    """Every call returns on the host with an error code: the fake pointers are never dereferenced, nothing is launched."""
    lib = _capi.load()
    p, odd, null = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1001), None
    E = _capi.E_INVALID
    err = lambda: lib.fiveeq_last_error().decode()   # noqa: E731
    mom = getattr(lib, f"fiveeq_wrow_moments_{sfx}")
    hist = getattr(lib, f"fiveeq_whist_rows_ranged_{sfx}")
    sel = getattr(lib, f"fiveeq_wselect_bins_{sfx}")
    pick = getattr(lib, f"fiveeq_wselect_pick_{sfx}")
    # moments (rows, weights, partial, moments)
    assert mom(2, 8, 8, null, p, p, p, None) == E and "NULL" in err()
    assert mom(2, 8, 8, p, null, p, p, None) == E and "NULL" in err()
    assert mom(2, 8, 8, p, p, null, p, None) == E and mom(2, 8, 8, p, p, p, null, None) == E
    assert mom(2, 8, 8, odd, p, p, p, None) == E and "aligned" in err()
    assert mom(2, 8, 8, p, odd, p, p, None) == E and "aligned" in err()
    assert mom(2, 8, 8, p, p, p, odd, None) == E and "aligned" in err()
    assert mom(2, 9, 8, p, p, p, p, None) == E and "ld=" in err()
    assert mom(2, 0, 8, p, p, p, p, None) == E and mom(-1, 8, 8, p, p, p, p, None) == E and mom(70000, 8, 8, p, p, p, p, None) == E
    assert mom(0, 8, 8, null, null, null, null, None) == _capi.OK
    # histogram (rows, weights, ranges, n_bins, hist)
    assert hist(2, 8, 8, null, p, p, 16, p, None) == E and hist(2, 8, 8, p, null, p, 16, p, None) == E
    assert hist(2, 8, 8, p, p, null, 16, p, None) == E and "NULL" in err()
    assert hist(2, 8, 8, p, p, p, 16, null, None) == E and "NULL" in err()
    assert hist(2, 8, 8, p, odd, p, 16, p, None) == E and "aligned" in err()
    assert hist(2, 8, 8, p, p, p, 16, odd, None) == E and "aligned" in err()
    assert hist(2, 9, 8, p, p, p, 16, p, None) == E and "ld=" in err()
    assert hist(2, 8, 8, p, p, p, 0, p, None) == E and "n_bins" in err()
    assert hist(2, 8, 8, p, p, p, 4097, p, None) == E and "n_bins" in err()
    assert hist(0, 8, 8, null, null, null, 16, null, None) == _capi.OK
    # selection (rows, weights, ranges, n_bins, binmask, cand, candw, cap, cand_n)
    good = [2, 8, 8, p, p, p, 16, p, p, p, 4, p, None]
    for at in (3, 4, 5, 7, 8, 9, 11):
        bad = list(good)
        bad[at] = null
        assert sel(*bad) == E and "NULL" in err(), at
    for at in (3, 4, 8, 9, 11):
        bad = list(good)
        bad[at] = odd
        assert sel(*bad) == E and "aligned" in err(), at
    assert sel(2, 9, 8, p, p, p, 16, p, p, p, 4, p, None) == E and "ld=" in err()
    assert sel(2, 8, 8, p, p, p, 0, p, p, p, 4, p, None) == E and "n_bins" in err()
    assert sel(2, 8, 8, p, p, p, 5000, p, p, p, 4, p, None) == E and "n_bins" in err()
    assert sel(2, 8, 8, p, p, p, 16, p, p, p, -1, p, None) == E and "cap" in err()
    assert sel(0, 8, 8, null, null, null, 16, null, null, null, 0, null, None) == _capi.OK
    # pick (n_seg, width, pool, poolw, seg_n, n_targets, targets, picked)
    good = [2, 1, 8, p, p, p, 3, p, p, None]
    for at in (3, 4, 5, 7, 8):
        bad = list(good)
        bad[at] = null
        assert pick(*bad) == E and "NULL" in err(), at
        bad[at] = odd
        assert pick(*bad) == E and "aligned" in err(), at
    assert pick(2, 0, 8, p, p, p, 3, p, p, None) == E and "n_seg" in err()
    assert pick(2, 1, -1, p, p, p, 3, p, p, None) == E and "width" in err()
    assert pick(2, 1, 8, p, p, p, 0, p, p, None) == E and "n_targets" in err()
    assert pick(-1, 1, 8, p, p, p, 3, p, p, None) == E
    assert pick(0, 1, 8, null, null, null, 3, null, null, None) == _capi.OK
