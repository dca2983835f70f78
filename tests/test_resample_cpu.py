"""Resampling a weighted ensemble (include/fiveeq.h, "RESAMPLING"), the parts that need no GPU: the rank arithmetic and the
NumPy twins of the kernels against the independent reference (tests/resample_reference.py), the exchange over gloo, and the
C ABI's validation."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fiveeqscm_amd import _capi, _resample_host
from fiveeqscm_amd.constrain import W_ONE, Resample, resample, resample_offset, resample_plan
from fiveeqscm_amd.distributed import shard_bounds
from resample_reference import first_output, offset, source_list, weight_patterns

I64 = 2 ** 63 - 1


def _cases(n=37, seed=11):
    rng = np.random.default_rng(seed)
    for name, w in weight_patterns(n, rng).items():
        W = sum(w)
        for M in (1, 2, 3, n, 3 * n + 1):
            for rho in (0, W - 1, int(rng.integers(0, W))):
                yield name, w, M, rho


def _splits(n):
    """shard bounds: 1, 2, 3 and 8 balanced shards, and a split with an empty shard in the middle"""
    out = [[shard_bounds(n, r, world) for r in range(world)] for world in (1, 2, 3, 8)]
    out.append([(0, n // 3), (n // 3, n // 3), (n // 3, n)])
    return out


def _local_src(w, bounds, M, rho):
    """every shard's src through resample_plan + the host twins, as global member indices"""
    sums = [sum(w[lo:hi]) for lo, hi in bounds]
    out = []
    for rank, (lo, hi) in enumerate(bounds):
        p = resample_plan(sums, rank, M, rho)
        assert p["j0"] == len(out)                                  # the shards tile the outputs in rank order
        n_out = p["j1"] - p["j0"]
        if n_out:
            cum, flag = _resample_host.wscan(np.array(w[lo:hi], dtype=np.int64))
            assert flag == 0
            src = _resample_host.pick(cum, p["C_lo"], M, p["q"], p["a"], p["s"], p["b"], p["j0"], n_out)
            assert src.dtype == np.int32
            out.extend(int(v) + lo for v in src)
    return out


def test_plan_and_host_twins_equal_the_reference_for_every_split():
    """patterns x M x rho: the one-shard list is the reference's; 1, 2, 3, 8 shards and an empty shard concatenate to it"""
    for name, w, M, rho in _cases():
        want = source_list(w, M, rho)
        for bounds in _splits(len(w)):
            assert _local_src(w, bounds, M, rho) == want, (name, M, rho, bounds)


def test_zero_mass_shards_and_all_mass_on_the_last_rank():
    n = 40
    w = [0] * n
    for i in (31, 35, 39):
        w[i] = 5
    for M in (1, 3, n, 3 * n + 1):
        for rho in (0, 14, 7):
            want = source_list(w, M, rho)
            bounds4 = [shard_bounds(n, r, 4) for r in range(4)]          # ranks 0..2 carry no mass
            assert _local_src(w, bounds4, M, rho) == want
            p = resample_plan([0, 0, 0, 15], 1, M, rho)
            assert p["j0"] == p["j1"] == 0 and p["C_lo"] == 0
    w2 = [4] * 10 + [0] * 10 + [9] * 10                                # a zero-mass shard in the middle
    for M in (2, 30, 91):
        assert _local_src(w2, [(0, 10), (10, 20), (20, 30)], M, 5) == source_list(w2, M, 5)


def test_plan_fields_and_int64_bounds():
    """j0 / j1 / q / a / s / b against Python-int arithmetic, up to W = 2^63 - 1 with M = 2^31 - 1: every intermediate of
    p_j = j q + a + (j s + b) div M stays inside int64."""
    rng = np.random.default_rng(5)
    M = 2 ** 31 - 1
    shapes = [([I64], M), ([I64 // 3, I64 - 2 * (I64 // 3), I64 // 3], M), ([2 ** 62, 0, 2 ** 62 - 1], M - 1), ([2 ** 40, 17, 0, 3], 1000),
              ([1], M), ([5, 0, 9], 1)]
    for sums, m in shapes:
        W = sum(sums)
        for rho in (0, W - 1, int(rng.integers(0, W, dtype=np.uint64))):
            for rank in range(len(sums)):
                p = resample_plan(sums, rank, m, rho)
                C_lo = sum(sums[:rank])
                assert p["W"] == W and p["C_lo"] == C_lo
                assert p["j0"] == first_output(C_lo, W, m, rho) and p["j1"] == first_output(C_lo + sums[rank], W, m, rho)
                assert p["q"] * m + p["s"] == W and p["a"] * m + p["b"] == rho and 0 <= p["s"] < m and 0 <= p["b"] < m
                for j in {0, min(1, m - 1), m // 2, m - 1, min(p["j0"], m - 1), max(p["j1"] - 1, 0)}:
                    inner = j * p["s"] + p["b"]
                    pj = j * p["q"] + p["a"] + inner // m
                    assert inner < 2 ** 62 and j * p["q"] + p["a"] <= pj < W <= I64 and pj == (j * W + rho) // m
                if p["j1"] > p["j0"]:                                    # the shard's outputs sit inside its cumulative range
                    assert C_lo <= (p["j0"] * W + rho) // m and ((p["j1"] - 1) * W + rho) // m < C_lo + sums[rank]
    with pytest.raises(ValueError, match="sum to 0"):
        resample_plan([0, 0], 0, 4, 0)
    for bad in (0, 2 ** 31):
        with pytest.raises(ValueError, match="n_out"):
            resample_plan([5], 0, bad, 0)
    with pytest.raises(ValueError, match="offset"):
        resample_plan([5], 0, 3, 5)


def test_copies_per_member_lie_within_floor_and_ceil():
    for name, w, M, rho in _cases(n=53, seed=2):
        W = sum(w)
        counts = np.bincount(resample(np.array(w, dtype=np.int64), M).src, minlength=len(w)).tolist()
        seeded = resample(np.array(w, dtype=np.int64), M, seed=rho)
        assert seeded.offset == offset(rho, M, W) == resample_offset(rho, M, W) and seeded.weight_sum == W
        for c in (counts, np.bincount(seeded.src, minlength=len(w)).tolist()):
            assert sum(c) == M
            for cm, wm in zip(c, w):
                assert (M * wm) // W <= cm <= -((-M * wm) // W), (name, M, wm, cm)
        assert np.all(np.diff(seeded.src) >= 0)
        assert seeded.src.tolist() == source_list(w, M, seeded.offset)


def test_a_mask_compacts_to_its_nonzero_members():
    rng = np.random.default_rng(8)
    for n in (1, 5, 1000):
        mask = rng.integers(0, 2, size=n).astype(bool)
        mask[rng.integers(0, n)] = True
        r = resample(mask)
        assert isinstance(r, Resample) and r.n_out == r.n_members == int(mask.sum()) == r.weight_sum and r.offset == 0 and r.j0 == 0
        assert np.array_equal(r.src, np.nonzero(mask)[0]) and r.src.dtype == np.int32
        t = resample(torch.from_numpy(mask), seed=5)                    # a mask without n_out is compacted whatever the seed
        assert t.offset == 0
        assert t.src.dtype == torch.int32 and np.array_equal(t.src.numpy(), r.src)
        rows = rng.normal(size=(2, 3, n))
        assert np.array_equal(r.gather(rows), rows[..., mask])
        assert torch.equal(t.gather(torch.from_numpy(rows.astype(np.float32))), torch.from_numpy(rows.astype(np.float32)[..., mask]))
    prm = {"r0": rng.normal(size=(3, n)), "q": rng.normal(size=(2, n)), "rC": [0.1, 0.2, 0.3], "tau": [[1.0]], "f_scale": np.ones(3)}
    got = r.gather_params(prm)
    assert np.array_equal(got["r0"], prm["r0"][:, mask]) and np.array_equal(got["q"], prm["q"][:, mask])
    assert got["rC"] is prm["rC"] and got["tau"] is prm["tau"] and got["f_scale"] is prm["f_scale"] and "rT" not in got


def test_refusals():
    w = np.array([1, 2, 3], dtype=np.int64)
    with pytest.raises(ValueError, match="n_out"):
        resample(w)
    for bad in (0, -1, 2 ** 31):
        with pytest.raises(ValueError, match="n_out"):
            resample(w, bad)
    with pytest.raises(ValueError, match=r"outside \[0, 2\^32\]"):
        resample(np.array([1, -2, 3], dtype=np.int64), 4)
    with pytest.raises(ValueError, match=r"outside \[0, 2\^32\]"):
        resample(np.array([1, W_ONE + 1], dtype=np.int64), 4)
    assert resample(np.array([1, W_ONE], dtype=np.int64), 4).weight_sum == W_ONE + 1
    with pytest.raises(ValueError, match="sum to 0"):
        resample(np.zeros(4, dtype=np.int64), 4)
    with pytest.raises(ValueError, match="sum to 0"):
        resample(np.zeros(4, dtype=bool))
    with pytest.raises(ValueError, match="int64"):
        resample(np.ones(4), 4)
    with pytest.raises(ValueError, match="2\\^31"):
        resample(np.broadcast_to(np.int64(1), (2 ** 31,)), 4)           # a view of one number: nothing of that size is allocated


# ---- the exchange over gloo: world 2 and 3, an empty shard, a zero-mass shard, W == 0 on every rank ------------------------
def _gloo_weights():
    rng = np.random.default_rng(31)
    w = rng.integers(0, W_ONE + 1, size=1001).astype(np.int64)
    w[rng.permutation(1001)[:600]] = 0
    return w


def _gloo_bounds(case, world, n):
    if case == "balanced":
        return [shard_bounds(n, r, world) for r in range(world)]
    return [(0, 0), (0, n)] + [(n, n)] * (world - 2)                       # rank 0 holds nothing: an empty shard first


def _worker(rank, world, port, case, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        w = _gloo_weights()
        if case == "zero_mass":
            w[:shard_bounds(w.size, 0, world)[1]] = 0                      # rank 0's members all weigh 0
        lo, hi = _gloo_bounds(case, world, w.size)[rank]
        out = []
        for M, seed in ((257, None), (3004, 9)):
            r = resample(w[lo:hi], M, seed=seed)
            out.append((r.j0, r.n_members, r.weight_sum, r.offset, (r.src.astype(np.int64) + lo).tolist()))
        m = resample(torch.from_numpy(w[lo:hi] > 0))
        out.append((m.j0, m.n_members, m.weight_sum, m.offset, (m.src.numpy().astype(np.int64) + lo).tolist()))
        zero_raised = False
        try:
            resample(np.zeros(hi - lo, dtype=np.int64), 5)
        except ValueError:
            zero_raised = True                                             # W == 0: on EVERY rank
        range_raised = False
        try:
            resample(np.full(hi - lo, W_ONE + (rank == 1), dtype=np.int64), 5)      # only rank 1's weights are bad
        except ValueError:
            range_raised = True
        try:
            resample(np.ones(hi - lo) if rank == 1 else w[lo:hi], 5)           # only rank 1 hands in another type
            range_raised = False
        except ValueError:
            pass
        q.put((rank, out, zero_raised, range_raised))
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
    return results


@pytest.mark.parametrize("world,case", [(2, "balanced"), (3, "balanced"), (3, "empty_shard"), (2, "zero_mass")])
def test_gloo_rehearsal_gives_the_one_rank_result(world, case):
    w = _gloo_weights()
    if case == "zero_mass":
        w[:shard_bounds(w.size, 0, world)[1]] = 0
    results = {r: (out, z, g) for r, out, z, g in _spawn(_worker, world, case)}
    assert all(z and g for _, z, g in results.values())
    ones = [resample(w, 257), resample(w, 3004, seed=9), resample(w > 0)]
    for i, one in enumerate(ones):
        assert one.src.tolist() == source_list(w.tolist() if i < 2 else (w > 0).astype(int).tolist(), one.n_out, one.offset)
        glued, at = [], 0
        for r in range(world):
            j0, n_mine, W, rho, src = results[r][0][i]
            assert (j0, W, rho) == (at, one.weight_sum, one.offset) and n_mine == len(src)
            glued += src
            at += n_mine
        assert glued == one.src.tolist() and at == one.n_out
    if case == "empty_shard":
        assert results[0][0][0][1] == 0                                    # n_members can be 0


# ---- the C ABI: exported, bound, additive, and validated on the host ------------------------------------------------------
NEW = ["fiveeq_wscan_chunks", "fiveeq_wscan", "fiveeq_resample_pick", "fiveeq_gather_rows_f64", "fiveeq_gather_rows_f32"]


def test_new_symbols_are_exported_and_the_abi_is_additive():
    lib = _capi.load()
    for name in NEW:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    assert lib.fiveeq_abi_version() == _capi.ABI_VERSION == 13
    assert lib.fiveeq_sizeof_model() == ctypes.sizeof(_capi.Model) == 448
    T = _capi.WSCAN_TILE
    assert [lib.fiveeq_wscan_chunks(n) for n in (-1, 0, 1, T, T + 1, 65 * T)] == [0, 0, 2, 2, 4, 130]
    assert any(p.endswith("fiveeq_resample.hpp") for p in _capi.SOURCES)


def test_new_entry_points_validate_on_the_host():
    """Every call returns on the host with an error code: the fake pointers are never dereferenced, nothing is launched."""
    lib = _capi.load()
    p, odd, null = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1001), None
    E = _capi.E_INVALID
    err = lambda: lib.fiveeq_last_error().decode()   # noqa: E731
    # scan (n, weights, partial, cum, flags)
    good = [8, p, p, p, p, None]
    for at in (1, 2, 3, 4):
        bad = list(good)
        bad[at] = null
        assert lib.fiveeq_wscan(*bad) == E and "NULL" in err(), at
        bad[at] = odd
        assert lib.fiveeq_wscan(*bad) == E and "aligned" in err(), at
    assert lib.fiveeq_wscan(0, p, p, p, p, None) == E and "n_members" in err()
    assert lib.fiveeq_wscan(2 ** 31, p, p, p, p, None) == E and "n_members" in err()
    # pick (n, cum, c_lo, M, q, a, s, b, j0, n_out, src)
    pick = lambda n=8, cum=p, c_lo=0, M=10, q=3, a=0, s=1, b=2, j0=0, n_out=4, src=p: lib.fiveeq_resample_pick(   # noqa: E731
        n, cum, c_lo, M, q, a, s, b, j0, n_out, src, None)
    assert pick(n=0) == E and "n_members" in err()
    assert pick(cum=null) == E and "NULL" in err() and pick(src=null) == E and "NULL" in err()
    assert pick(cum=odd) == E and "aligned" in err() and pick(src=ctypes.c_void_p(0x1002)) == E and "aligned" in err()
    for M in (0, -1, 2 ** 31):
        assert pick(M=M, s=0, b=0, n_out=0) == E and "M=" in err()
    for kw in (dict(s=-1), dict(s=10), dict(b=-1), dict(b=10)):
        assert pick(**kw) == E and "outside [0, M" in err(), kw
    assert pick(j0=-1) == E and "j0=" in err() and pick(n_out=-1) == E and "n_out=" in err()
    assert pick(j0=8, n_out=3) == E and pick(q=-1) == E and pick(a=-1) == E
    assert pick(M=2 ** 31 - 1, q=2 ** 33, s=0, b=0) == E and "2^63" in err()
    assert pick(n_out=0, cum=null, src=null) == _capi.OK                      # nothing to do
    assert pick(M=2 ** 31 - 1, q=I64 // (2 ** 31 - 1), a=0, s=I64 % (2 ** 31 - 1), b=0, j0=2 ** 31 - 1, n_out=0) == _capi.OK
    # gather (n_rows, n_out, ld_in, rows_in, ld_out, rows_out, src)
    for sfx, el in (("f64", 8), ("f32", 4)):
        g = getattr(lib, f"fiveeq_gather_rows_{sfx}")
        good = [3, 8, 8, p, 8, p, p, None]
        for at in (3, 5, 6):
            bad = list(good)
            bad[at] = null
            assert g(*bad) == E and "NULL" in err(), at
            bad[at] = ctypes.c_void_p(0x1000 + (2 if at == 6 else el // 2))
            assert g(*bad) == E and "aligned" in err(), at
        assert g(-1, 8, 8, p, 8, p, p, None) == E and "n_rows" in err()
        assert g(3, -1, 8, p, 8, p, p, None) == E and "n_out" in err()
        assert g(3, 8, 0, p, 8, p, p, None) == E and "ld_in" in err()
        assert g(3, 8, 8, p, 7, p, p, None) == E and "ld_out" in err()
        assert g(3, 0, 8, null, 0, null, null, None) == _capi.OK and g(0, 8, 8, null, 8, null, null, None) == _capi.OK
