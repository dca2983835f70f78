"""Scoring stored rows on the MI355X (include/fiveeq.h, "SCORING STORED ROWS"): the pass against the in-loop misfit, against
the NumPy reference (tests/score_reference.py) at the kernel's edges, under row and member splits, with dead records, NaN
isolation, and on engines the in-loop form cannot serve.  Every comparison is on bits; every case has n_steps <= 48."""
import ctypes

import numpy as np
import pytest
import torch

from fiveeqscm_amd import _capi, emissions
from fiveeqscm_amd import params as prm
from fiveeqscm_amd.constrain import W_ONE, Observations, chi2_from_misfit, importance_weights, score_rows
from fiveeqscm_amd.engine import EnsembleEngine
from score_reference import make_rows, make_table, reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_STEPS = 48
TORCH = {np.float64: torch.float64, np.float32: torch.float32}


def _tile(dtype):
    return _capi.load().fiveeq_score_tile(np.dtype(dtype).itemsize)


def _unroll(wide):
    return _capi.load().fiveeq_score_unroll(1 if wide else 0)


def _lay_out(x, wide):
    """x [K, Q, N] host -> a device view of the same values in the C layout [K][Q][ld], NaN in the padding.  wide: base and
    strides multiples of 16 bytes (the 16-byte loads, and the element loads on a ragged tail); else a base one element off and
    an odd ld (the element loads throughout)."""
    K, Q, N = x.shape
    per16 = 16 // x.dtype.itemsize
    ld = (N + per16 - 1) // per16 * per16 + per16 if wide else (N + 2) | 1
    off = 0 if wide else 1
    flat = torch.full((off + K * Q * ld,), float("nan"), dtype=TORCH[x.dtype.type], device=DEV)
    view = flat[off:].view(K, Q, ld)[:, :, :N]
    view.copy_(torch.from_numpy(x))
    assert (view.data_ptr() % 16 == 0) == wide and view.stride() == (Q * ld, ld, 1)
    return view


# ---- 1. the pass equals the in-loop misfit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["co2", "multigas"])
def test_equals_the_in_loop_misfit(kind, dtype):
    N = _tile(np.float64 if dtype == torch.float64 else np.float32) + 3
    G = 1 if kind == "co2" else 3
    p = prm.sample_ensemble(prm.default_params(kind), N, seed=5)
    E = emissions.rcp_like_emissions(750, G)[230:230 + N_STEPS]
    anomaly = make_table(N_STEPS, 1, live_every=3, baseline=(4, 15), lo=20)
    absolute = make_table(N_STEPS, 2, live_every=2, anomaly=False, lo=7)
    for rec in (anomaly, absolute):
        for mode in ("per_step", "fused"):
            eng = EnsembleEngine(p, N, E, observations=rec, dtype=dtype, device=DEV)
            eng.run(mode=mode)
            torch.cuda.synchronize()
            assert np.array_equal(eng.out_steps, np.arange(N_STEPS)) and bool(eng.misfit[1:].abs().sum() > 0)
            got = score_rows(eng.T, eng.out_steps, rec)
            assert torch.equal(got, eng.misfit), (kind, dtype, mode, rec.anomaly)
            if not rec.anomaly:
                assert not bool(got[0].any()) and torch.equal(eng.chi2(), got[2])
            s = eng.score({"T": rec})
            assert torch.equal(s.misfit["T"], eng.misfit) and torch.equal(s.total, eng.chi2())
            eng.close()


# ---- 2. the pass equals the NumPy reference at the kernel's edges -------------------------------------------------------------
@pytest.mark.parametrize("wide", [True, False], ids=["16-byte", "element"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_equals_the_reference_at_the_edges(dtype, wide):
    tile, U = _tile(dtype), _unroll(wide)
    obs = [make_table(N_STEPS, 30 + j, live_every=1, baseline=(3 * j, 3 * j + 9), anomaly=j != 2) for j in range(4)]
    for N in (1, tile - 1, tile, tile + 1, 2 * tile + 5):
        for K in (1, U - 1, U, U + 1, 3 * U + 2):
            steps = np.arange(K) + (N_STEPS - K) // 2
            for Q in (1, 3, 4):
                x = make_rows(K, Q, N, dtype, 7 * K + Q)
                got = score_rows(_lay_out(x, wide), steps, obs[:Q])
                want = reference(x, steps, [o.table for o in obs[:Q]])
                assert got.shape == (Q, 3, N) and np.array_equal(got.cpu().numpy(), want), (N, K, Q)


# ---- 3. splits of the rows and of the members ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_row_and_member_splits_equal_one_call(dtype):
    tile, U = _tile(dtype), _unroll(True)
    K, Q, N = 2 * U + 3, 3, 2 * tile + 5
    steps = np.arange(K) * 2 + 1
    obs = [make_table(N_STEPS, 40 + j, live_every=1 + j, baseline=(1, 11), anomaly=j != 1, lo=1) for j in range(Q)]
    x = make_rows(K, Q, N, dtype, 11)
    rows = _lay_out(x, True)
    whole = score_rows(rows, steps, obs)
    assert np.array_equal(whole.cpu().numpy(), reference(x, steps, [o.table for o in obs]))
    for k in (1, U, K - 1):
        head = score_rows(rows[:k], steps[:k], obs)
        assert torch.equal(score_rows(rows[k:], steps[k:], obs, acc=head), whole), k
    for cut in (1, tile, tile + 1):
        assert torch.equal(score_rows(rows[:, :, :cut], steps, obs), whole[:, :, :cut]), cut
        assert torch.equal(score_rows(rows[:, :, cut:], steps, obs), whole[:, :, cut:]), cut
    assert torch.equal(score_rows(rows[:, 1], steps, obs[1]), whole[1])


# ---- 4. dead records ----------------------------------------------------------------------------------------------------------
def _raw(view, steps, tables, misfit, ld_m):
    """The C entry point on a row view [K, Q, N] (C layout), device tables [Q, n_steps, 4] and a caller's misfit block."""
    lib = _capi.load()
    K, Q, N = view.shape
    fn = lib.fiveeq_score_rows_f64 if view.dtype == torch.float64 else lib.fiveeq_score_rows_f32
    st = torch.from_numpy(np.asarray(steps, dtype=np.int32)).to(DEV)
    ob = torch.from_numpy(np.stack(tables)).to(DEV)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    _capi.check(lib, fn(Q, K, N, ptr(view), view.stride(0), view.stride(1), ptr(st), ptr(ob), ob.shape[1], ptr(misfit), ld_m,
                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dead_records_are_neither_read_nor_scored(dtype):
    tile = _tile(dtype)
    K, Q, N = N_STEPS, 3, tile + 1
    steps = np.arange(K)
    # live on every fifth step and in one baseline block; each quantity its own live set
    obs = [make_table(N_STEPS, 50 + j, live_every=5, baseline=(8 + 9 * j, 14 + 9 * j), anomaly=j != 2, lo=j) for j in range(Q)]
    tabs = [o.table for o in obs]
    x = make_rows(K, Q, N, dtype, 13)
    planted = x.copy()
    n_dead = 0
    for j in range(Q):
        dead = (tabs[j][:, 1] == 0) & (tabs[j][:, 2] == 0)
        planted[dead, j, 0::2], planted[dead, j, 1::2] = np.nan, np.inf
        n_dead += int(dead.sum())
    assert n_dead > Q * K // 2 and len({tuple(o.live_steps) for o in obs}) == Q
    clean = reference(np.where(np.isfinite(planted), x, 0), steps, tabs)     # the planted rows do not reach it: dropped as dead
    assert np.isfinite(clean).all() and np.array_equal(clean, reference(x, steps, tabs))
    got = score_rows(_lay_out(planted, True), steps, obs)
    assert np.array_equal(got.cpu().numpy(), clean)
    # an all-dead table leaves a non-zero misfit untouched, whatever the rows hold
    start = torch.arange(Q * 3 * N, dtype=torch.float64, device=DEV).reshape(Q, 3, N) + 0.5
    block = start.clone()
    _raw(_lay_out(planted, True), steps, [np.zeros((N_STEPS, 4))] * Q, block, N)
    assert torch.equal(block, start)
    block = start.clone()
    _raw(_lay_out(planted, False), steps, [tabs[0], np.zeros((N_STEPS, 4)), tabs[2]], block, N)
    assert torch.equal(block[1], start[1]) and not torch.equal(block[0], start[0])
    assert np.array_equal(block.cpu().numpy()[0::2], reference(x[:, 0::2], steps, tabs[0::2], acc=start.cpu().numpy()[0::2]))


# ---- 5. isolation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [True, False], ids=["16-byte", "element"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_nan_and_the_padding_stay_where_they_are(dtype, wide):
    tile = _tile(dtype)
    K, Q, N, ld_m = 12, 2, tile + 2, tile + 9
    steps = np.arange(K) + 10
    obs = [make_table(N_STEPS, 60 + j, live_every=2, baseline=(10, 16), lo=10) for j in range(Q)]
    tabs = [o.table for o in obs]
    x = make_rows(K, Q, N, dtype, 17)
    clean = reference(x, steps, tabs)
    hit = x.copy()
    member = tile - 1
    hit[4, 1, member] = np.nan                                    # step 14: observed and inside the baseline
    SENT = -777.25
    buf = torch.full((Q * 3 + 2, ld_m), SENT, dtype=torch.float64, device=DEV)
    buf[1:-1, :N] = 0.0
    _raw(_lay_out(hit, wide), steps, tabs, buf[1:], ld_m)
    host = buf.cpu().numpy()
    assert np.all(host[0] == SENT) and np.all(host[-1] == SENT) and np.all(host[:, N:] == SENT)
    got = host[1:-1, :N].reshape(Q, 3, N)
    assert np.isnan(got[1, :, member]).all()
    mask = np.ones((Q, 3, N), dtype=bool)
    mask[1, :, member] = False
    assert np.array_equal(got[mask], clean[mask]) and np.isfinite(got[mask]).all()
    assert np.array_equal(got, reference(hit, steps, tabs), equal_nan=True)


# ---- 6. engines the in-loop form cannot serve ---------------------------------------------------------------------------------
def _two_gas_params():
    """Pools (4, 4): a compiled layout without a misfit form."""
    base = prm.default_params("multigas")
    rng = np.random.default_rng(3)
    a, tau = np.zeros((2, 4)), np.ones((2, 4))
    for g in range(2):
        w = rng.uniform(0.2, 1.0, size=4)
        a[g], tau[g] = w / w.sum(), np.sort(rng.uniform(2.0, 400.0, size=4))[::-1]
    return {"a": a, "tau": tau, "r0": [30.0, 9.0], "rC": [0.015, 0.0], "rT": [3.0, -0.3], "ra": [0.0, 3e-4], "PI_conc": base["PI_conc"][:2],
            "emis2conc": base["emis2conc"][:2], "f": base["f"][:2], "iirf_max": 97.0, "d": base["d"], "q": base["q"]}


@pytest.mark.parametrize("case", ["co2-quad", "octet", "no-misfit-form"])
def test_engines_without_an_in_loop_form_are_scored(case):
    N = 300
    base, G, dtype, kw, mode = {
        "co2-quad": (prm.default_params("co2"), 1, torch.float64, {}, "auto"),
        "octet": (prm.default_params("multigas"), 3, torch.float32, {"small_lanes": 8}, "small"),
        "no-misfit-form": (_two_gas_params(), 2, torch.float64, {}, "fused"),
    }[case]
    p = prm.sample_ensemble(base, N, seed=4)
    E = emissions.rcp_like_emissions(750, G)[230:230 + N_STEPS]
    out_steps = list(range(2, N_STEPS, 2))
    eng = EnsembleEngine(p, N, E, dtype=dtype, device=DEV, output_steps=out_steps, **kw)
    if case == "no-misfit-form":
        with pytest.raises(ValueError, match="no misfit form"):
            EnsembleEngine(p, N, E, dtype=dtype, device=DEV, observations=make_table(N_STEPS, 1))
    eng.run(mode=mode)
    torch.cuda.synchronize()
    if case == "co2-quad":
        assert eng.last_mode == "small" and eng.small_form() == 4
    if case == "octet":
        assert eng.small_form() == 8
    T, C = eng.T.cpu().numpy(), eng.C.cpu().numpy()
    # records on stored steps, around the ensemble's own rows: T as an anomaly, the gases in absolute terms
    rng = np.random.default_rng(8)
    tT = np.zeros((N_STEPS, 4))
    tT[[20, 30, 40], 0] = (T[[9, 14, 19]] - T[[2, 3, 4, 5]].mean(0)).mean(1) + 0.05
    tT[[20, 30, 40], 1] = 1.0 / 0.1 ** 2
    tT[[6, 8, 10, 12], 2] = 0.25
    records = {"T": Observations(tT)}
    for g in ([0] if G == 1 else [0, G - 1]):
        t = np.zeros((N_STEPS, 4))
        rows_g = [4 + 5 * g, 12, 22]
        t[[2 * r + 2 for r in rows_g], 0] = C[rows_g, g].mean(1) * (1.0 + 0.01 * rng.normal(size=3))
        t[[2 * r + 2 for r in rows_g], 1] = 1.0 / (0.01 * C[rows_g, g].mean(1)) ** 2
        records[g] = Observations(t, anomaly=False)
    s = eng.score(records)
    assert list(s.chi2) == ["T"] + sorted(k for k in records if k != "T")
    assert np.array_equal(s.misfit["T"].cpu().numpy(), reference(T, eng.out_steps, records["T"].table))
    total = chi2_from_misfit(s.misfit["T"], records["T"].P)
    for g in sorted(k for k in records if k != "T"):
        assert np.array_equal(s.misfit[g].cpu().numpy(), reference(C[:, g], eng.out_steps, records[g].table))
        assert torch.equal(s.chi2[g], s.misfit[g][2]) and s.n_obs[g] == 3
        total = total + s.chi2[g]
    assert torch.equal(s.total, total) and bool(torch.isfinite(s.total).all()) and bool((s.total > 0).all())
    w = importance_weights(s.total)
    assert int(w[int(torch.argmin(s.total))]) == W_ONE == int(w.max())
    # a record with a live step that is not stored raises, naming it
    tT2 = tT.copy()
    tT2[21, 1] = 1.0
    with pytest.raises(ValueError, match=r"not stored steps.*\[21\]"):
        eng.score({"T": Observations(tT2)})
    if G > 1:
        no_c = EnsembleEngine(p, N, E, dtype=dtype, device=DEV, output_steps=out_steps, store_concentrations=False, **kw)
        with pytest.raises(ValueError, match="need stored concentrations"):
            no_c.score(records)
        no_c.close()
    eng.close()
