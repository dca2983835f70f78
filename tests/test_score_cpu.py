"""Scoring stored rows without a GPU: the C ABI (exported, bound, additive, validated on the host), Observations.absolute and
anomaly=False, the NumPy twin of the kernel against the independent reference (tests/score_reference.py), and the host side of
constrain.score_rows / EnsembleEngine.score under _score_host.host_passes().  Every comparison is on bits."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from fiveeqscm_amd import _capi, _score_host
from fiveeqscm_amd.constrain import W_ONE, Observations, Score, chi2_from_misfit, importance_weights, score_rows
from fiveeqscm_amd.engine import EnsembleEngine
from score_reference import make_rows, make_table, reference

NEW = ["fiveeq_max_score_quantities", "fiveeq_score_tile", "fiveeq_score_unroll", "fiveeq_score_rows_f64", "fiveeq_score_rows_f32"]
N_STEPS = 40


def test_new_symbols_are_exported_and_the_abi_is_additive():
    lib = _capi.load()
    for name in NEW:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    assert lib.fiveeq_abi_version() == _capi.ABI_VERSION == 13
    assert lib.fiveeq_sizeof_model() == ctypes.sizeof(_capi.Model) == 448
    assert lib.fiveeq_max_score_quantities() == _capi.MAX_SCORE_Q == 4
    assert any(p.endswith("fiveeq_score.hpp") for p in _capi.SOURCES)
    with open(os.path.join(os.path.dirname(_capi.SOURCES[0]), "Makefile")) as fh:
        assert "fiveeq_score.hpp" in fh.read()
    assert (lib.fiveeq_score_tile(8), lib.fiveeq_score_tile(4), lib.fiveeq_score_tile(2)) == (_capi.SCORE_TILE_F64, _capi.SCORE_TILE_F32, 0)
    assert (lib.fiveeq_score_unroll(1), lib.fiveeq_score_unroll(0)) == (_capi.SCORE_UNROLL, _capi.SCORE_UNROLL_NARROW)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_the_entry_points_validate_on_the_host(sfx):
    """Every call returns on the host with an error code: the fake pointers are never dereferenced, nothing is launched."""
    lib = _capi.load()
    fn = getattr(lib, f"fiveeq_score_rows_{sfx}")
    w = 8 if sfx == "f64" else 4
    p = ctypes.c_void_p(0x1000)
    E = _capi.E_INVALID
    err = lambda: lib.fiveeq_last_error().decode()   # noqa: E731

    def call(n_q=2, n_rows=4, n=8, rows=p, row_stride=16, q_stride=8, steps=p, obs=p, n_steps=10, misfit=p, ld_m=8):
        return fn(n_q, n_rows, n, rows, row_stride, q_stride, steps, obs, n_steps, misfit, ld_m, None)

    for n_q in (0, -1, 5):
        assert call(n_q=n_q) == E and "n_q" in err()
    assert call(n_rows=-1) == E and "n_rows" in err()
    assert call(n=0) == E and "n_members" in err()
    assert call(n=2 ** 31, ld_m=2 ** 31, row_stride=2 ** 32, q_stride=2 ** 31) == E and "n_members" in err()
    assert call(ld_m=7) == E and "ld_m" in err()
    for q_stride in (7, -7, 0):
        assert call(q_stride=q_stride) == E and "q_stride" in err()
    for row_stride in (7, 0, -16):
        assert call(row_stride=row_stride) == E and "row_stride" in err()
    for n_steps in (0, -3):
        assert call(n_steps=n_steps) == E and "n_steps" in err()
    for kw, needle in [(dict(rows=None), "rows"), (dict(steps=None), "steps"), (dict(obs=None), "obs"), (dict(misfit=None), "misfit")]:
        assert call(**kw) == E and needle in err() and "NULL" in err(), kw
    odd = lambda k: ctypes.c_void_p(0x1000 + k)   # noqa: E731
    for kw, needle in [(dict(rows=odd(w // 2)), "rows"), (dict(steps=odd(2)), "steps"), (dict(obs=odd(4)), "obs"),
                       (dict(misfit=odd(4)), "misfit")]:
        assert call(**kw) == E and needle in err() and "aligned" in err(), kw
    # what is NOT an error: the strides a call does not use, and no rows at all (rows / steps may then be NULL) — nothing is launched
    assert call(n_rows=0, rows=None, steps=None) == _capi.OK
    assert call(n_rows=0, n_q=1, q_stride=0, row_stride=0) == _capi.OK
    assert call(n_rows=0, q_stride=-8) == _capi.OK
    assert call(n_rows=0, misfit=None) == E and call(n_rows=0, obs=None) == E


# ---- Observations.absolute and anomaly=False -----------------------------------------------------------------------------------
def test_absolute_records_and_the_anomaly_switch():
    years = np.arange(1850, 1850 + N_STEPS)
    oy, vals, sg = np.array([1860, 1875, 1889]), np.array([286.0, 289.5, 294.0]), np.array([1.0, 0.5, 0.25])
    obs = Observations.absolute(years, oy, vals, sg)
    want = np.zeros((N_STEPS, 4))
    want[[10, 25, 39], 0], want[[10, 25, 39], 1] = vals, 1.0 / (sg * sg)
    assert np.array_equal(obs.table, want) and obs.anomaly is False
    assert obs.P == float(np.sum(want[:, 1])) == 1.0 + 4.0 + 16.0 and obs.n_obs == 3 and obs.window == (10, 40)
    import hashlib
    assert obs.sha256 == hashlib.sha256(want.tobytes()).hexdigest()
    assert np.array_equal(obs.live_steps, [10, 25, 39])
    assert np.array_equal(Observations(want, anomaly=False).table, want)
    # from_years' year matching and checks
    with pytest.raises(ValueError, match="not steps of the run"):
        Observations.absolute(years, [1849], [1.0], 1.0)
    with pytest.raises(ValueError, match="appears twice"):
        Observations.absolute(years, [1860, 1860], [1.0, 2.0], 1.0)
    with pytest.raises(ValueError, match="sigma must be > 0"):
        Observations.absolute(years, [1860], [1.0], 0.0)
    with pytest.raises(ValueError, match="values has 2 values for 1 years"):
        Observations.absolute(years, [1860], [1.0, 2.0], 1.0)
    with pytest.raises(ValueError, match="non-finite"):
        Observations.absolute(years, [1860], [np.nan], 1.0)
    # b != 0 is refused with anomaly=False; the default constructor still refuses an empty baseline, and keeps its sha256
    with_b = want.copy()
    with_b[3, 2] = 1.0
    with pytest.raises(ValueError, match="anomaly=False"):
        Observations(with_b, anomaly=False)
    with pytest.raises(ValueError, match="empty baseline"):
        Observations(want)
    with pytest.raises(ValueError, match="no observation"):
        Observations(np.zeros((4, 4)), anomaly=False)
    dflt = Observations(with_b)
    assert dflt.anomaly is True and dflt.sha256 == hashlib.sha256(with_b.tobytes()).hexdigest() and dflt.window == (3, 40)
    fy = Observations.from_years(years, oy, vals, sg, baseline=(1850, 1859))
    assert np.array_equal(fy.table[:, :2], want[:, :2]) and np.array_equal(fy.table[:10, 2], np.full(10, 0.1)) and not fy.table[10:, 2].any()
    with pytest.raises(ValueError, match="T_obs has 2 values for 1 years"):
        Observations.from_years(years, [1860], [1.0, 2.0], 1.0, baseline=(1850, 1859))


# ---- the NumPy twin against the reference -------------------------------------------------------------------------------------
SENT = -777.25


def _twin(x, steps, tables, *, ld, off, ld_m, acc=None):
    """The twin through its pointer signature on rows in the C layout [K][Q][ld], base `off` elements off; sentinel padding
    and guard rows around misfit."""
    K, Q, N = x.shape
    host = np.full(off + K * Q * ld + 1, np.nan, dtype=x.dtype)
    host[off:off + K * Q * ld].reshape(K, Q, ld)[:, :, :N] = x
    st = np.asarray(steps, dtype=np.int32)
    ob = np.stack([np.asarray(t) for t in tables])
    mis = np.full((Q * 3 + 2, ld_m), SENT)
    mis[1:-1, :N] = 0.0 if acc is None else np.asarray(acc).reshape(Q * 3, N)
    fn = getattr(_score_host.ScorePasses(), "fiveeq_score_rows_f64" if x.dtype == np.float64 else "fiveeq_score_rows_f32")
    assert fn(Q, K, N, host.ctypes.data + off * host.itemsize, Q * ld, ld, st.ctypes.data, ob.ctypes.data, ob.shape[1],
              mis[1:].ctypes.data, ld_m, None) == 0
    assert np.all(mis[0] == SENT) and np.all(mis[-1] == SENT) and np.all(mis[:, N:] == SENT)
    return mis[1:-1, :N].reshape(Q, 3, N).copy()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_host_twin_equals_the_reference(dtype):
    for K, Q, N, off in [(1, 1, 1, 0), (7, 3, 5, 1), (N_STEPS, 4, 33, 0)]:
        steps = np.sort(np.random.default_rng(K).choice(N_STEPS, K, replace=False))
        obs = [make_table(N_STEPS, 10 + j, live_every=1 + j, baseline=(2 * j, 2 * j + 6), anomaly=j != 1) for j in range(Q)]
        tabs = [o.table for o in obs]
        x = make_rows(K, Q, N, dtype, K + N)
        want = reference(x, steps, tabs)
        got = _twin(x, steps, tabs, ld=N + 3, off=off, ld_m=N + 2)
        assert np.array_equal(got, want), (K, Q, N)
        if K > 2:                                              # rows [0, k) then [k, K) through the accumulators
            first = _twin(x[:3], steps[:3], tabs, ld=N + 3, off=off, ld_m=N)
            assert np.array_equal(_twin(x[3:], steps[3:], tabs, ld=N, off=0, ld_m=N + 1, acc=first), want)


def test_the_twin_on_nan_rows_and_dead_records():
    K, Q, N = 20, 2, 6
    steps = np.arange(K) * 2
    live5 = make_table(N_STEPS, 1, live_every=5, baseline=(10, 14))
    dead = np.zeros((N_STEPS, 4))
    x = make_rows(K, Q, N, np.float64, 3)
    rec = live5.table[steps]
    dead_rows = ~((rec[:, 1] != 0) | (rec[:, 2] != 0))
    assert dead_rows.any() and (~dead_rows).sum() >= 4
    planted = x.copy()
    planted[dead_rows, 0] = np.nan
    planted[:, 1] = np.inf                                       # quantity 1: every record dead
    start = np.arange(Q * 3 * N, dtype=np.float64).reshape(Q, 3, N) + 1.0
    got = _twin(planted, steps, [live5.table, dead], ld=N, off=0, ld_m=N, acc=start)
    assert np.array_equal(got[0], reference(x[~dead_rows, 0], steps[~dead_rows], live5.table, acc=start[0]))
    assert np.array_equal(got[1], start[1]) and np.isfinite(got).all()
    # a NaN at a live element: that member's accumulators of that quantity, and nothing else
    k_obs = int(np.nonzero(rec[:, 1] != 0)[0][0])
    hit = x.copy()
    hit[k_obs, 0, 2] = np.nan
    got2 = _twin(hit, steps, [live5.table, live5.table], ld=N, off=0, ld_m=N)
    clean = reference(x, steps, [live5.table, live5.table])
    assert np.isnan(got2[0, 1:, 2]).all()
    mask = np.ones((Q, 3, N), dtype=bool)
    mask[0, :, 2] = False
    assert np.array_equal(got2[mask], clean[mask])
    assert np.array_equal(got2, reference(hit, steps, [live5.table, live5.table]), equal_nan=True)


# ---- constrain.score_rows on host tensors, through the twin --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_score_rows_host_side(dtype):
    K, G, N = 12, 3, 9
    steps = np.arange(3, 3 + 2 * K, 2)
    obs = [make_table(N_STEPS, 20 + j, live_every=2 + j, baseline=(3 + j, 12 + j), anomaly=j != 2, lo=1) for j in range(G)]
    tabs = [o.table for o in obs]
    ld = N + 4
    buf = torch.full((K, G, ld), float("nan"), dtype=torch.from_numpy(np.zeros(1, dtype)).dtype)
    C = buf[:, :, 1:1 + N]                                       # the engine's C layout seen through a member slice
    C.copy_(torch.from_numpy(make_rows(K, G, N, dtype, 5)))
    x = C.numpy()
    with _score_host.host_passes():
        got3 = score_rows(C, steps, obs)
        assert got3.shape == (G, 3, N) and got3.dtype == torch.float64
        assert np.array_equal(got3.numpy(), reference(x, steps, tabs))
        # 2-D rows: one gas of the block, a strided view read in place
        got2 = score_rows(C[:, 1], steps, obs[1])
        assert got2.shape == (3, N) and np.array_equal(got2.numpy(), got3[1].numpy())
        # gases 0 and 2 through a strided quantity axis; a transposed (copied) view; one row; no rows
        assert np.array_equal(score_rows(C[:, 0::2], steps, [obs[0], obs[2]]).numpy(), got3[0::2].numpy())
        Tt = C[:, 0].t().contiguous().t()
        assert Tt.stride(1) != 1 and np.array_equal(score_rows(Tt, steps, obs[0]).numpy(), got3[0].numpy())
        assert np.array_equal(score_rows(C[4:5], steps[4:5], obs).numpy(), reference(x[4:5], steps[4:5], tabs))
        assert not score_rows(C[:0], steps[:0], obs).any()
        # acc= continues earlier rows, and is not written
        head = score_rows(C[:5], steps[:5], obs)
        keep = head.clone()
        assert np.array_equal(score_rows(C[5:], steps[5:], obs, acc=head).numpy(), got3.numpy()) and torch.equal(head, keep)
        assert np.array_equal(score_rows(C[5:, 1], steps[5:], obs[1], acc=head[1]).numpy(), got3[1].numpy())
        # the refusals
        with pytest.raises(ValueError, match="equal n_steps"):
            score_rows(C, steps, [obs[0], obs[1], make_table(N_STEPS + 1, 1)])
        for bad in (steps[::-1].copy(), np.r_[steps[:-1], steps[-2]]):
            with pytest.raises(ValueError, match="strictly increasing"):
                score_rows(C, bad, obs)
        for bad in (np.r_[-1, steps[1:]], np.r_[steps[:-1], N_STEPS]):
            with pytest.raises(ValueError, match="outside the tables"):
                score_rows(C, bad, obs)
        with pytest.raises(ValueError, match="one per row"):
            score_rows(C, steps[:-1], obs)
        with pytest.raises(ValueError, match="quantities"):
            score_rows(C, steps, obs[:2])
        with pytest.raises(ValueError, match="rows: want"):
            score_rows(C[:, 0], steps, obs[:1])
        with pytest.raises(ValueError, match="acc: want"):
            score_rows(C, steps, obs, acc=head[0])
        with pytest.raises(TypeError, match="fp32 / fp64"):
            score_rows(C.to(torch.float16), steps, obs)
    with pytest.raises(TypeError, match="no CPU fallback"):       # outside the switch host rows are refused
        score_rows(C, steps, obs)


def _stub(T, C, out_steps, n_steps, **kw):
    eng = types.SimpleNamespace(T=T, C=C, out_steps=np.asarray(out_steps), n_steps=n_steps, n_gas=3,
                                scenario_axis=False, n_scenarios=1, concentration_driven=False, _ps_unjoined=None)
    eng.__dict__.update(kw)
    eng._scen = types.MethodType(EnsembleEngine._scen, eng)
    return eng


def test_engine_score_on_a_stub():
    K, G, N = 19, 3, 7
    out_steps = np.arange(2, 2 + 2 * K, 2)                        # the even steps 2..38
    T = torch.from_numpy(make_rows(K, 1, N, np.float64, 1)[:, 0])
    C = torch.from_numpy(make_rows(K, G, N, np.float32, 2) + 280.0)
    eng = _stub(T, C, out_steps, N_STEPS)

    def even(seed, anomaly):
        return make_table(N_STEPS, seed, live_every=4, baseline=(4, 12), anomaly=anomaly, lo=2)
    recT, rec0, rec2 = even(1, True), even(2, False), even(3, False)
    tabT = recT.table.copy()
    tabT[5:12:2, 2] = 0.0                                         # the baseline on stored steps only
    recT = Observations(tabT)
    with _score_host.host_passes():
        s = EnsembleEngine.score(eng, {2: rec2, "T": recT, 0: rec0})
        assert isinstance(s, Score) and list(s.chi2) == ["T", 0, 2] and set(s.misfit) == {"T", 0, 2}
        assert np.array_equal(s.misfit["T"].numpy(), reference(T.numpy(), out_steps, recT.table))
        for g, rec in ((0, rec0), (2, rec2)):
            assert np.array_equal(s.misfit[g].numpy(), reference(C[:, g].numpy(), out_steps, rec.table))
            assert not s.misfit[g][0].any() and torch.equal(s.chi2[g], s.misfit[g][2])          # anomaly=False: A = 0, chi2 = V
        assert torch.equal(s.chi2["T"], chi2_from_misfit(s.misfit["T"], recT.P))
        assert torch.equal(s.total, (s.chi2["T"] + s.chi2[0]) + s.chi2[2])
        assert s.n_obs == {"T": recT.n_obs, 0: rec0.n_obs, 2: rec2.n_obs}
        w = importance_weights(s.total)
        assert int(w.max()) == W_ONE and int(w[int(torch.argmin(s.total))]) == W_ONE
        one = EnsembleEngine.score(eng, {1: rec0})
        assert list(one.chi2) == [1] and torch.equal(one.total, one.chi2[1])
        # a live step that is not stored: named, never a partial chi2
        odd = make_table(N_STEPS, 4, live_every=2, anomaly=False, lo=1)
        with pytest.raises(ValueError, match=r"not stored steps.*first \[1, 3, 5, 7, 9\]"):
            EnsembleEngine.score(eng, {"T": recT, 0: odd})
        with pytest.raises(ValueError, match="need stored concentrations"):
            EnsembleEngine.score(_stub(T, None, out_steps, N_STEPS), {"T": recT, 0: rec0})
        with pytest.raises(ValueError, match="need stored concentrations"):
            EnsembleEngine.score(_stub(T, C, out_steps, N_STEPS, concentration_driven=True), {0: rec0})
        with pytest.raises(ValueError, match="pass scenario="):
            EnsembleEngine.score(_stub(T[None], C[None], out_steps, N_STEPS, scenario_axis=True, n_scenarios=1), {"T": recT})
        sc = EnsembleEngine.score(_stub(T[None], C[None], out_steps, N_STEPS, scenario_axis=True, n_scenarios=1), {"T": recT, 2: rec2},
                                  scenario=0)
        assert torch.equal(sc.total, s.chi2["T"] + s.chi2[2])
        for bad in ({}, {"C": recT}, {3: rec0}, {True: rec0}, {0: rec0.table}):
            with pytest.raises(ValueError, match="records"):
                EnsembleEngine.score(eng, bad)
        with pytest.raises(ValueError, match="steps for a run of"):
            EnsembleEngine.score(eng, {"T": make_table(N_STEPS + 1, 1)})
        with pytest.raises(ValueError, match="no stored rows"):
            EnsembleEngine.score(_stub(None, None, out_steps[:0], N_STEPS), {"T": recT})
