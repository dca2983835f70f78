"""The weighted summary on the GPU (include/fiveeq.h, "WEIGHTED SUMMARY"): the four HIP passes under the product's host
logic against the independent reference of tests/weighted_reference.py.  Percentiles, weight_sum, count, min and max must
equal the reference EXACTLY; mean, std and ess within the bounds fp64 summation gives (stated at `_check`).

Shapes: N in {1, 63, 64, 65, 255, 256, 257, 1000, 4097} (below / at / above a wave, a workgroup and one workgroup's 16-byte
strides, several loads per lane, a ragged tail) in rows of a wider buffer (ld > N), one row and three."""
import ctypes
import math

import numpy as np
import pytest
import torch

from fiveeqscm_amd import _capi
from fiveeqscm_amd import distributed as D
from fiveeqscm_amd import params as prm
from fiveeqscm_amd.constrain import W_ONE
from fiveeqscm_amd.distributed import gather_weighted_summary
from weighted_reference import weighted_rows

pytestmark = pytest.mark.gpu

PCT = (0, 5, 50, 95, 100)
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 4097)
WEIGHTS = ("equal", "one_member", "random_half_zero", "at_min", "at_max")
VALUES = ("normal", "constant", "ties", "heavy_tail", "inf_w0", "nan_w0", "nan_weighted")
U = 2.0 ** -53


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): the relative error bound of k successive fp64 roundings."""
    return k * U / (1.0 - k * U)


def _case(n, n_rows, wname, vname, dtype, seed):
    """(rows [n_rows, n] of `dtype`, w [n] int64) for one weight pattern x one value pattern."""
    rng = np.random.default_rng(seed)
    if vname == "constant":
        rows = np.full((n_rows, n), 1.25)
    elif vname == "ties":
        rows = rng.choice([-3.5, -1.0, 0.25, 2.0, 1.0e6], size=(n_rows, n))
    elif vname == "heavy_tail":
        rows = rng.standard_cauchy(size=(n_rows, n)) * 1.0e3
    else:
        rows = rng.normal(1.5, 0.7, size=(n_rows, n))
    rows = rows.astype(dtype)
    if wname == "equal":
        w = np.full(n, 12345, dtype=np.int64)
    elif wname == "one_member":
        w = np.zeros(n, dtype=np.int64)
        w[int(rng.integers(n))] = W_ONE
    elif wname == "random_half_zero":
        w = rng.integers(0, W_ONE + 1, size=n, dtype=np.int64)
        w[rng.uniform(size=n) < 0.5] = 0
        if not w.any():
            w[int(rng.integers(n))] = 1
    else:
        w = np.zeros(n, dtype=np.int64)
        w[int(np.argmin(rows[0]) if wname == "at_min" else np.argmax(rows[0]))] = 3
    keep = int(np.argmax(w))                                   # a member that keeps its weight whatever is injected below
    spare = [i for i in range(n) if i != keep][:2]
    if vname == "inf_w0" and spare:
        w[spare] = 0
        rows[:, spare[0]] = np.inf
        rows[:, spare[-1]] = -np.inf
    elif vname == "nan_w0" and spare:
        w[spare] = 0
        rows[:, spare] = np.nan
    elif vname == "nan_weighted":
        rows[n_rows // 2, keep] = np.nan                       # ONE row holds a NaN that carries weight: the others are unaffected
    return rows, w


def _on_device(rows, w, ld=None):
    """rows as a view [K, n] of a wider device buffer [K, ld] (ld > n; default: the next multiple of 8 — 16-byte aligned
    rows, so the 16-byte loads run), the rest of the buffer poisoned with NaN."""
    K, n = rows.shape
    ld = (n // 8 + 1) * 8 if ld is None else ld
    buf = torch.full((K, ld), float("nan"), dtype=torch.from_numpy(rows).dtype, device="cuda")
    buf[:, :n] = torch.from_numpy(rows).cuda()
    return buf[:, :n], torch.from_numpy(w).cuda()


def _check(s, rows, w, pct=PCT):
    """Exact: percentiles (bit for bit), weight_sum, count, min, max.  Bounded, with n = the members that carry weight:
      sum w x    n products w x rounded once each (w <= 2^32 is exact in fp64), summed in fp64 in some fixed order — at most
                 n - 1 further roundings on any term: |error| <= gamma(n) sum |w x|; the reference rounds its products too and
                 fsum rounds once: gamma(n + 2) sum |w x| in all.  mean = that / float(W): three more roundings of the result.
      sum w x^2  the same with one more rounding per product (w x, then the fused multiply-add with x): gamma(n + 4) sum w x^2.
                 var = s2 / W - mean^2 inherits err(s2) / W + 2 |mean| err(mean) + the roundings of its own four operations
                 on numbers of size s2 / W, here and in the reference: gamma(8) sum w x^2 / W; std = sqrt(var) turns an error e of var into e / (2 std) — or sqrt(e) at most
                 where std is smaller than that (|sqrt(a) - sqrt(b)| <= sqrt(|a - b|)).
      ess        sum w^2 of positive terms: relative error gamma(n); float(W) twice, a product, a division, and the
                 reference's own rounding: gamma(n + 6) ess."""
    ref = weighted_rows(rows, w, pct)
    got = s["percentiles"].cpu().numpy()
    assert s["method"] == "weighted_inverted_cdf"
    for k, r in enumerate(ref):
        same = (got[k].view(np.int64) == r["percentiles"].view(np.int64)) | (np.isnan(got[k]) & np.isnan(r["percentiles"]))
        assert same.all(), (k, got[k], r["percentiles"])
        assert s["weight_sum"] == r["weight_sum"] and isinstance(s["weight_sum"], int)
        assert int(s["count"][k]) == r["count"]
        assert float(s["min"][k]) == r["min"] and float(s["max"][k]) == r["max"]
        n, W = r["count"], r["weight_sum"]
        assert abs(s["ess"] - r["ess"]) <= gamma(n + 6) * r["ess"]
        if math.isnan(r["mean"]):
            assert math.isnan(float(s["mean"][k])) and math.isnan(float(s["std"][k]))
            continue
        e_mean = gamma(n + 2) * r["sum_abs_wx"] / W + gamma(3) * abs(r["mean"])
        assert abs(float(s["mean"][k]) - r["mean"]) <= e_mean, (k, float(s["mean"][k]), r["mean"], e_mean)
        e_var = gamma(n + 4) * r["sum_abs_wx2"] / W + 2 * abs(r["mean"]) * e_mean + e_mean ** 2 + gamma(8) * r["sum_abs_wx2"] / W
        e_std = e_var / (2 * r["std"]) if r["std"] > 0 and e_var < r["std"] ** 2 else math.sqrt(e_var)
        assert abs(float(s["std"][k]) - r["std"]) <= e_std + gamma(2) * r["std"], (k, float(s["std"][k]), r["std"], e_std)


@pytest.mark.parametrize("n_rows", [1, 3])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_weighted_summary_equals_the_reference(dtype, n, n_rows):
    for wi, wname in enumerate(WEIGHTS):
        for vi, vname in enumerate(VALUES):
            rows, w = _case(n, n_rows, wname, vname, dtype, seed=1000 * n + 10 * wi + vi)
            x, wd = _on_device(rows, w)
            s = gather_weighted_summary(x, wd, PCT)
            try:
                _check(s, rows, w)
            except AssertionError as exc:
                raise AssertionError(f"weights={wname} values={vname}: {exc}") from exc


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_unaligned_rows_and_weights_take_the_narrow_loads(dtype):
    """ld = n + 1 (rows off the 16-byte grid) and a weight vector that starts 8 bytes into its buffer."""
    for n in (65, 1000, 4097):
        rows, w = _case(n, 3, "random_half_zero", "normal", dtype, seed=n)
        x, _ = _on_device(rows, w, ld=n + 1)
        wbuf = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        wbuf[1:] = torch.from_numpy(w).cuda()
        _check(gather_weighted_summary(x, wbuf[1:], PCT), rows, w)


def test_every_member_in_one_bin_and_fractional_percentiles():
    """A far outlier squeezes every other member into bin 0: the candidate set of most percentiles is the whole row, and the
    pick pass alone finds them.  Percentiles that are no integers exercise the rational rank."""
    n = 4097
    rng = np.random.default_rng(77)
    rows = rng.normal(size=(3, n))
    rows[:, 5] = 1.0e15
    w = rng.integers(1, W_ONE + 1, size=n, dtype=np.int64)
    pct = (0, 0.1, 2.5, 33.3, 50, 99.9, 100)
    for dtype in (np.float64, np.float32):
        x, wd = _on_device(rows.astype(dtype), w)
        _check(gather_weighted_summary(x, wd, pct), rows.astype(dtype), w, pct)


def test_bad_weights_are_refused():
    x = torch.randn(2, 100, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="sum to 0"):
        gather_weighted_summary(x, torch.zeros(100, dtype=torch.int64, device="cuda"), PCT)
    with pytest.raises(ValueError, match="outside"):
        gather_weighted_summary(x, torch.full((100,), W_ONE + 1, dtype=torch.int64, device="cuda"), PCT)
    with pytest.raises(ValueError, match="int64"):
        gather_weighted_summary(x, torch.ones(100, dtype=torch.int32, device="cuda"), PCT)
    with pytest.raises(ValueError, match="int64"):
        gather_weighted_summary(x, torch.ones(100, dtype=torch.int64), PCT)               # weights on the host


# ---- shard invariance on one GPU: two "ranks" through the device passes, merged by hand -----------------------------------
def _two_shards_by_hand(x, wd, a, pct):
    """Members [0, a) and [a, n) as two ranks: each runs the moments pass; the extrema are merged; both histograms add into ONE
    buffer (the all-reduce SUM); the product's host step plans the selection; each shard selects into its own segment; the
    pick pass runs over the two segments, as on the root."""
    lib = _capi.load()
    K, n = x.shape
    P, nb = len(pct), D.SELECT_BINS
    sfx = "f64" if x.dtype == torch.float64 else "f32"
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    shards = [(x[:, :a], wd[:a]), (x[:, a:], wd[a:])]
    recs = []
    for xs, ws in shards:
        rec = torch.zeros((K, D.WMOM_WORDS), dtype=torch.int64, device="cuda")
        D._weighted_moments_dev(lib, _capi, ctypes, st, xs, ws, rec)
        recs.append(rec.cpu().numpy())
    parts = np.stack(recs)
    f = parts[:, :, :5].view(np.float64)
    lo, hi = f[:, :, 3].min(axis=0), f[:, :, 4].max(axis=0)
    W = int(parts[0, 0, 7]) + int(parts[1, 0, 7])
    ranges = torch.from_numpy(np.ascontiguousarray(np.stack([lo, hi], axis=1))).cuda()
    counts = torch.zeros((K, nb), dtype=torch.int64, device="cuda")
    for xs, ws in shards:
        _capi.check(lib, getattr(lib, f"fiveeq_whist_rows_ranged_{sfx}")(K, xs.shape[1], xs.stride(0), ptr(xs), ptr(ws), ptr(ranges),
                                                                          nb, ptr(counts), st))
    counts_np = counts.cpu().numpy()
    cumw = np.cumsum(counts_np, axis=1)
    assert (cumw[:, -1] == W).all()
    skip = ~(hi > lo)
    targets, binmask = D._weighted_plan(counts_np, cumw, W, pct, skip)
    t_dev, m_dev = torch.from_numpy(targets).cuda(), torch.from_numpy(binmask.view(np.int32)).cuda()
    cap = n
    pool = torch.zeros((K, 2, cap), dtype=x.dtype, device="cuda")
    poolw = torch.zeros((K, 2, cap), dtype=torch.int64, device="cuda")
    seg_n = torch.zeros((K, 2), dtype=torch.int64, device="cuda")
    for g, (xs, ws) in enumerate(shards):
        cand = torch.zeros((K, cap), dtype=x.dtype, device="cuda")
        candw = torch.zeros((K, cap), dtype=torch.int64, device="cuda")
        cn = torch.zeros(K, dtype=torch.int64, device="cuda")
        _capi.check(lib, getattr(lib, f"fiveeq_wselect_bins_{sfx}")(K, xs.shape[1], xs.stride(0), ptr(xs), ptr(ws), ptr(ranges), nb,
                                                                     ptr(m_dev), ptr(cand), ptr(candw), cap, ptr(cn), st))
        pool[:, g], poolw[:, g], seg_n[:, g] = cand, candw, cn
    picked = torch.zeros((K, P), dtype=torch.float64, device="cuda")
    _capi.check(lib, getattr(lib, f"fiveeq_wselect_pick_{sfx}")(K, 2, cap, ptr(pool), ptr(poolw), ptr(seg_n), P, ptr(t_dev),
                                                                 ptr(picked), st))
    out = picked.cpu().numpy()
    return np.where(skip[:, None], lo[:, None], out), W, int(parts[0, 0, 5] + parts[1, 0, 5]), lo, hi


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_shard_split_does_not_change_a_bit(dtype):
    n = 4097
    rows, w = _case(n, 3, "random_half_zero", "normal", dtype, seed=9)
    rows[1] = np.float64(2.5)                                                    # a constant row among them
    x, wd = _on_device(rows, w)
    one = gather_weighted_summary(x, wd, PCT)
    _check(one, rows, w)
    for a in (1, 64, 1000, 2049, n - 1):
        pct, W, count, lo, hi = _two_shards_by_hand(x, wd, a, PCT)
        assert np.array_equal(pct.view(np.int64), one["percentiles"].numpy().view(np.int64)), a
        assert W == one["weight_sum"] and count == int(one["count"][0])
        assert np.array_equal(lo, one["min"].numpy()) and np.array_equal(hi, one["max"].numpy())


# ---- engine level ---------------------------------------------------------------------------------------------------------
N_ENGINE, STEPS_ENGINE = 1000, 20


def _engine(scenarios=False):
    """A 4 + 1 + 1 engine with 1000 sampled members, run for 20 steps (with `scenarios`: under two emission scenarios)."""
    from fiveeqscm_amd.emissions import rcp_like_emissions
    from fiveeqscm_amd.engine import EnsembleEngine
    p = prm.sample_ensemble(prm.default_params("multigas"), N_ENGINE)
    E = rcp_like_emissions(STEPS_ENGINE, 3)
    eng = EnsembleEngine(p, N_ENGINE, np.stack([E, 0.5 * E]) if scenarios else E, device="cuda:0")
    eng.run()
    return eng


def _weights_for(n, seed=4):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, W_ONE + 1, size=n, dtype=np.int64)
    w[rng.uniform(size=n) < 0.5] = 0
    return w


def test_engine_weighted_summary_of_T_and_of_a_gas():
    eng, N, steps = _engine(), N_ENGINE, STEPS_ENGINE
    w = _weights_for(N)
    wd = torch.from_numpy(w).to(eng.device)
    at = [4, steps - 1]
    row_of = {int(t): r for r, t in enumerate(eng.out_steps)}
    T_rows = eng.T[[row_of[t] for t in at]].cpu().numpy()
    s = eng.gather_summary(at, PCT, weights=wd)
    _check(s, T_rows, w)
    assert set(s) >= {"count", "mean", "var", "min", "max", "percentiles", "weight_sum", "ess", "method"}
    g = eng.gather_summary(at, PCT, gas=1, weights=wd)
    _check(g, eng.C[[row_of[t] for t in at], 1].cpu().numpy(), w)
    with pytest.raises(ValueError, match="exclude"):
        eng.gather_summary(at, PCT, weights=wd, accepted=wd > 0)
    # every member at W_ONE: the reference with equal weights
    ones = np.full(N, W_ONE, dtype=np.int64)
    _check(eng.gather_summary(at, PCT, weights=torch.from_numpy(ones).to(eng.device)), T_rows, ones)
    # without weights= nothing changed: the unweighted summary, and its keys
    plain = eng.gather_summary(at, PCT)
    assert "weight_sum" not in plain and np.array_equal(plain["percentiles"].numpy(), np.percentile(T_rows, PCT, axis=1).T)
    eng.close()


def test_engine_weighted_summary_under_the_scenario_axis():
    eng, N, steps = _engine(scenarios=True), N_ENGINE, STEPS_ENGINE
    w = _weights_for(N, seed=6)
    wd = torch.from_numpy(w).to(eng.device)
    row_of = {int(t): r for r, t in enumerate(eng.out_steps)}
    for sc in (0, 1):
        s = eng.gather_summary([3, steps - 1], PCT, scenario=sc, weights=wd)
        _check(s, eng.T[sc][[row_of[3], row_of[steps - 1]]].cpu().numpy(), w)
        g = eng.gather_summary([steps - 1], PCT, scenario=sc, gas=0, weights=wd)
        _check(g, eng.C[sc][[row_of[steps - 1]], 0].cpu().numpy(), w)
    with pytest.raises(ValueError, match="scenario"):
        eng.gather_summary([steps - 1], PCT, weights=wd)
    eng.close()
