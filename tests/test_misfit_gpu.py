"""The in-loop misfit (include/fiveeq.h "CONSTRAINED RUNS") against references that do not share its code.

Every kernel that carries the accumulators calls one misfit_step(), so comparing the forms with each other
(tests/test_constrain_gpu.py) cannot see a mistake inside it.  Three references do:
  R1  bit for bit: constrain.misfit_numpy on the T rows the same run stored (every step stored), onto the run's own
      starting accumulators.  The header promises step order and one rounding per operation (no fma; the library is built
      with -ffp-contract=off), and fp32 T widens exactly, so the tolerance is zero.
  R2  the model: the C oracle's fp64 T through the same restatement — fp64 within the project's 1e-10 of the per-member
      scale of |terms|; fp32 chi2 within the bound of test_fp32_chi2_against_the_fp64_oracle built on 4x the default fp32
      form's measured worst T error.
  R3  exact arithmetic: the score sum_t p_t (T_t - sum_t b_t T_t - o_t)^2 in rationals on the device's own T, against
      eng.chi2() within a derived bound (oracle/misfit_exact.py, test_r3_score's docstring).
Through the engine: both misfit layouts x fp64 / fp32 packed / fp32 unpacked x N x every form x seven observation tables.
Through the C ABI: member sub-ranges (packed half lanes), untouched memory outside them, nonzero starting accumulators and
the skip rule.  At size: 100M fp32 members, misfit words past 2^31 bytes."""
import functools
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from fiveeqscm_amd import _capi, constrain, emissions, scenario
from fiveeqscm_amd import params as prm
from fiveeqscm_amd.constrain import Observations
from fiveeqscm_amd.engine import EnsembleEngine
from oracle import c_oracle
from oracle import misfit_exact as mx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STEPS = 400
RUN_YEARS = 1750.0 + np.arange(N_STEPS)
FP64_REL = 1e-10          # the project's fp64 target (BASELINE north star); the C oracle is within 2.1e-14 of 50 digits
# the default fp32 form's worst T error against 50-digit arithmetic, relative with a 1e-2 K floor, as
# tests/test_golden_fiveeq.py::test_fp32_kernels_against_50_digit_arithmetic measures it: {4} 1.673e-5, 4 + 1 + 1 1.049e-5
FP32_T_WORST = 1.673e-5
GASES = {"co2": 1, "multigas": 3}
PRECISIONS = ("fp64", "fp32_packed", "fp32_unpacked")
NS = (1, 2, 63, 64, 65, 130, 4096 + 37)
NAN32, NAN64 = 0x7FC0DEAD, 0x7FF8DEADBEEF0001          # quiet NaNs with a payload: sentinel bits
NEG0_32, NEG0_64 = -(1 << 31), -(1 << 63)              # -0.0 as int32 / int64


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _record(rng, years, baseline):
    years = np.asarray(years, dtype=np.float64)
    T = 0.4 + 0.006 * (years - 1900.0) + rng.normal(0.0, 0.1, years.size)
    return Observations.from_years(RUN_YEARS, years, T, rng.uniform(0.05, 0.3, years.size), baseline=baseline)


@functools.lru_cache(maxsize=None)
def _tables():
    """The observation tables over the run's 400 steps (step t is year 1750 + t)."""
    rng = np.random.default_rng(20261016)
    y, T, s = scenario.read_observations_csv(os.path.join(ROOT, "tests", "golden", "obs_synthetic.csv"))
    return {
        # window from step 0, baseline holding step 0, last observation on the last step
        "a_edges": _record(rng, np.r_[np.arange(1750, 2147, 3), 2149], (1750, 1760)),
        # window [125, 250): both edges on refills of the fused kernel's drive table (every 125 steps from t_begin = 0)
        "b_refill": _record(rng, np.arange(1875, 2000), (1875, 1900)),
        # every third year, with a 30-year gap inside the window
        "c_sparse": _record(rng, [y_ for y_ in range(1900, 2070, 3) if not 1960 <= y_ < 1990], (1900, 1950)),
        # baseline disjoint from the observations: before them, then after them
        "d_base_before": _record(rng, np.arange(1950, 2050, 2), (1800, 1830)),
        "d_base_after": _record(rng, np.arange(1900, 2000, 2), (2100, 2120)),
        # a window of one step
        "e_single": _record(rng, [2000], (2000, 2000)),
        "f_fixture": Observations.from_years(RUN_YEARS, y, T, s, baseline=(1900, 1950)),
    }


TABLES = ("a_edges", "b_refill", "c_sparse", "d_base_before", "d_base_after", "e_single", "f_fixture")


@functools.lru_cache(maxsize=None)
def _ensemble(kind, N):
    return prm.sample_ensemble(prm.default_params(kind), N), emissions.rcp_like_emissions(N_STEPS, GASES[kind])


@functools.lru_cache(maxsize=None)
def _oracle_T(kind, N):
    p, E = _ensemble(kind, N)
    return c_oracle.run(E, p, N, keep=("T",))["T"]


class _Packing:
    """fiveeq_set_f32_packing for the precision form, restored on exit."""

    def __init__(self, prec):
        self.on = 0 if prec == "fp32_unpacked" else 1

    def __enter__(self):
        self.prev = _capi.load().fiveeq_set_f32_packing(self.on)

    def __exit__(self, *exc):
        _capi.load().fiveeq_set_f32_packing(self.prev)


def _dtype(prec):
    return torch.float64 if prec == "fp64" else torch.float32


def _bits(x):
    return x.view(torch.int64 if x.dtype == torch.float64 else torch.int32)


# ---- the three references -----------------------------------------------------------------------------------------------
def _r1(T_rows, table, misfit, acc=None, what=""):
    """R1: the accumulators equal misfit_numpy on the run's own stored T, bit for bit (tolerance zero)."""
    want = torch.from_numpy(constrain.misfit_numpy(np.asarray(T_rows), table, acc=acc))
    got = misfit.cpu()
    assert torch.equal(_bits(got), _bits(want)), (what, int((_bits(got) != _bits(want)).sum()))     # tolerance zero


def _r2(T_dev, misfit, chi2, table, P, T_or, prec, what=""):
    """R2: against the C oracle's fp64 T through the same restatement.  fp64: every accumulator within FP64_REL of its
    per-member scale of |terms| (test_fp64_accumulators_against_the_c_oracle).  fp32: chi2 within the construction of
    test_fp32_chi2_against_the_fp64_oracle — |T error| <= dT = 4 FP32_T_WORST (max_t |T| + 1e-2 K), so a residual
    r_t = T_t - mean_ref T - o_t errs by at most 2 dT and |d chi2| <= sum_t p_t (2 |r_t| 2 dT + (2 dT)^2)."""
    want = constrain.misfit_numpy(T_or, table)
    if prec == "fp64":
        got = misfit.cpu().numpy()
        d = T_or - table[:, 0:1]
        scale = np.stack([(table[:, 2:3] * np.abs(T_or)).sum(0), (table[:, 1:2] * np.abs(d)).sum(0),
                          (table[:, 1:2] * d * d).sum(0)])
        err = np.abs(got - want)
        print(f"  R2 fp64 {what}: worst |err| / (1e-10 scale) = {float((err / (FP64_REL * scale)).max()):.3g}")
        assert np.isfinite(got).all() and np.all(err <= FP64_REL * scale), what          # the project's 1e-10
    else:
        got = chi2.cpu().numpy()
        r = T_or - (table[:, 2:3] * T_or).sum(0)[None, :] - table[:, 0:1]
        dT = 4 * FP32_T_WORST * (np.abs(T_or).max(0) + 1e-2)
        bound = (table[:, 1:2] * (4 * np.abs(r) * dT + 4 * dT * dT)).sum(0)
        err = np.abs(got - constrain.chi2_from_misfit(want, P))
        print(f"  R2 fp32 {what}: worst |d chi2| / bound = {float((err / bound).max()):.3g}")
        assert np.all(err <= bound), what                                                # 4 x the measured fp32 worst case


def _r3(T_dev, misfit, chi2, table, P, members, what=""):
    """R3: eng.chi2() against the exact score on the device's own T, within the derived bound (mx.chi2_bound)."""
    T = np.asarray(T_dev)
    mis = misfit.cpu().numpy()
    c2 = chi2.cpu().numpy()
    worst = 0.0
    for m in members:
        exact, bound = mx.chi2_bound(T[:, m], table, mis[:, m], P)
        err = abs(Fraction(float(c2[m])) - exact)
        worst = max(worst, float(err / bound) if bound else float(err > 0))
        assert err <= bound, (what, int(m), float(err), float(bound))                   # the derived bound
    print(f"  R3 {what}: {len(members)} members, worst |chi2 - exact| / bound = {worst:.3g}")


def _sample(N, n=64):
    return np.unique(np.linspace(0, N - 1, min(N, n)).round().astype(np.int64))


# ---- the matrix through the engine --------------------------------------------------------------------------------------
def _forms(N, window):
    """(name, engine keywords, [(t_begin, t_end, mode, run keywords)]) of every form a case runs."""
    w0, w1 = window
    whole = lambda mode, **kw: [(0, N_STEPS, mode, kw)]                                  # noqa: E731
    out = [("per_step/1", dict(per_step_streams=1), whole("per_step"))]
    if N >= 1024:                                                   # per_step_launches cuts two parts from 1024 members
        out.append(("per_step/2", dict(per_step_streams=2), whole("per_step")))
    out += [("graph", dict(per_step_streams=1), whole("graph")),
            ("fused/None", dict(fused_span=None), whole("fused")),
            ("fused/7", dict(fused_span=7), whole("fused")),
            ("fused/auto", dict(fused_span="auto"), whole("fused"))]
    out += [(f"ksteps/{k}", {}, whole("ksteps", k_steps=k)) for k in (1, 8, 125, 126)]
    out.append(("auto", {}, whole("auto")))
    if N > 256:                                                     # 4133 = 16 x 256 + a ragged chunk of 37
        out.append(("chunk256", dict(chunk_members=256, per_step_streams=1), whole("per_step")))
    edge = w0 if w0 > 0 else (w1 if w1 < N_STEPS else 125)
    inside = (w0 + w1) // 2 if w1 - w0 > 1 else edge
    out.append(("split/edge", dict(fused_span=None), [(0, edge, "per_step", {}), (edge, N_STEPS, "fused", {})]))
    out.append(("split/inside", dict(fused_span=7), [(0, inside, "fused", {}), (inside, N_STEPS, "ksteps", dict(k_steps=8))]))
    return out


def _run(kind, N, prec, obs, ekw, calls, **more):
    p, E = _ensemble(kind, N)
    eng = EnsembleEngine(p, N, E, observations=obs, dtype=_dtype(prec), store_concentrations=False, device="cuda:0",
                         **ekw, **more)
    for t0, t1, mode, kw in calls:
        eng.run(t0, t1, mode=mode, **kw)
    torch.cuda.synchronize()
    return eng


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("kind", sorted(GASES))
def test_matrix(kind, prec, N, table):
    """R1 for every form on all members (each form's T equals the first form's bit for bit, and its accumulators equal
    misfit_numpy of that T); R2 and R3 on the first form (the others are the same bits)."""
    obs = _tables()[table]
    tab = obs.table
    ref = None
    with _Packing(prec):
        for name, ekw, calls in _forms(N, obs.window):
            eng = _run(kind, N, prec, obs, ekw, calls)
            T, mis = eng.T.cpu(), eng.misfit.cpu()
            if ref is None:
                _r1(T.numpy(), tab, mis, what=name)
                ref = (name, T, mis, eng.chi2().cpu())
            else:
                assert torch.equal(_bits(T), _bits(ref[1])), (name, "T differs from", ref[0])
                assert torch.equal(_bits(mis), _bits(ref[2])), (name, "misfit differs from R1")
            eng.close()
    _, T, mis, chi2 = ref
    what = f"{kind}/{prec}/N={N}/{table}"
    _r2(T, mis, chi2, tab, obs.P, _oracle_T(kind, N), prec, what)
    _r3(T.numpy(), mis, chi2, tab, obs.P, _sample(N), what)


# ---- R3 where it is hardest ---------------------------------------------------------------------------------------------
def _cancelling_case(kind, N):
    """Members whose T starts ~10 K above equilibrium (slow thermal box S0 = 10 K: T decays over d = 239 yr) and a record
    o_t = T_c(t) - mean_ref T_c + eps_t of the centre member c (C oracle), baseline over the first 21 steps: o_t and T_t are
    apart by the common offset mean_ref T ~ 9.5 K, so V ~ P (9.5 K)^2 while chi2 ~ sum p eps^2 (V >> chi2)."""
    p, E = _ensemble(kind, N)
    S0 = np.tile(np.array([[10.0], [0.0]]), (1, N))
    Tc = c_oracle.run(E, prm.default_params(kind), 1, keep=("T",), S0=S0[:, :1])["T"][:, 0]
    rng = np.random.default_rng(7)
    steps = np.arange(10, 121, 2)
    ref = Tc[0:21].mean()
    obs = Observations.from_years(RUN_YEARS, RUN_YEARS[steps], Tc[steps] - ref + rng.normal(0.0, 0.01, steps.size), 0.05,
                                  baseline=(RUN_YEARS[0], RUN_YEARS[20]))
    T_or = c_oracle.run(E, p, N, keep=("T",), S0=S0)["T"]
    return obs, S0, T_or


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("kind", sorted(GASES))
def test_r3_score(kind, prec):
    """R3 on a table that forces cancellation, beside R1 and R2.  The bound (oracle/misfit_exact.py, chi2_bound) is
    derived, not fitted.  u = 2^-53, k = (steps of the window) + 3, gamma_k = k u / (1 - k u).  The device adds, in step
    order, n <= k - 3 terms onto zero: A += b T (1 rounding per term), U += p fl(T - o) (2), V += fl(p d) d (4, the
    rounding of d counted twice); by recursive summation (Higham lemma 3.3) |A' - A| <= gamma_k sum b|T| = eA,
    |U' - U| <= gamma_k sum p|T - o| = eU, |V' - V| <= gamma_k sum p (T - o)^2 = eV, and the table's P' (an fp64 sum of the
    n_obs <= k nonzero p_t) |P' - P| <= gamma_k sum p = eP.  The exact score equals V - 2 A U + A^2 P, so
        |chi2' - chi2| <= eV + 2 (eA |U'| + |A'| eU + eA eU) + (2 |A'| eA + eA^2) P' + (|A'| + eA)^2 eP
                          + gamma_3 (|V'| + 2 |A' U'| + A'^2 P'),
    the last line the final roundings of chi2' = fl(fl(V' - fl(2 A' U')) + fl(fl(A' A') P')): each of its three terms
    passes through at most three roundings.  The absolute sums are taken exactly; A', U', V', P' are the device's words."""
    N = 130
    obs, S0, T_or = _cancelling_case(kind, N)
    with _Packing(prec):
        eng = _run(kind, N, prec, obs, dict(fused_span=7), [(0, N_STEPS, "fused", {})], S0=S0)
    T, mis, chi2 = eng.T.cpu(), eng.misfit.cpu(), eng.chi2().cpu()
    eng.close()
    _r1(T.numpy(), obs.table, mis, what="cancel")
    V = mis[2].numpy()
    assert np.all(V > 100 * chi2.numpy()), float((V / chi2.numpy()).min())           # the table does force cancellation
    _r2(T, mis, chi2, obs.table, obs.P, T_or, prec, f"{kind}/{prec}/cancel")
    _r3(T.numpy(), mis, chi2, obs.table, obs.P, _sample(N, N), f"{kind}/{prec}/cancel")


@pytest.mark.parametrize("prec", PRECISIONS)
def test_r3_on_the_extreme_corner_of_the_hypercube(prec):
    """The {4} members of test_extreme_corner_of_the_hypercube (highest emissions and rT: the iIRF clip engages) on two
    tables: R1, R2 and R3 on all 64."""
    N = 64
    base = prm.default_params("co2")
    p = dict(base)
    p["r0"] = np.full((1, N), 1.2 * base["r0"][0])
    p["rC"] = np.full((1, N), 1.5 * base["rC"][0])
    p["rT"] = np.linspace(0.5, 1.5, N)[None, :] * base["rT"][0]
    p["q"] = prm.k_q(np.full(N, 2.5), np.full(N, 4.5), base["d"], prm.forcing_2x(base))
    E = 3.0 * np.abs(emissions.rcp_like_emissions(N_STEPS, 1))
    T_or = c_oracle.run(E, p, N, keep=("T",))["T"]
    for table in ("a_edges", "f_fixture"):
        obs = _tables()[table]
        with _Packing(prec):
            eng = EnsembleEngine(p, N, E, observations=obs, dtype=_dtype(prec), store_concentrations=False, device="cuda:0")
            eng.run(mode="per_step")
            torch.cuda.synchronize()
        T, mis, chi2 = eng.T.cpu(), eng.misfit.cpu(), eng.chi2().cpu()
        eng.close()
        what = f"corner/{prec}/{table}"
        _r1(T.numpy(), obs.table, mis, what=what)
        _r2(T, mis, chi2, obs.table, obs.P, T_or, prec, what)
        _r3(T.numpy(), mis, chi2, obs.table, obs.P, np.arange(N), what)


# ---- through the C ABI: sub-ranges, half lanes, untouched memory, the skip rule -----------------------------------------
def _fill_sentinels(x):
    """Every word of x (fp32 or fp64) becomes a NaN with a payload or -0.0, alternately."""
    b = _bits(x)
    nan, neg0 = (NAN64, NEG0_64) if x.dtype == torch.float64 else (NAN32, NEG0_32)
    idx = torch.arange(b.numel(), device=b.device).view(b.shape)
    b.copy_(torch.where(idx % 2 == 0, torch.full_like(b, nan), torch.full_like(b, neg0)))


def _run_obs(eng, t0, t1, m0, n, form, k):
    fn = eng._fn("run_obs")
    rc = fn(*eng._run_args(t0, t1, m0, n), *eng._obs_args(m0), form, k, eng._stream())
    _capi.check(eng.lib, rc)
    torch.cuda.synchronize()


SUBRANGES = (
    # fp32 4 + 1 + 1, even ld and m0, odd n: a packed half lane in the per-step and the fused kernel
    *[("multigas", "fp32_packed", 2, n, form, k) for n in (3, 65, 257)
      for form, k in ((_capi.FORM_PER_STEP, 0), (_capi.FORM_FUSED, 0), (_capi.FORM_FUSED, 7))],
    # odd m0: the rows are not 8-byte aligned, the unpacked kernels run
    ("multigas", "fp32_packed", 3, 65, _capi.FORM_PER_STEP, 0),
    ("multigas", "fp32_packed", 3, 65, _capi.FORM_FUSED, 7),
    # {4}: a packed per-step half lane; the fused kernel has no packed misfit form for it and runs unpacked
    ("co2", "fp32_packed", 2, 65, _capi.FORM_PER_STEP, 0),
    ("co2", "fp32_packed", 2, 65, _capi.FORM_FUSED, 0),
    ("co2", "fp64", 1, 65, _capi.FORM_FUSED, 7),
    ("multigas", "fp64", 1, 65, _capi.FORM_PER_STEP, 0),
)


@pytest.mark.parametrize("kind,prec,m0,n,form,k", SUBRANGES)
def test_member_subrange_through_the_c_abi(kind, prec, m0, n, form, k):
    """fiveeq_run_obs_* on members [m0, m0 + n) of rows of length ld = 600 (a plain pointer offset, include/fiveeq.h):
    R, S, T and misfit words outside the range — the column just past its last member, which a packed half lane reads,
    included — keep their sentinel bits; the range's accumulators start at random nonzero values and end as R1 of its own
    T onto them; its T is that of an engine built from those members alone (members never interact)."""
    ld = 600
    obs = _tables()["b_refill"]
    p, E = _ensemble(kind, ld)
    eng = EnsembleEngine(p, ld, E, observations=obs, dtype=_dtype(prec), store_concentrations=False, device="cuda:0")
    for x in (eng.R, eng.S, eng.T, eng.misfit):
        _fill_sentinels(x)
    sl = slice(m0, m0 + n)
    eng.R[:, sl] = 0.0
    eng.S[:, sl] = 0.0
    rng = np.random.default_rng(m0 * 1000 + n)
    acc0 = np.stack([rng.normal(0.0, 1.0, n), rng.normal(0.0, 30.0, n), rng.uniform(1.0, 1e4, n)])
    eng.misfit[:, sl] = torch.from_numpy(acc0).cuda()
    torch.cuda.synchronize()
    before = [_bits(x).clone() for x in (eng.R, eng.S, eng.T, eng.misfit)]
    with _Packing(prec):
        _run_obs(eng, 0, N_STEPS, m0, n, form, k)
    outside = torch.ones(ld, dtype=torch.bool, device="cuda:0")
    outside[sl] = False
    for name, x, b in zip("RSTM", (eng.R, eng.S, eng.T, eng.misfit), before):
        same = _bits(x)[..., outside] == b[..., outside]
        assert bool(same.all()), (name, "words outside the range changed", int((~same).sum()))   # bits, no tolerance
    _r1(eng.T[:, sl].cpu().numpy(), obs.table, eng.misfit[:, sl], acc=acc0, what="sub-range")
    sub = dict(p)
    for key in ("r0", "rC", "rT", "q"):
        sub[key] = np.asarray(p[key])[:, sl]
    alone = EnsembleEngine(sub, n, E, observations=obs, dtype=_dtype(prec), store_concentrations=False, device="cuda:0")
    alone.run(mode="per_step")
    torch.cuda.synchronize()
    assert torch.equal(_bits(alone.T), _bits(eng.T[:, sl]))                  # bits, no tolerance
    alone.close()
    eng.close()


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("kind", sorted(GASES))
def test_steps_outside_the_window_neither_read_nor_write(kind, prec):
    """The skip rule.  (1) Ranges wholly outside the window [125, 250), per-step and fused, on accumulators preset to -0.0
    and NaN payloads: every bit stays (a read-modify-write with zero weights turns -0.0 into +0.0).  (2) NaN in o_t of every
    step with p_t = b_t = 0, written straight into the engine's obs (Observations refuses non-finite values): the
    accumulators stay finite and equal R1 in every form (computing such a step would give 0 * NaN)."""
    ld = 130
    obs = _tables()["b_refill"]
    p, E = _ensemble(kind, ld)
    with _Packing(prec):
        eng = EnsembleEngine(p, ld, E, observations=obs, dtype=_dtype(prec), store_trajectory=False, device="cuda:0")
        _fill_sentinels(eng.misfit)
        torch.cuda.synchronize()
        before = _bits(eng.misfit).clone()
        for form, k in ((_capi.FORM_PER_STEP, 0), (_capi.FORM_FUSED, 0), (_capi.FORM_FUSED, 7)):
            for t0, t1, m0, n in ((0, 125, 0, ld), (250, N_STEPS, 0, ld), (0, 125, 2, 65), (250, N_STEPS, 1, 64)):
                _run_obs(eng, t0, t1, m0, n, form, k)
                assert torch.equal(_bits(eng.misfit), before), (form, k, t0, t1, m0, n)          # bits, no tolerance
        eng.close()
        nan_tab = np.array(_tables()["c_sparse"].table)
        dead = (nan_tab[:, 1] == 0) & (nan_tab[:, 2] == 0)
        nan_tab[dead, 0] = np.nan
        for name, ekw, calls in _forms(ld, _tables()["c_sparse"].window):
            eng = EnsembleEngine(p, ld, E, observations=_tables()["c_sparse"], dtype=_dtype(prec), store_concentrations=False,
                                 device="cuda:0", **ekw)
            eng.obs.copy_(torch.from_numpy(nan_tab))
            for t0, t1, mode, kw in calls:
                eng.run(t0, t1, mode=mode, **kw)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(eng.misfit).all()), name
            _r1(eng.T.cpu().numpy(), nan_tab, eng.misfit, what=name)
            eng.close()


# ---- at size -------------------------------------------------------------------------------------------------------------
def test_misfit_rows_past_2_31_bytes():
    """fp32 4 + 1 + 1 with 100,000,000 members: misfit [3][ld] fp64 is 2.4 GB, and the V words of members from ~68.4M on lie
    past 2^31 bytes.  The fused run and the chunk-major per-step run (misfit pointers offset per chunk) give the same bits;
    a strided sample of 4097 members (N - 1 and members past that offset included) has the bits of a small engine built
    from the sampled fp32 parameters, and that engine passes R1 on its own stored T."""
    N, n_steps = 100_000_000, 60
    if torch.cuda.mem_get_info()[0] < 40 << 30:
        pytest.skip("needs ~40 GB of free HBM")
    years = 1900.0 + np.arange(n_steps)
    rng = np.random.default_rng(3)
    oy = years[20:]
    obs = Observations.from_years(years, oy, 0.5 + rng.normal(0.0, 0.1, oy.size), 0.1, baseline=(1905, 1925))
    E = emissions.rcp_like_emissions(n_steps, 3)
    pd = prm.sample_ensemble_shard(prm.default_params("multigas"), N, device="cuda:0", dtype=torch.float32)
    eng = EnsembleEngine(pd, N, E, observations=obs, dtype=torch.float32, store_trajectory=False, device="cuda:0")
    eng.run(mode="fused")
    torch.cuda.synchronize()
    fused = eng.misfit.clone()
    eng.reset_state()
    eng.run(mode="per_step")
    torch.cuda.synchronize()
    assert eng.chunk_members and eng.chunk_members < N                 # the per-step run is chunk-major
    assert torch.equal(_bits(eng.misfit), _bits(fused))                    # bits, no tolerance
    idx = torch.cat([torch.arange(4096, device="cuda:0") * (N // 4096) + 17, torch.tensor([N - 1], device="cuda:0")])
    assert int(idx.max()) == N - 1 and int(((2 * N + idx) * 8 >= 1 << 31).sum()) > 1000
    sample = dict(pd)
    for key in ("r0", "rC", "rT", "q"):
        sample[key] = pd[key][:, idx].double().cpu().numpy()              # the fp32 parameters, widened exactly
    got = eng.misfit[:, idx].cpu()
    eng.close()
    del eng, pd, fused
    torch.cuda.empty_cache()
    n = int(idx.numel())
    small = EnsembleEngine(sample, n, E, observations=obs, dtype=torch.float32, store_concentrations=False, device="cuda:0")
    small.run(mode="per_step")
    torch.cuda.synchronize()
    assert torch.equal(_bits(small.misfit.cpu()), _bits(got))              # bits, no tolerance
    _r1(small.T.cpu().numpy(), obs.table, small.misfit, what="small engine")
    small.close()
    del small
    torch.cuda.empty_cache()
