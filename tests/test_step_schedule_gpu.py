"""The per-step kernels' row schedule (fiveeq_step.hpp, step_body): in the fp64 kernels rows are loaded in order of use and stored
as soon as their value is final — R of gas g and, on a stored step, its C row right after gas g's arithmetic (member_step's after-gas hook).  The
schedule moves WHEN bytes move, never a value: every per-step form must give the bits of the time-fused kernel, which calls
the unhooked member_step() and stores everything at the end of the launch.

  1. the C entry points fiveeq_run_* (step_kernel) and fiveeq_run_uniform_* (step_uniform_kernel: mask 0, a mixed mask, every r
     row single-valued) against fiveeq_run_fused_* on the same inputs, bit for bit: R, S, every stored C / T row; the wave
     records' minimum and maximum too, their two sums against the exact restatement of the per-step kernels' own fold (the
     fused kernel folds in another order: _check_records, profiles/r18/NOTES.md) — for 1, 63, 64, 65, 129 and 1,000 members (idle
     tail lanes parked on the last member, the half-filled packed lane, one and several waves), pools {4} and 4 + 1 + 1, fp64 / packed fp32 (even ld, odd counts included) / scalar fp32,
     both row policies, every step stored / a strict subset stored (the others take the row < 0 path) / nothing stored (null
     C and T pointers);
  2. a member sub-range [256, 256 + n) of rows with a larger ld — what the two-launch form does — which must also leave every
     member outside the range untouched;
  3. the engine's feature forms per_step against fused: observations= (MISFIT, with steps outside the window), forcing= with
     K = 0 and K = 2 (FORC), both together, hist= (BINS) and collect_stats=True;
  4. one plain case against the C oracle at the project's tolerance |a - b| <= 1e-10 |b| + 1e-13.
Inputs are centred on the parameter sets' defaults, 8 steps of the emission scenario where every gas is emitted; the C oracle
(CPU, fp64) confirms beforehand that every member stays in the model's domain (finite, C > 0), so no row is ever left out of a
comparison."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fiveeqscm_amd import _capi  # noqa: E402
from fiveeqscm_amd import params as prm  # noqa: E402
from fiveeqscm_amd.emissions import make_drive, rcp_like_emissions  # noqa: E402

DEV = "cuda:0"
T0, N_STEPS = 280, 8                                    # steps 280 .. 287 of the scenario: CO2, CH4 and N2O all emitted
COUNTS = (1, 63, 64, 65, 129, 1000)
N_MAX = 1400                                            # members of the input set (the sub-range cases reach 256 + 1000 + padding)
ROWS_CACHED, ROWS_STREAMED, ROWS_AUTO = 0, 1, 2
FORMS = {                                               # dtype, ld(n): fp32 packs with an even ld, cannot with an odd one
    "f64": (torch.float64, lambda n: n + 3),
    "f32_packed": (torch.float32, lambda n: (n + 3) // 2 * 2),
    "f32_scalar": (torch.float32, lambda n: (n + 2) | 1),
}
STORED = {"all": list(range(N_STEPS)), "some": [1, 2, 6], "none": None}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _capi.load()


def _ptr(t, off=0):
    return ctypes.c_void_p(0 if t is None else t.data_ptr() + off)


def _bits(t):
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def _same(a, b):
    return torch.equal(a, b) and torch.equal(_bits(a), _bits(b))


def _emissions(G):
    E = rcp_like_emissions(T0 + N_STEPS, G)[T0:]
    assert (E > 0).all()
    return E


def _masks(G):
    """plain kernel (None); the uniform kernel with mask 0, a mixed mask, every r row single-valued"""
    mixed = (1 << 4) | (1 << 7) | (1 << 8) if G == 3 else (1 << 1)       # three gases: the multi-gas defaults' rows
    return (None, 0, mixed, (1 << 3 * G) - 1)


_ROWS = {}


def _rows(kind, mask):
    """fp64 parameter rows [3G + 2, N_MAX] around the set's defaults, each row of `mask` holding one value — built once per
    (kind, mask) and checked once, on the CPU with the C oracle, to keep every member in the model's domain."""
    key = (kind, mask or 0)
    if key not in _ROWS:
        from oracle import c_oracle
        base = prm.default_params(kind)
        G = prm.n_gas_of(base)
        rng = np.random.default_rng(1800 + 31 * G + (mask or 0))
        centre = np.array([np.asarray(base[k], dtype=np.float64).reshape(G)[g] for g in range(G) for k in ("r0", "rC", "rT")]
                          + list(base["q"]))
        rows = centre[:, None] * rng.uniform(0.8, 1.2, size=(3 * G + 2, N_MAX)) + rng.uniform(0.0, 0.01, size=(3 * G + 2, N_MAX))
        for k in range(3 * G + 2):
            if (mask or 0) >> k & 1:
                rows[k, :] = rows[k, 0]
        p = dict(base)
        for i, name in enumerate(("r0", "rC", "rT")):
            p[name] = rows[i:3 * G:3]
        p["q"] = rows[3 * G:]
        want = c_oracle.run(_emissions(G), p, N_MAX, keep=("C", "T"))
        assert np.isfinite(want["C"]).all() and np.isfinite(want["T"]).all() and (want["C"] > 0).all(), key
        assert np.isfinite(want["R"]).all() and np.isfinite(want["S"]).all(), key
        _ROWS[key] = (rows, p, want)
    return _ROWS[key]


def _run(lib, entry, kind, dtype, n, ld, m0, rows, stored, mask=None):
    """N_STEPS steps from a zero state for members [m0, m0 + n) of rows with leading dimension ld, through `entry`
    ("run", "run_uniform" or "run_fused").  Untouched elements keep the fill values (R, S: 0; C, T: -7; records: -7)."""
    model = prm.make_model(prm.default_params(kind))
    G, SP = model.n_gas, sum(prm.pools_of(prm.default_params(kind)))
    sfx, w = ("f64", 8) if dtype == torch.float64 else ("f32", 4)
    out_steps = STORED[stored]
    drive = torch.from_numpy(make_drive(_emissions(G), output_steps=out_steps if out_steps is not None else [])).to(DEV, dtype)
    n_rows = len(out_steps) if out_steps is not None else 0
    par = torch.zeros((3 * G + 2, ld), dtype=dtype, device=DEV)
    par[:, :min(ld, N_MAX)] = torch.from_numpy(rows[:, :min(ld, N_MAX)]).to(DEV, dtype)
    r, q = par[:3 * G].contiguous(), par[3 * G:].contiguous()
    R = torch.zeros((SP, ld), dtype=dtype, device=DEV)
    S = torch.zeros((2, ld), dtype=dtype, device=DEV)
    C = torch.full((n_rows, G, ld), -7.0, dtype=dtype, device=DEV) if n_rows else None
    T = torch.full((n_rows, ld), -7.0, dtype=dtype, device=DEV) if n_rows else None
    stats = torch.full(((ld + 63) // 64, N_STEPS, 4), -7.0, dtype=torch.float64, device=DEV)
    args = [ctypes.byref(model), n, ld, _ptr(drive), N_STEPS, 0, N_STEPS, _ptr(r, m0 * w), _ptr(q, m0 * w), _ptr(R, m0 * w),
            _ptr(S, m0 * w), _ptr(C, m0 * w), _ptr(T, m0 * w), n_rows, _ptr(stats, (m0 // 64) * N_STEPS * 4 * 8)]
    if entry == "run_uniform":
        first = torch.cat([r[:, m0], q[:, m0]]).cpu().numpy()
        args += [mask, first.ctypes.data_as(ctypes.c_void_p)]
    rc = getattr(lib, f"fiveeq_{entry}_{sfx}")(*args, None)
    _capi.check(lib, rc)
    torch.cuda.synchronize()
    out = {"R": R, "S": S, "T_stats": stats}
    if n_rows:
        out.update(C=C, T=T)
    return out


def _ladder(v, packed):
    """wave_reduce_to_lane63 / wave_reduce_to_lanes_31_63 (fiveeq_stats.hpp) on v [..., 64] fp64, operation for operation:
    row_shr 1, 2, 4, 8 inside each row of 16 lanes, row_bcast:15 into rows 1 and 3, and (scalar lanes) row_bcast:31 into rows
    2 and 3; a lane without a source adds 0.  Returns the totals of lane 63, or of lanes 31 and 63 (packed)."""
    v = v.copy()
    lane = np.arange(64)
    for sh in (1, 2, 4, 8):
        src = np.where(lane % 16 >= sh, np.roll(v, sh, axis=-1), 0.0)
        v = v + src
    src = np.zeros_like(v)
    src[..., 16:32] = v[..., 15:16]
    src[..., 48:64] = v[..., 47:48]
    v = v + src
    if packed:
        return v[..., [31, 63]]
    src = np.zeros_like(v)
    src[..., 32:64] = v[..., 31:32]
    return (v + src)[..., 63]


def _records(T_rows, packed):
    """The per-step kernels' wave records [ceil(n / 64), n_steps, 4] (sum, sum of squares, min, max) of T_rows [n_steps, n],
    EXACTLY: the sums in the kernels' own order of additions (_ladder), every operation one IEEE fp64 operation."""
    T = np.asarray(T_rows, dtype=np.float64)
    n_steps, n = T.shape
    n_rec = (n + 63) // 64
    per = 128 if packed else 64
    n_wave = (n + per - 1) // per
    pad = np.zeros((n_steps, n_wave * per))
    pad[:, :n] = T
    live = np.zeros(n_wave * per, dtype=bool)
    live[:n] = True
    if packed:
        x, y = pad[:, 0::2].reshape(n_steps, n_wave, 64), pad[:, 1::2].reshape(n_steps, n_wave, 64)
        s1 = _ladder(x + y, True).reshape(n_steps, 2 * n_wave)[:, :n_rec]
        s2 = _ladder(x * x + y * y, True).reshape(n_steps, 2 * n_wave)[:, :n_rec]
    else:
        v = pad.reshape(n_steps, n_wave, 64)
        s1, s2 = _ladder(v, False), _ladder(v * v, False)
    grp = np.full((n_steps, n_rec * 64), np.nan)
    grp[:, :n] = T
    grp = grp.reshape(n_steps, n_rec, 64)
    out = np.stack([s1, s2, np.nanmin(grp, axis=2), np.nanmax(grp, axis=2)], axis=2)     # [n_steps, n_rec, 4]
    return np.ascontiguousarray(out.transpose(1, 0, 2))


def _check_records(got, fused, T_rows, packed, rec0, what):
    """The wave records of a per-step run.  Minimum and maximum do not depend on the order of the fold: the fused kernel's
    bits.  The two sums do — the fused kernel folds its LDS tile in another order than the per-step kernels' DPP ladder, and
    the two differ in the last bit of a sum now and then (on the commit before the row schedule changed as well) — so they
    are held to the exact restatement of the ladder on the run's own T rows, which are the fused kernel's bits themselves."""
    assert torch.equal(got[..., 2:], fused[..., 2:]), (what, "T_stats min / max")
    want = torch.from_numpy(_records(T_rows.cpu().numpy(), packed)).to(got.device)
    n_rec = want.shape[0]
    assert n_rec > 0 and _same(got[rec0:rec0 + n_rec], want), (what, "T_stats")
    rest = torch.ones(got.shape[0], dtype=torch.bool, device=got.device)
    rest[rec0:rec0 + n_rec] = False
    assert bool((got[rest] == -7).all()) or got.shape[0] == n_rec, (what, "T_stats records of other members")


def _compare(got, want, what):
    compared = 0
    for name in want:
        if name == "T_stats":
            continue                                           # _check_records
        assert _same(got[name], want[name]), (what, name)
        compared += want[name].numel()
    assert compared > 0 and bool(torch.isfinite(want["R"]).all()) and bool(torch.isfinite(want["S"]).all()), what
    assert bool((want["R"] != 0).any()), what                  # the run really stepped


# ---- 1. every count, layout, precision, policy and stored-row pattern --------------------------------------------------------
@pytest.mark.parametrize("policy", [ROWS_CACHED, ROWS_STREAMED])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("kind", ["multigas", "co2"])
def test_per_step_kernels_give_the_fused_kernel_s_bits(lib, kind, form, policy):
    dtype, ld_of = FORMS[form]
    G = prm.n_gas_of(prm.default_params(kind))
    for mask in _masks(G):
        rows = _rows(kind, mask)[0]
        for n in COUNTS:
            ld = ld_of(n)
            T_all = _run(lib, "run_fused", kind, dtype, n, ld, 0, rows, "all")["T"][:, :n]      # T of every step: the records' reference
            for stored in STORED:
                want = _run(lib, "run_fused", kind, dtype, n, ld, 0, rows, stored)
                lib.fiveeq_set_row_policy(policy)
                try:
                    got = _run(lib, "run" if mask is None else "run_uniform", kind, dtype, n, ld, 0, rows, stored, mask)
                finally:
                    lib.fiveeq_set_row_policy(ROWS_AUTO)
                _compare(got, want, (kind, form, policy, mask, n, stored))
                _check_records(got["T_stats"], want["T_stats"], T_all, form == "f32_packed", 0, (kind, form, policy, mask, n, stored))
                if stored != "none":
                    assert bool(torch.isfinite(want["T"][:, :n]).all()) and bool((want["C"][:, :, :n] > 0).all())
                    assert bool((want["T"][:, n:] == -7).all())      # the padding of a stored row is never written


# ---- 2. a member sub-range of wider rows -------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["f64", "f32_packed", "f32_scalar"])
def test_member_sub_range_inside_a_larger_ld(lib, form):
    dtype = FORMS[form][0]
    m0 = 256
    for kind in ("multigas", "co2"):
        G = prm.n_gas_of(prm.default_params(kind))
        for mask in _masks(G)[:3]:
            rows = _rows(kind, mask)[0]
            for n in (1, 65, 129, 1000):
                ld = m0 + n + (70 if form != "f32_scalar" else 71)       # even: the packed kernel; odd: the scalar one
                T_all = _run(lib, "run_fused", kind, dtype, n, ld, m0, rows, "all")["T"][:, m0:m0 + n]
                for stored in ("some", "none"):
                    want = _run(lib, "run_fused", kind, dtype, n, ld, m0, rows, stored)
                    got = _run(lib, "run" if mask is None else "run_uniform", kind, dtype, n, ld, m0, rows, stored, mask)
                    _compare(got, want, (kind, form, mask, n, stored))
                    _check_records(got["T_stats"], want["T_stats"], T_all, form == "f32_packed", m0 // 64, (kind, form, mask, n))
                    outside = torch.ones(ld, dtype=torch.bool, device=DEV)
                    outside[m0:m0 + n] = False
                    assert bool((got["R"][:, outside] == 0).all()) and bool((got["S"][:, outside] == 0).all())
                    assert bool((got["R"][:, ~outside] != 0).all())
                    if stored != "none":
                        assert bool((got["C"][:, :, outside] == -7).all()) and bool((got["T"][:, outside] == -7).all())
                        assert bool((got["C"][:, :, ~outside] > 0).all())


# ---- 3. the engine's feature forms -------------------------------------------------------------------------------------------
def _engine(kind, N, dtype, mode, **kw):
    from fiveeqscm_amd.engine import EnsembleEngine
    rows, p, _ = _rows(kind, None)
    G = prm.n_gas_of(p)
    p = dict(p, r0=p["r0"][:, :N], rC=p["rC"][:, :N], rT=p["rT"][:, :N], q=p["q"][:, :N])
    if "forcing" in kw:
        K = kw["forcing"].n_categories
        sc = np.random.default_rng(18).uniform(0.7, 1.3, size=(G + K, N))
        p["f_scale"] = sc[:G]
        if K:
            p["fx_scale"] = sc[G:]
    eng = EnsembleEngine(p, N, _emissions(G), dtype=dtype, device=DEV, per_step_streams=2, **kw)
    eng.run(mode=mode)
    torch.cuda.synchronize()
    out = {k: getattr(eng, k).clone() for k in ("R", "S", "C", "T", "misfit", "T_hist", "T_stats") if getattr(eng, k) is not None}
    parts = len(eng.per_step_launches())
    eng.close()
    return out, parts


def _features():
    from fiveeqscm_amd.constrain import Observations
    from fiveeqscm_amd.forcing import ExternalForcings
    tab = np.zeros((N_STEPS, 4))
    tab[1:3, 2] = 0.5                                   # the reference period: steps 1, 2
    tab[2:7, 0] = 0.01 * np.arange(5)
    tab[2:7, 1] = 4.0                                   # observed steps 2 .. 6; steps 0 and 7 lie outside the window
    tt = np.arange(N_STEPS)
    fx2 = ExternalForcings(np.stack([-0.3 - 0.01 * tt, np.where(tt % 3 == 1, -1.5, 0.0)], 1), ("aerosol", "volcanic"))
    fx0 = ExternalForcings(np.zeros((N_STEPS, 0)))
    return {
        "observations": dict(observations=Observations(tab)),
        "forcing K=0": dict(forcing=fx0),
        "forcing K=2": dict(forcing=fx2),
        "forcing K=2 + observations": dict(forcing=fx2, observations=Observations(tab)),
        "hist": dict(hist=(-0.5, 1.5, 64), collect_stats=True, store_trajectory=False),
        "collect_stats": dict(collect_stats=True),
        "output_steps": dict(output_steps=[1, 2, 6], collect_stats=True),
    }


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("feature", ["observations", "forcing K=0", "forcing K=2", "forcing K=2 + observations", "hist",
                                     "collect_stats", "output_steps"])
def test_engine_feature_forms_match_fused(lib, feature, dtype):
    kw = _features()[feature]
    for kind, N in (("multigas", 1100), ("co2", 129)):       # two launches per step (members [0, 512) and [512, 1100)); one
        if dtype == torch.float32 and N % 2:
            N += 1                                           # (an even count lets fp32 pack)
        got, parts = _engine(kind, N, dtype, "per_step", **kw)
        want, _ = _engine(kind, N, dtype, "fused", **kw)
        assert parts == (2 if N >= 1024 else 1)
        assert set(got) == set(want) and ("misfit" in want) == ("observations" in kw) and ("T_hist" in want) == ("hist" in kw)
        for name in want:
            if name != "T_stats":
                assert _same(got[name], want[name]), (feature, kind, name)
        if "T_stats" in want:                                # (T of every step: these features leave T what the plain run gives)
            T_all = want["T"] if "T" in want and want["T"].shape[0] == N_STEPS else _engine(kind, N, dtype, "fused")[0]["T"]
            _check_records(got["T_stats"], want["T_stats"], T_all, dtype == torch.float32, 0, (feature, kind))
        assert bool(torch.isfinite(want["R"]).all()) and bool((want["R"] != 0).any())
        if "observations" in kw:
            assert bool((want["misfit"] != 0).any())
        if "hist" in kw:
            assert want["T_hist"].sum(1).tolist() == [N] * N_STEPS
        if "forcing" in kw and kw["forcing"].n_categories:   # the scales really act: not the plain run's T
            plain, _ = _engine(kind, N, dtype, "fused")
            assert not torch.equal(plain["T"], want["T"])


# ---- 4. the C oracle ---------------------------------------------------------------------------------------------------------
def test_plain_case_against_the_c_oracle(lib):
    rows, _, want = _rows("multigas", None)
    n = 1000
    for mask in (None, 0):
        got = _run(lib, "run" if mask is None else "run_uniform", "multigas", torch.float64, n, n + 3, 0, rows, "all", mask)
        for name, ref in (("C", want["C"][:, :, :n]), ("T", want["T"][:, :n]), ("R", want["R"][:, :n]), ("S", want["S"][:, :n])):
            a = got[name][..., :n].cpu().numpy()
            err = np.abs(a - ref) / (1e-10 * np.abs(ref) + 1e-13)
            assert np.isfinite(a).all() and err.max() <= 1.0, (mask, name, float(err.max()))
