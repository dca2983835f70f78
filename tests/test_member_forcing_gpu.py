"""Per-member forcing rows and the AR(1) generator on the MI355X (include/fiveeq.h "MEMBER FORCING", "AR(1) NOISE ROWS"): the
generator against its NumPy twin bit for bit (member offsets, step cuts, guard columns, fp32 rounded once); the stepping forms
against fiveeq_run_forc_* for zero and member-uniform rows, against the frozen oracle member by member for distinct rows, and
among themselves; guard columns; resampled(plan); the constructor's refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from fiveeqscm_amd import _capi, constrain, emissions
from fiveeqscm_amd import params as prm
from fiveeqscm_amd.constrain import Observations
from fiveeqscm_amd.engine import ConcentrationDrivenEngine, EnsembleEngine
from fiveeqscm_amd.forcing import ExternalForcings, ar1_noise_rows
from oracle import fiveeq_oracle as npo
import noise_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 20261020
N_STEPS = 24
GASES = {"co2": 1, "multigas": 3}
KINDS = ["co2", "multigas"]                       # pool layouts {4} and 4 + 1 + 1
DTYPES = [torch.float64, torch.float32]
NS = [65, 129, 130]                               # odd N, the packed tail, a partial wave
NP_OF = {torch.float64: np.float64, torch.float32: np.float32}
SENTINEL = -777.25


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


# ---- the generator ----------------------------------------------------------------------------------------------------------
def _generate(dtype, N, ld, m0, phi, s, xi, t0, t1):
    """One fiveeq_noise_rows_* call into guarded buffers of row length ld: (rows [t1 - t0, ld], xi [ld]) on the host."""
    lib = _capi.load()
    pad = lambda a, dt: torch.cat([torch.from_numpy(a), torch.full((ld - N,), SENTINEL, dtype=torch.float64)]).to(DEV, dt)  # noqa: E731
    phi_d, s_d, xi_d = pad(phi, dtype), pad(s, dtype), pad(xi, torch.float64)
    rows = torch.full((max(t1 - t0, 0), ld), SENTINEL, dtype=dtype, device=DEV)
    fn = getattr(lib, "fiveeq_noise_rows_" + ("f64" if dtype == torch.float64 else "f32"))
    with torch.cuda.device(DEV):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _capi.check(lib, fn(SEED, m0, N, ld, t0, t1, _ptr(phi_d), _ptr(s_d), _ptr(xi_d), _ptr(rows) if t0 >= 0 else None, st))
    torch.cuda.synchronize()
    return rows.cpu().numpy(), xi_d.cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_generator_equals_the_twin_and_leaves_the_guards(N, dtype):
    ld, n_steps, npd = (N + 63) // 64 * 64 + 64, 12, NP_OF[dtype]
    rng = np.random.default_rng(N)
    for m0 in (0, 64, 100):
        sigma, phi = rng.uniform(0.1, 0.9, N), rng.uniform(-0.5, 0.95, N)
        s = sigma * np.sqrt(1.0 - phi * phi)
        _, xi0 = _generate(dtype, N, ld, m0, phi, sigma, np.zeros(N), -1, 0)          # the start call stores no row
        _, want0 = ref.noise_steps(SEED, m0, N, -1, 0, phi, sigma, np.zeros(N), npd)
        assert np.array_equal(xi0[:N], want0) and (xi0[N:] == SENTINEL).all(), m0
        want, want_xi = ref.noise_steps(SEED, m0, N, 0, n_steps, phi, s, want0, npd)
        got, xi = _generate(dtype, N, ld, m0, phi, s, xi0[:N], 0, n_steps)
        assert got.dtype == npd and np.array_equal(got[:, :N], want) and np.array_equal(xi[:N], want_xi), (m0, "whole")
        assert (got[:, N:] == SENTINEL).all() and (xi[N:] == SENTINEL).all(), (m0, "guards")
        parts, x = [], xi0[:N]                                                        # the range cut at steps 1 and 7
        for a, b in ((0, 1), (1, 7), (7, n_steps)):
            rows, x_ld = _generate(dtype, N, ld, m0, phi, s, x, a, b)
            parts.append(rows[:, :N])
            x = x_ld[:N]
        assert np.array_equal(np.concatenate(parts), want) and np.array_equal(x, want_xi), (m0, "cut")
        if dtype == torch.float32:                                                    # the fp64 recursion rounded once
            wide, _ = ref.noise_steps(SEED, m0, N, 0, n_steps, phi.astype(np.float32), s.astype(np.float32), want0, np.float64)
            assert np.array_equal(got[:, :N], wide.astype(np.float32)), m0


@pytest.mark.parametrize("dtype", DTYPES)
def test_ar1_noise_rows_is_its_host_twin_for_any_shard(dtype):
    from fiveeqscm_amd.forcing import ar1_noise_rows_host
    n_total, rng = 300, np.random.default_rng(1)
    sigma, phi = rng.uniform(0.1, 0.9, n_total), rng.uniform(-0.5, 0.95, n_total)
    whole = ar1_noise_rows(n_total, N_STEPS, sigma, phi, seed=SEED, device=DEV, dtype=dtype)
    assert whole.dtype == dtype and np.array_equal(whole.cpu().numpy(),
                                                   ar1_noise_rows_host(n_total, N_STEPS, sigma, phi, seed=SEED, dtype=NP_OF[dtype]))
    for lo, hi in ((0, 100), (100, 229), (229, 300)):
        part = ar1_noise_rows(n_total, N_STEPS, sigma, phi, lo, hi, seed=SEED, device=DEV, dtype=dtype)
        assert torch.equal(part, whole[:, lo:hi]), (lo, hi)


# ---- the stepping forms -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(kind, N):
    """(params with non-unit f_scale / fx_scale rows, E, a two-category table, F_ext > 0): no F_ext equal to -0."""
    G = GASES[kind]
    base = prm.default_params(kind)
    p = prm.sample_ensemble_shard(base, N)
    s = prm.sample_forcing_scales(base, N, ranges=[(0.8, 1.2)] * G + [(0.3, 2.0), (0.5, 1.5)], seed=7)
    p["f_scale"], p["fx_scale"] = s[:G], s[G:]
    E = emissions.rcp_like_emissions(N_STEPS, G)
    tt = np.arange(N_STEPS)
    fx = ExternalForcings(np.stack([-0.9 * (tt + 1) / N_STEPS, np.where(tt % 7 == 5, -2.5, 0.0)], 1), ("aerosol", "volcanic"))
    return p, E, fx, 0.02 * (tt + 1) / N_STEPS


def _plain(p):
    return {k: v for k, v in p.items() if k not in ("f_scale", "fx_scale")}


@functools.lru_cache(maxsize=None)
def _noise(N, dtype):
    """Twin noise with sigma = 0.5, phi = 0.6, [N_STEPS, N] on the host in the kernel precision."""
    return ref.noise_rows(SEED, N, N_STEPS, 0.5, 0.6, dtype=NP_OF[dtype])


@functools.lru_cache(maxsize=None)
def _obs():
    rng = np.random.default_rng(11)
    table = np.zeros((N_STEPS, 4))
    table[:, 0] = rng.normal(0.2, 0.1, N_STEPS)
    table[10:21, 1] = 1.0 / rng.uniform(0.05, 0.2, 11) ** 2
    table[3:8, 2] = 1.0 / 5
    return Observations(table)


def _dev(rows, dtype):
    return torch.from_numpy(np.ascontiguousarray(rows)).to(DEV, dtype)


def _run(p, N, E, mode="per_step", split=None, **kw):
    """{C, T, R, S[, misfit]} on the host after a run of every step in `mode`, or in two calls cut at `split`."""
    eng = EnsembleEngine(p, N, E, device=DEV, **kw)
    k = {"k_steps": 5} if mode == "ksteps" else {}
    if split:
        eng.run(0, split, mode=mode, **k)
        eng.run(split, N_STEPS, mode=mode, **k)
    else:
        eng.run(mode=mode, **k)
    torch.cuda.synchronize()
    out = {name: getattr(eng, name).cpu() for name in ("C", "T", "R", "S")}
    if eng.misfit is not None:
        out["misfit"] = eng.misfit.cpu()
    eng.close()
    return out


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_zero_rows_are_the_forcing_run_bit_for_bit(kind, dtype, N):
    p, E, fx, Fx = _case(kind, N)
    zeros = torch.zeros((N_STEPS, N), dtype=dtype, device=DEV)
    for forcing, params in ((fx, p), (ExternalForcings(np.zeros((N_STEPS, 0))), _plain(p))):
        kw = dict(F_ext=Fx, dtype=dtype, forcing=forcing, observations=_obs())
        for mode in ("per_step", "fused"):
            want = _run(params, N, E, mode, **kw)
            assert want["T"].abs().sum() > 0 and want["misfit"].abs().sum() > 0
            assert _same(_run(params, N, E, mode, member_forcing=zeros, **kw), want), (mode, forcing.n_categories)
    alone = _run(_plain(p), N, E, F_ext=Fx, dtype=dtype, member_forcing=zeros)       # without forcing=: the plain run
    assert _same(alone, _run(_plain(p), N, E, F_ext=Fx, dtype=dtype))


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_member_uniform_rows_are_a_shifted_external_forcing(kind, dtype, N):
    """Rows uniform over the members, x_t, against the existing run with F_ext'[t] = fl(F_ext[t] + x_t) formed in the kernel
    precision (the engine rounds F_ext to it first, the rows are given in it)."""
    p, E, fx, Fx = _case(kind, N)
    npd = NP_OF[dtype]
    x = ref.noise_rows(SEED, 1, N_STEPS, 0.5, 0.6, dtype=npd)[:, 0]
    shifted = (Fx.astype(npd) + x).astype(np.float64)             # one add in the kernel precision
    rows = _dev(np.repeat(x[:, None], N, axis=1), dtype)
    kw = dict(dtype=dtype, forcing=fx, observations=_obs())
    for mode in ("per_step", "fused"):
        want = _run(p, N, E, mode, F_ext=shifted, **kw)
        got = _run(p, N, E, mode, F_ext=Fx, member_forcing=rows, **kw)
        assert _same(got, want), mode
        assert not torch.equal(want["T"], _run(p, N, E, mode, F_ext=Fx, **kw)["T"])          # the rows do something


@functools.lru_cache(maxsize=None)
def _oracle(kind, N, dtype):
    """The frozen oracle, member by member, on scaled coefficients and F_ext + X @ sx + member_forcing[:, m]."""
    G = GASES[kind]
    p, E, fx, Fx = _case(kind, N)
    rows = _noise(N, dtype).astype(np.float64)
    base_f = np.asarray(prm.default_params(kind)["f"], float).reshape(G, 3)
    C, T = np.empty((N_STEPS, G, N)), np.empty((N_STEPS, N))
    for m in range(N):
        pm = _plain(p)
        for k in ("r0", "rC", "rT", "q"):
            pm[k] = np.asarray(p[k])[:, m:m + 1]
        pm["f"] = base_f * p["f_scale"][:, m][:, None]
        o = npo.run(E, pm, 1, F_ext=Fx + fx.table @ p["fx_scale"][:, m] + rows[:, m])
        C[:, :, m], T[:, m] = o["C"][:, :, 0], o["T"][:, 0]
    return C, T


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_distinct_rows_fp64_against_the_oracle_member_by_member(kind, N):
    p, E, fx, Fx = _case(kind, N)
    C_ref, T_ref = _oracle(kind, N, torch.float64)
    rows = _dev(_noise(N, torch.float64), torch.float64)
    for mode in ("per_step", "fused"):
        got = _run(p, N, E, mode, F_ext=Fx, forcing=fx, member_forcing=rows)
        for name, a, b in (("C", got["C"].numpy(), C_ref), ("T", got["T"].numpy(), T_ref)):
            err = np.abs(a - b) / (1e-10 * np.abs(b) + 1e-13)
            print(f"{kind} N={N} {mode} {name}: worst err/bound {err.max():.3g}")
            assert np.isfinite(a).all() and err.max() <= 1.0, (mode, name, float(err.max()))


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_distinct_rows_fp32_against_the_oracle(kind, N):
    """The project's fp32 bounds, as tests/test_forcing_gpu.py takes them: C 5e-6 relative, T 3e-5 relative + 2e-6 K; the
    oracle reads the fp32 rows the kernel reads."""
    p, E, fx, Fx = _case(kind, N)
    C_ref, T_ref = _oracle(kind, N, torch.float32)
    rows = _dev(_noise(N, torch.float32), torch.float32)
    for mode in ("per_step", "fused"):
        got = _run(p, N, E, mode, F_ext=Fx, forcing=fx, member_forcing=rows, dtype=torch.float32)
        C, T = got["C"].double().numpy(), got["T"].double().numpy()
        errC = (np.abs(C - C_ref) / np.abs(C_ref)).max()
        errT = (np.abs(T - T_ref) / (3e-5 * np.abs(T_ref) + 2e-6)).max()
        print(f"fp32 {kind} N={N} {mode}: C worst rel {errC:.3g} (bound 5e-6), T worst err/bound {errT:.3g}")
        assert np.isfinite(C).all() and np.isfinite(T).all() and errC <= 5e-6 and errT <= 1.0, (mode, float(errC), float(errT))


@pytest.mark.parametrize("with_forcing", [False, True])
@pytest.mark.parametrize("with_obs", [False, True])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_form_gives_the_same_bits(kind, dtype, N, with_obs, with_forcing):
    p, E, fx, Fx = _case(kind, N)
    rows = _dev(_noise(N, dtype), dtype)
    kw = dict(F_ext=Fx, dtype=dtype, member_forcing=rows, observations=_obs() if with_obs else None,
              forcing=fx if with_forcing else None)
    params = p if with_forcing else _plain(p)
    want = _run(params, N, E, "per_step", **kw)
    assert want["T"].abs().sum() > 0 and ("misfit" in want) == with_obs
    without = _run(params, N, E, "per_step", **dict(kw, member_forcing=None))
    assert not torch.equal(without["T"], want["T"])                # the rows do something
    for mode in ("graph", "fused", "ksteps"):
        assert _same(_run(params, N, E, mode, **kw), want), mode
    for mode in ("per_step", "fused"):                             # the step range cut in two calls
        assert _same(_run(params, N, E, mode, split=7, **kw), want), (mode, "split")
    if dtype == torch.float32:                                     # packed lanes (even N) and scalar lanes: the same bits
        lib = _capi.load()
        prev = lib.fiveeq_set_f32_packing(0)
        try:
            assert _same(_run(params, N, E, "per_step", **kw), want) and _same(_run(params, N, E, "fused", **kw), want)
        finally:
            lib.fiveeq_set_f32_packing(prev)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_resume_through_a_checkpoint_is_bit_identical(kind, dtype):
    N = 130
    p, E, fx, Fx = _case(kind, N)
    rows = _dev(_noise(N, dtype), dtype)
    kw = dict(F_ext=Fx, dtype=dtype, forcing=fx, observations=_obs(), member_forcing=rows, device=DEV)
    want = _run(p, N, E, "per_step", **{k: v for k, v in kw.items() if k != "device"})
    first = EnsembleEngine(p, N, E, **kw)
    first.run(0, 9, mode="fused")
    state = first.state_dict()
    assert state["member_forcing_sha256"] == first.member_forcing_sha256() and len(state["member_forcing_sha256"]) == 64
    first.close()
    second = EnsembleEngine(p, N, E, **kw)
    second.load_state_dict(state)
    second.run(state["t_next"], N_STEPS, mode="per_step")
    torch.cuda.synchronize()
    for name in ("R", "S", "misfit"):
        assert torch.equal(getattr(second, name).cpu(), want[name]), name
    assert torch.equal(second.T[9:].cpu(), want["T"][9:]) and torch.equal(second.C[9:].cpu(), want["C"][9:])
    other = EnsembleEngine(p, N, E, **dict(kw, member_forcing=rows * 2))
    with pytest.raises(ValueError, match="member_forcing rows"):
        other.load_state_dict(state)
    plain = EnsembleEngine(p, N, E, **dict(kw, member_forcing=None))
    with pytest.raises(ValueError, match="member_forcing rows"):
        plain.load_state_dict(state)
    for eng in (second, other, plain):
        eng.close()


@pytest.mark.parametrize("form", [_capi.FORM_PER_STEP, _capi.FORM_FUSED])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_guard_columns_of_every_row_stay_untouched(kind, dtype, N, form):
    """Members [0, N) of rows of length ld = N + 63 or N + 64 (even: fp32 lanes pack, and an odd N ends in a half-filled
    lane) through the C ABI: the N members' bits are those of an engine of exactly N members, and columns [N, ld) of R, S,
    C, T and misfit keep the sentinel."""
    ld = N + 63 if N % 2 else N + 64
    p, E, fx, Fx = _case(kind, N)
    wide = dict(_plain(p))
    for k in ("r0", "rC", "rT", "q", "f_scale", "fx_scale"):
        wide[k] = np.concatenate([np.asarray(p[k]), np.repeat(np.asarray(p[k])[:, :1], ld - N, axis=1)], axis=1)
    noise = _noise(N, dtype)
    rows = _dev(np.concatenate([noise, np.full((N_STEPS, ld - N), 1e30, dtype=noise.dtype)], axis=1), dtype)
    kw = dict(F_ext=Fx, dtype=dtype, forcing=fx, observations=_obs())
    want = _run(p, N, E, "per_step", member_forcing=_dev(noise, dtype), **kw)
    eng = EnsembleEngine(wide, ld, E, device=DEV, member_forcing=rows, **kw)
    for t in (eng.R, eng.S, eng.C, eng.T, eng.misfit):
        t[..., N:] = SENTINEL
    args = eng._run_args(0, N_STEPS, 0, N) + (eng._ptr(eng.fscale), eng._ptr(eng.fext), 2, *eng._obs_args(),
                                              eng._ptr(eng.member_forcing), N_STEPS)
    _capi.check(eng.lib, eng._fn("run_mforc")(*args, form, 5 if form == _capi.FORM_FUSED else 0, eng._stream()))
    torch.cuda.synchronize()
    for name in ("R", "S", "C", "T", "misfit"):
        got = getattr(eng, name).cpu()
        assert torch.equal(got[..., :N], want[name]), name
        assert bool((got[..., N:] == SENTINEL).all()), (name, "guard")
    eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_resampled_plan_continues_bit_for_bit(kind, dtype):
    """A plan that repeats and drops members, then 6 more steps: the fresh engine built from the gathered columns equals the
    source engine's continued members."""
    N, t_cut = 130, N_STEPS - 6
    p, E, fx, Fx = _case(kind, N)
    rows = _dev(_noise(N, dtype), dtype)
    kw = dict(F_ext=Fx, dtype=dtype, forcing=fx, device=DEV)
    eng = EnsembleEngine(p, N, E, member_forcing=rows, **kw)
    eng.run(0, t_cut, mode="per_step")
    w = torch.from_numpy(np.random.default_rng(5).integers(0, 4, N) * (np.arange(N) % 3 != 1)).to(DEV)
    plan = constrain.resample(w, 97, seed=3)
    src = plan.src.cpu().numpy()
    assert np.unique(src).size < src.size and np.unique(src).size < N              # repeats and drops
    params, R0, S0, mf = eng.resampled(plan)
    assert tuple(mf.shape) == (N_STEPS, 97) and torch.equal(mf.cpu(), rows.cpu()[:, src])
    eng.run(t_cut, N_STEPS, mode="fused")
    fresh = EnsembleEngine(params, plan.n_members, E, R0=R0, S0=S0, member_forcing=mf, **kw)
    fresh.run(t_cut, N_STEPS, mode="per_step")
    torch.cuda.synchronize()
    for name in ("R", "S"):
        assert torch.equal(getattr(fresh, name).cpu(), getattr(eng, name).cpu()[:, src]), name
    assert torch.equal(fresh.T[t_cut:].cpu(), eng.T[t_cut:].cpu()[:, src])
    assert torch.equal(fresh.C[t_cut:].cpu(), eng.C[t_cut:].cpu()[:, :, src])
    eng.close()
    fresh.close()


def test_constructor_and_mode_refusals_and_byte_accounting():
    N = 130
    p, E, fx, Fx = _case("multigas", N)
    rows = _dev(_noise(N, torch.float64), torch.float64)
    refusals = [
        (dict(hist=(-1.0, 3.0, 64)), "member_forcing= cannot be combined with hist="),
        (dict(concentration_driven=True), "member_forcing= cannot be combined with concentration_driven"),
        (dict(compensated=True, dtype=torch.float32, member_forcing=rows.float()), "member_forcing= cannot be combined with compensated"),
    ]
    for kw, needle in refusals:
        with pytest.raises(ValueError, match=needle):
            EnsembleEngine(_plain(p), N, E, F_ext=Fx, device=DEV, **{"member_forcing": rows, **kw})
    with pytest.raises(ValueError, match="member_forcing= cannot be combined with emissions of several scenarios"):
        EnsembleEngine(_plain(p), N, np.stack([E, E]), member_forcing=rows, device=DEV)
    with pytest.raises(ValueError, match="member_forcing= cannot be combined with concentration_driven"):
        ConcentrationDrivenEngine(p, N, np.full((N_STEPS, 3), 300.0), forcing=fx, member_forcing=rows, device=DEV)
    for bad in (rows[:-1], rows[:, :-1], rows.float(), rows.cpu(), rows.cpu().numpy()):
        with pytest.raises(ValueError, match="member_forcing: want a tensor"):
            EnsembleEngine(_plain(p), N, E, member_forcing=bad, device=DEV)
    eng = EnsembleEngine(p, N, E, F_ext=Fx, forcing=fx, member_forcing=rows, device=DEV)
    forc = EnsembleEngine(p, N, E, F_ext=Fx, forcing=fx, device=DEV)
    assert forc.bytes_per_member_step("per_step") == 248.0 + 8 * 5
    assert eng.bytes_per_member_step("per_step") == 248.0 + 8 * 5 + 8
    assert eng.bytes_per_member_step("ksteps", 8) == forc.bytes_per_member_step("ksteps", 8) + 8
    assert eng.bytes_per_member_step("fused") == forc.bytes_per_member_step("fused") + 8
    assert eng.chunk_members == forc.chunk_members                # the rows are streamed: the chunk-major schedule does not count them
    assert eng.small_form() == 0 and eng.resolve_mode("auto")[0] in ("per_step", "ksteps")
    with pytest.raises(ValueError, match="mode 'small'"):
        eng.run(mode="small")
    with pytest.raises(ValueError, match="member_forcing"):
        eng.forcing_rows()
    alone = EnsembleEngine(_plain(p), N, E, member_forcing=rows, device=DEV)
    assert alone.fscale is None and alone.bytes_per_member_step("per_step") == 248.0 + 8 * 3 + 8
    with pytest.raises(ValueError, match="does not carry the per-member forcing rows of member_forcing="):
        alone.run(mode="small")
    for e in (eng, forc, alone):
        e.close()
