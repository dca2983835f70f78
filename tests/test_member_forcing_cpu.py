"""Per-member forcing rows and AR(1) noise (include/fiveeq.h "MEMBER FORCING", "AR(1) NOISE ROWS"), the parts that need no GPU:
the NumPy twin of the generator against an independent statement (tests/noise_reference.py), its invariance under member and
step splits, its statistics, the host-side refusals of the new entry points, and the engine's mode rule, byte accounting and
checkpoint identity in pure Python."""
import ctypes
import types

import numpy as np
import pytest

from fiveeqscm_amd import _capi, forcing
from fiveeqscm_amd import params as prm
from fiveeqscm_amd.checkpoint import CheckpointMixin
from fiveeqscm_amd.engine import EnsembleEngine
import noise_reference as ref

SEED = 20261020


def test_the_new_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = _capi.load()
    for base in ("run_mforc", "plan_create_mforc", "noise_rows"):
        for sfx in ("f64", "f32"):
            name = f"fiveeq_{base}_{sfx}"
            assert name in _capi.SIGNATURES and hasattr(lib, name), name
    sig = _capi.SIGNATURES
    forc, mforc = sig["fiveeq_run_forc_f64"][1], sig["fiveeq_run_mforc_f64"][1]
    assert mforc == forc[:-3] + [ctypes.c_void_p, ctypes.c_int32] + forc[-3:]      # run_forc's, then mforc, n_mforc_rows, the tail
    forc, mforc = sig["fiveeq_plan_create_forc_f32"][1], sig["fiveeq_plan_create_mforc_f32"][1]
    assert mforc == forc[:-1] + [ctypes.c_void_p, ctypes.c_int32] + forc[-1:]
    assert lib.fiveeq_abi_version() == 13 and lib.fiveeq_sizeof_model() == 448      # additive: nothing existing changed
    assert any(p.endswith("fiveeq_noise.hpp") for p in _capi.SOURCES)


# ---- the twin ---------------------------------------------------------------------------------------------------------------
def test_the_deviate_in_python_integers():
    """The package twin's deviate against the header's text restated in Python integers; |z| <= 6 and the exact numerator."""
    members, steps = [0, 1, 63, 64, 129, 2 ** 31 - 1, 2 ** 40 + 5], [-1, 0, 1, 7, 749, 2 ** 31 - 2]
    z = forcing._noise_deviates(SEED, members, steps)
    for i, t in enumerate(steps):
        for j, M in enumerate(members):
            num, want = ref.deviate_ints(SEED, M, t)
            assert abs(num) <= 6 * (2 ** 32 - 1) and z[i, j] == want and z[i, j] * 2.0 ** 32 == num, (M, t)
    assert not np.array_equal(z, forcing._noise_deviates(SEED + 1, members, steps))
    with pytest.raises(ValueError):
        forcing._noise_deviates(SEED, [0], [-2])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_twin_invariance_under_member_and_step_splits(dtype):
    n_total, n_steps = 130, 40
    rng = np.random.default_rng(3)
    sigma, phi = rng.uniform(0.1, 0.9, n_total), rng.uniform(-0.5, 0.95, n_total)
    whole = forcing.ar1_noise_rows_host(n_total, n_steps, sigma, phi, seed=SEED, dtype=dtype)
    assert whole.shape == (n_steps, n_total) and whole.dtype == dtype
    assert np.array_equal(whole, ref.noise_rows(SEED, n_total, n_steps, sigma, phi, dtype=dtype))      # the independent statement
    for cuts in ([0, 130], [0, 1, 64, 129, 130], [0, 65, 100, 130], [0, 63, 130]):                   # members
        parts = [forcing.ar1_noise_rows_host(n_total, n_steps, sigma, phi, lo, hi, seed=SEED, dtype=dtype)
                 for lo, hi in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate(parts, axis=1), whole), cuts
    s = sigma * np.sqrt(1.0 - phi * phi)
    members = np.arange(n_total)
    _, xi0 = forcing.ar1_noise_steps_host(SEED, members, -1, 0, phi, sigma, np.zeros(n_total), dtype)
    assert np.array_equal(xi0, np.asarray(sigma, dtype=dtype).astype(np.float64) * forcing._noise_deviates(SEED, members, [-1])[0])
    for cuts in ([1], [7], [1, 7, 39], [20]):                                                        # steps
        xi, parts = xi0, []
        for a, b in zip([0] + cuts, cuts + [n_steps]):
            rows, xi = forcing.ar1_noise_steps_host(SEED, members, a, b, phi, s, xi, dtype)
            parts.append(rows)
        assert np.array_equal(np.concatenate(parts), whole), cuts
        assert np.array_equal(ref.noise_rows(SEED, n_total, n_steps, sigma, phi, dtype=dtype, cuts=cuts), whole), cuts
    if dtype == np.float32:                        # fp32 rows: the fp64 recursion rounded once (phi and s taken in fp32)
        ph32, sg32 = phi.astype(np.float32).astype(np.float64), sigma.astype(np.float32).astype(np.float64)
        s32 = s.astype(np.float32).astype(np.float64)
        xi, want = sg32 * forcing._noise_deviates(SEED, members, [-1])[0], []
        for t in range(n_steps):
            xi = ph32 * xi + s32 * forcing._noise_deviates(SEED, members, [t])[0]
            want.append(xi.astype(np.float32))
        assert np.array_equal(whole, np.stack(want))


@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9])
def test_twin_statistics_within_five_standard_errors(phi):
    """Sample mean, variance and lag-1 autocorrelation of the stationary series at 4096 members x 200 steps against 0, sigma^2
    and phi.  The standard errors come from the AR(1) formulas: with rho_k = phi^k (the series) or phi^2k (its square), the
    variance of a time mean of T terms is v / T * ((1 + rho) / (1 - rho) - 2 rho (1 - rho^T) / (T (1 - rho)^2)); Var(x^2) =
    sigma^4 (2 + kappa) with kappa = -0.1 (1 - phi^2) / (1 + phi^2), the excess kurtosis the sum-of-uniforms deviate leaves in
    x; Bartlett's Var(r_1) = (1 - phi^2) / n for the lag-1 autocorrelation.  Members are independent: divide by N."""
    N, T, sigma = 4096, 200, 0.5
    x = forcing.ar1_noise_rows_host(N, T, sigma, phi, seed=SEED)

    def time_mean_factor(rho):
        return ((1 + rho) / (1 - rho) - 2 * rho * (1 - rho ** T) / (T * (1 - rho) ** 2)) / T

    se_mean = np.sqrt(sigma ** 2 * time_mean_factor(phi) / N)
    kappa = -0.1 * (1 - phi ** 2) / (1 + phi ** 2)
    se_var = np.sqrt(sigma ** 4 * (2 + kappa) * time_mean_factor(phi ** 2) / N)
    se_r1 = np.sqrt((1 - phi ** 2) / (N * (T - 1)))
    mean, var = x.mean(), (x * x).mean()                       # the true mean is 0: the second moment about it
    r1 = (x[1:] * x[:-1]).mean() / var
    print(f"phi {phi}: mean {mean:+.3e} (se {se_mean:.2e}), var {var:.6f} vs {sigma ** 2} (se {se_var:.2e}), "
          f"r1 {r1:.5f} (se {se_r1:.2e})")
    assert abs(mean) <= 5 * se_mean
    assert abs(var - sigma ** 2) <= 5 * se_var
    assert abs(r1 - phi) <= 5 * se_r1
    z = forcing._noise_deviates(SEED, np.arange(N), np.arange(-1, T))
    assert np.abs(z).max() <= 6.0 and np.abs(x).max() <= 6.0 * sigma / (1 - phi) * np.sqrt(1 - phi ** 2) + 6.0 * sigma


def test_generator_arguments_are_validated_on_the_host():
    with pytest.raises(ValueError, match="members"):
        forcing.ar1_noise_rows_host(10, 5, 0.5, 0.5, lo=4, hi=11)
    with pytest.raises(ValueError, match="phi"):
        forcing.ar1_noise_rows_host(10, 5, 0.5, 1.0)
    with pytest.raises(ValueError, match="sigma"):
        forcing.ar1_noise_rows_host(10, 5, -0.5, 0.5)
    with pytest.raises(ValueError, match="a scalar, or a row"):
        forcing.ar1_noise_rows_host(10, 5, np.ones(3), 0.5)
    assert forcing.ar1_noise_rows_host(10, 0, 0.5, 0.5).shape == (0, 10)
    shard = forcing.ar1_noise_rows_host(10, 5, np.full(4, 0.5), np.full(10, 0.5), lo=3, hi=7)      # a shard's row, a design's row
    assert np.array_equal(shard, forcing.ar1_noise_rows_host(10, 5, 0.5, 0.5)[:, 3:7])


# ---- the C ABI's refusals ---------------------------------------------------------------------------------------------------
def _noise(lib, sfx="f64", seed=1, m0=0, n=8, ld=8, t0=0, t1=4, phi=0x1000, s=0x2000, xi=0x3000, rows=0x4000):
    vp = ctypes.c_void_p
    return getattr(lib, "fiveeq_noise_rows_" + sfx)(seed, m0, n, ld, t0, t1, vp(phi), vp(s), vp(xi), vp(rows), None)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_noise_rows_refuses_bad_arguments_before_any_launch(sfx):
    lib = _capi.load()
    cases = [
        (dict(phi=0), "phi is NULL"), (dict(s=0), "s is NULL"), (dict(xi=0), "xi_state is NULL"), (dict(rows=0), "rows is NULL"),
        (dict(phi=0x1002), "phi must be"), (dict(s=0x2001), "s must be"), (dict(xi=0x3004), "xi_state must be 8-byte"),
        (dict(rows=0x4001), "rows must be"),
        (dict(t0=3, t1=2), "step range"), (dict(t0=-2, t1=0), "step range"), (dict(t0=-1, t1=1), "step range"),
        (dict(t0=-1, t1=-1), "step range"),
        (dict(n=9), "ld=8 < n_members=9"), (dict(n=0), "n_members"), (dict(m0=-1), "m0=-1"),
    ]
    for kw, needle in cases:
        rc = _noise(lib, sfx, **kw)
        msg = lib.fiveeq_last_error().decode()
        assert rc == _capi.E_INVALID and needle in msg, (kw, rc, msg)
    assert _noise(lib, sfx, t0=2, t1=2) == _capi.OK                       # an empty range: nothing launched


def _mforc(lib, sfx="f64", n_gas=3, plan=False, n=8, ld=8, n_steps=4, t0=0, t1=4, ptr=0x1000, fscale=0x2000, fext=0x3000,
           n_fext=2, obs=None, misfit=None, mforc=0x6000, n_mforc_rows=4, form=_capi.FORM_PER_STEP, k_steps=0):
    model = prm.make_model(prm.default_params("multigas"))
    model.n_gas = n_gas                              # 2: pools 4 + 1, a compiled layout without the forcing forms
    p, vp = ctypes.c_void_p(ptr), ctypes.c_void_p
    head = (ctypes.byref(model), n, ld, p, n_steps, t0, t1, p, p, p, p, None, None, 0, None, vp(fscale), vp(fext), n_fext,
            vp(obs), vp(misfit), vp(mforc), n_mforc_rows)
    if plan:
        out = ctypes.c_void_p(0xDEAD)
        rc = getattr(lib, "fiveeq_plan_create_mforc_" + sfx)(*head, ctypes.byref(out))
        assert out.value is None                    # no plan comes back from a refused call
        return rc
    return getattr(lib, "fiveeq_run_mforc_" + sfx)(*head, form, k_steps, None)


@pytest.mark.parametrize("plan", [False, True])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_run_mforc_refuses_bad_arguments_before_any_launch(sfx, plan):
    """The member-forcing rows' own refusals, and fiveeq_run_forc's through the shared checks, in its order: every call
    returns on the host with FIVEEQ_E_INVALID (the fake pointers are never dereferenced), so this runs without a GPU."""
    lib = _capi.load()
    cases = [
        (dict(mforc=0), "mforc is NULL"),
        (dict(mforc=0x6001), "mforc must be"),
        (dict(n_mforc_rows=3), "n_mforc_rows=3 < t_end=4"),
        (dict(n_mforc_rows=0, t1=1), "n_mforc_rows=0 < t_end=1"),
        (dict(n_gas=2), "has no forcing form"),
        (dict(fscale=0), "fscale is NULL"),
        (dict(fscale=0, mforc=0), "fscale is NULL"),                   # the scales are checked first
        (dict(fext=0, n_fext=1), "fext is NULL with n_fext=1"),
        (dict(n_fext=5), "n_fext=5 outside 0..4"),
        (dict(obs=0x4000), "obs and misfit go together"),
        (dict(obs=0x4000, mforc=0), "mforc is NULL"),                  # ... and the rows before the misfit pair
        (dict(obs=0x4001, misfit=0x5000), "8-byte aligned"),
        (dict(n=0), "n_members"),
        (dict(ld=4), "ld="),
        (dict(ptr=0), "NULL device pointer"),
        (dict(t0=3, t1=2), "step range"),
        (dict(t1=5, n_mforc_rows=5), "step range"),
    ]
    if not plan:
        cases += [(dict(form=2), "form=2"), (dict(k_steps=-1), "k_steps=-1")]
    for kw, needle in cases:
        rc = _mforc(lib, sfx, plan=plan, **kw)
        msg = lib.fiveeq_last_error().decode()
        assert rc == _capi.E_INVALID, (kw, rc, msg)
        assert needle in msg, (kw, msg)
    if not plan:                                     # unit scales with no category and no table: allowed (an empty range launches nothing)
        assert _mforc(lib, sfx, fext=0, n_fext=0, t0=2, t1=2) == _capi.OK


# ---- the engine's rules, in pure Python ------------------------------------------------------------------------------------
def _bare_engine(member_forcing, forcing_rows=0, dtype_bytes=8, observations=None):
    """An EnsembleEngine that never saw a GPU: the attributes mode_refusal(), resolve_mode() and bytes_per_member_step() read."""
    eng = EnsembleEngine.__new__(EnsembleEngine)
    eng.__dict__.update(
        T_hist=None, compensated=False, scenario_axis=False, forcing=object() if forcing_rows else None,
        observations=observations, member_forcing=member_forcing, concentration_driven=False, small_widest=8,
        small_lanes="auto", collect_stats=False, _w=dtype_bytes, n_gas=3, sum_pools=6, n_rows=0, n_steps=100, C=None,
        n_members=1000, n_scenarios=1, fused_span=None,
        fscale=types.SimpleNamespace(shape=(forcing_rows, 1000)) if forcing_rows else None,
        _unit_fscale=types.SimpleNamespace(shape=(3, 1000)) if member_forcing is not None and not forcing_rows else None)
    return eng


def test_mode_small_is_refused_and_auto_never_takes_it():
    eng = _bare_engine(member_forcing=object())
    for mode in ("per_step", "graph", "fused", "ksteps"):
        assert eng.mode_refusal(mode) is None
    assert "member_forcing=" in eng.mode_refusal("small")
    assert eng.small_form() == 0
    assert eng.resolve_mode("auto")[0] in ("per_step", "ksteps")          # 1000 members are launch-bound: never 'small'
    assert _bare_engine(None).mode_refusal("small") is None
    both = _bare_engine(member_forcing=object(), forcing_rows=5)
    assert "forcing scales" in both.mode_refusal("small")                 # the first rule that applies is reported


@pytest.mark.parametrize("w", [8, 4])
def test_byte_accounting_adds_one_word_per_member_step_in_every_form(w):
    plain = _bare_engine(None, dtype_bytes=w)
    forc = _bare_engine(None, forcing_rows=5, dtype_bytes=w)                   # G + K = 3 + 2 scale rows
    alone = _bare_engine(object(), dtype_bytes=w)                              # unit scales: G rows
    both = _bare_engine(object(), forcing_rows=5, dtype_bytes=w)
    assert plain.bytes_per_member_step("per_step") == w * 27                   # 2 SP + 3 G + 6, nothing stored
    assert forc.bytes_per_member_step("per_step") == w * (27 + 5)
    assert both.bytes_per_member_step("per_step") == forc.bytes_per_member_step("per_step") + w
    assert alone.bytes_per_member_step("per_step") == w * (27 + 3) + w
    for mode, k in (("fused", None), ("ksteps", 8)):                          # streamed, not resident: w per step here too
        assert both.bytes_per_member_step(mode, k) == forc.bytes_per_member_step(mode, k) + w
        assert alone.bytes_per_member_step(mode, k) == plain.bytes_per_member_step(mode, k) + w + w * 3 / (k or 100)
    if w == 8:                                                                  # the ratio DESIGN.md prices the per-step form at
        stored = 8 * (3 + 1)
        assert (both.bytes_per_member_step("per_step") + stored) / (forc.bytes_per_member_step("per_step") + stored) == \
            (248 + 8 * 5 + 8) / (248 + 8 * 5)


class _Stub(CheckpointMixin):
    """The attributes load_state_dict() reads before it validates the member_forcing identity."""
    cumE = misfit = observations = forcing = R = S = None
    scenario_axis = collect_stats = False

    def __init__(self, rows):
        self.member_forcing = rows

    def member_forcing_sha256(self):
        import hashlib
        return None if self.member_forcing is None else hashlib.sha256(np.asarray(self.member_forcing).tobytes()).hexdigest()


def test_a_checkpoint_of_other_member_forcing_rows_is_refused():
    rows = forcing.ar1_noise_rows_host(6, 5, 0.5, 0.6)
    mine = _Stub(rows)
    state = {"member_forcing_sha256": mine.member_forcing_sha256()}
    for other in (_Stub(rows * 2.0), _Stub(forcing.ar1_noise_rows_host(6, 5, 0.5, 0.6, seed=1)), _Stub(None)):
        with pytest.raises(ValueError, match="member_forcing rows"):
            other.load_state_dict(state)
    with pytest.raises(ValueError, match="member_forcing rows"):
        mine.load_state_dict({})                                  # a checkpoint of a run without member_forcing=
    with pytest.raises(KeyError, match="'R'"):
        mine.load_state_dict(state)                               # the same rows pass the check and go on to the state
