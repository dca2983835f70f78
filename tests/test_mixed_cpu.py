"""The mixed drive — emission-driven and concentration-driven gases in one run (include/fiveeq.h "MIXED DRIVE",
fiveeq_run_mixed_*, MixedDriveEngine) — the parts that need no GPU: the new symbols, every host-side refusal in the documented
order, the references of tests/mixed_reference.py against each other and against the 50-digit step (K_MIXED: the yardstick of
tests/test_mixed_gpu.py), the proof that the yardstick sees each of three mistakes, and the host plumbing (make_drive's per-gas
form, MixedDriveEngine's argument refusals, the checkpoint's mask)."""
import ctypes

import numpy as np
import pytest

import inverse_reference as ir
import mixed_reference as mx
import step_reference as sr
from fiveeqscm_amd import _capi, emissions
from fiveeqscm_amd import params as prm
from fiveeqscm_amd.checkpoint import CheckpointMixin
from oracle import fiveeq_oracle as npo

BOUND = 8.0            # the single-step bound's factor (tests/test_step_edges_gpu.py): |got - ref| <= 8 max(K, 1) eps scale

# The NumPy twin's worst anchored-step error over the 12 steps x 16 members, per case and mask, in units of eps64 x scale (printed
# by test_the_twin_agrees_with_the_50_digit_step_at_every_step, which holds the figures to these constants: they cover the
# measurement and exceed it by less than a unit).  Order: X, T, R, S, cum.  cum is that of the concentration-driven gases (an
# emission-driven gas's must be met exactly: scale 0).  Measured 2026-10-20.
_K_ROWS = {
    "4+1+1": {
        0b001: (0.50, 0.45, 1.90, 0.55, 0.05), 0b010: (0.45, 0.60, 1.55, 0.60, 0.15), 0b011: (0.45, 0.45, 1.35, 0.50, 0.15),
        0b100: (0.45, 0.60, 1.65, 0.55, 0.05), 0b101: (0.40, 0.40, 1.40, 0.40, 0.05), 0b110: (0.50, 0.55, 1.35, 0.55, 0.15)},
    "multigas dt=0.5": {
        0b001: (0.50, 0.45, 1.40, 0.45, 0.05), 0b010: (0.50, 0.60, 1.25, 0.65, 0.10), 0b011: (0.50, 0.45, 1.50, 0.45, 0.10),
        0b100: (0.45, 0.65, 1.35, 0.65, 0.05), 0b101: (0.35, 0.40, 1.05, 0.40, 0.05), 0b110: (0.45, 0.55, 1.45, 0.55, 0.10)},
}
K_MIXED = {name: {mask: dict(zip(mx.OUTPUTS, row)) for mask, row in rows.items()} for name, rows in _K_ROWS.items()}


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = _capi.load()
    for name in ("fiveeq_run_mixed_f64", "fiveeq_run_mixed_f32", "fiveeq_mixed_layout_supported"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES, name
    for sfx in ("f64", "f32"):
        # the arguments of fiveeq_run_inverse_forc_* with conc_mask behind T_stats
        forc = _capi.SIGNATURES["fiveeq_run_inverse_forc_" + sfx][1]
        assert _capi.SIGNATURES["fiveeq_run_mixed_" + sfx][1] == forc[:16] + [ctypes.c_int32] + forc[16:]
    assert lib.fiveeq_abi_version() == 13 and lib.fiveeq_sizeof_model() == 448      # additive: nothing existing changed


def _pools(lib, pools, mask):
    return lib.fiveeq_mixed_layout_supported(len(pools), (ctypes.c_int32 * len(pools))(*pools), mask)


def test_which_masks_a_layout_runs():
    lib = _capi.load()
    for pools in ((4, 1, 1), (4, 4, 4), (4, 1), (4,), (1, 1, 1)):
        full = (1 << len(pools)) - 1
        assert _pools(lib, pools, 0) == 1 and _pools(lib, pools, full) == 1        # the forward and the inverse kernels
        assert _pools(lib, pools, -1) == 0 and _pools(lib, pools, full + 1) == 0
        for mask in range(1, full):
            assert _pools(lib, pools, mask) == (1 if pools == (4, 1, 1) else 0), (pools, mask)
    assert _pools(lib, (5, 1, 1), 0) == 0                                          # not a compiled layout at all


def _call(lib, sfx, kind="multigas", n_gas=3, n=8, ld=8, n_steps=4, t0=0, t1=4, ptr=0x1000, cumE=0x1800, mask=0b110,
          fscale=0x2000, fext=0x3000, n_fext=2, obs=0x4000, misfit=0x5000):
    p = prm.default_params("multigas")
    if kind == "444":                                # pools 4 + 4 + 4: a compiled layout without the mixed form
        p["a"], p["tau"] = np.tile(p["a"][0], (3, 1)), np.tile(p["tau"][0], (3, 1))
    model = prm.make_model(p)
    model.n_gas = n_gas                              # 2: pools 4 + 1, a compiled layout with none of the three forms
    q, vp = ctypes.c_void_p(ptr), ctypes.c_void_p
    rc = getattr(lib, "fiveeq_run_mixed_" + sfx)(ctypes.byref(model), n, ld, q, n_steps, t0, t1, q, q, q, q, vp(cumE), None, None, 0,
                                                 None, mask, vp(fscale), vp(fext), n_fext, vp(obs), vp(misfit), None)
    return rc, lib.fiveeq_last_error().decode()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_the_refusals_come_in_the_documented_order(sfx):
    """Every call is refused on the host: the (fake) pointers are never dereferenced and nothing is launched, so this runs without
    a GPU.  The list starts with EVERY argument wrong and mends the one just reported: the order of the messages is the order of
    the checks — the base arguments, a negative mask, a mask bit at or above n_gas, a NULL cumE with a non-zero mask, the
    refusals of fiveeq_run_inverse_forc_* in its order, and last FIVEEQ_E_UNSUPPORTED for a proper mask on a layout without
    the form."""
    lib = _capi.load()
    wrong = dict(n=0, mask=-2, cumE=0, n_fext=5, fscale=0, fext=0, n_gas=2, obs=0, misfit=0x5004)
    steps = [
        ("n_members", dict(n=8)),                                    # the base arguments (make_args)
        ("conc_mask=-2 must be >= 0", dict(mask=0b100)),
        ("conc_mask=0x4 has bits at or above n_gas=2", dict(mask=0b01)),
        ("cumE is NULL", dict(cumE=0x1800)),
        ("n_fext=5 outside 0..4", dict(n_fext=2)),                   # check_forcing, in its own order
        ("fscale is NULL", dict(fscale=0x2001)),
        ("fscale must be", dict(fscale=0x2000)),
        ("fext is NULL with n_fext=2", dict(fext=0x3001)),
        ("fext must be", dict(fext=0x3000)),
        ("has no forcing form", dict(fscale=0, n_fext=0)),           # (the 4 + 1 layout stays: the misfit has no form for it either)
        ("obs and misfit go together", dict(obs=0x4000)),
        ("8-byte aligned", dict(misfit=0x5000)),
        ("has no misfit form", dict(obs=0, misfit=0)),
    ]
    for needle, mend in steps:
        rc, msg = _call(lib, sfx, t0=1, t1=1, **wrong)
        assert rc == _capi.E_INVALID and needle in msg, (needle, rc, msg)
        wrong.update(mend)
    rc, msg = _call(lib, sfx, t0=1, t1=1, **wrong)                   # a proper mask of pools 4 + 1: the last refusal, its own code
    assert rc == _capi.E_UNSUPPORTED and "no mixed-drive form" in msg, (rc, msg)
    # ... and E_UNSUPPORTED comes AFTER the inverse-forc refusals: the same layout with a bad misfit pair is E_INVALID
    rc, msg = _call(lib, sfx, t0=1, t1=1, **dict(wrong, obs=0x4000))
    assert rc == _capi.E_INVALID and "obs and misfit go together" in msg, (rc, msg)
    for mask in range(1, 7):                                          # every proper mask of 4 + 4 + 4 and of 4 + 1
        rc, msg = _call(lib, sfx, kind="444", t0=1, t1=1, mask=mask, fscale=0, fext=0, n_fext=0, obs=0, misfit=0)
        assert rc == _capi.E_UNSUPPORTED and "no mixed-drive form" in msg, (mask, rc, msg)
    for mask in (1, 2):
        rc, msg = _call(lib, sfx, n_gas=2, t0=1, t1=1, mask=mask, fscale=0, fext=0, n_fext=0, obs=0, misfit=0)
        assert rc == _capi.E_UNSUPPORTED, (mask, rc, msg)
    # accepted with an EMPTY step range (nothing to launch): every mask of 4 + 1 + 1 in every carrier; the degenerate masks of
    # the other layouts; mask 0 with a NULL cumE
    for mask in range(8):
        for kw in (dict(), dict(fscale=0, fext=0, n_fext=0), dict(obs=0, misfit=0), dict(fscale=0, fext=0, n_fext=0, obs=0, misfit=0)):
            rc, msg = _call(lib, sfx, t0=1, t1=1, mask=mask, **kw)
            assert rc == _capi.OK, (mask, kw, msg)
    plain = dict(fscale=0, fext=0, n_fext=0, obs=0, misfit=0, t0=1, t1=1)
    assert _call(lib, sfx, mask=0, cumE=0, **plain)[0] == _capi.OK
    assert _call(lib, sfx, kind="444", mask=0, cumE=0, **plain)[0] == _capi.OK and _call(lib, sfx, kind="444", mask=7, **plain)[0] == _capi.OK
    assert _call(lib, sfx, n_gas=2, mask=3, **plain)[0] == _capi.OK
    rc, msg = _call(lib, sfx, mask=0b111, cumE=0, **plain)
    assert rc == _capi.E_INVALID and "cumE is NULL" in msg
    rc, msg = _call(lib, sfx, mask=8, **plain)
    assert rc == _capi.E_INVALID and "bits at or above n_gas=3" in msg
    # the base arguments as fiveeq_run_inverse_* reports them, whatever the rest
    for kw, needle in ((dict(ld=4), "ld="), (dict(ptr=0), "NULL device pointer"), (dict(t0=3, t1=2), "step range"),
                       (dict(t1=5), "step range")):
        rc, msg = _call(lib, sfx, **dict(dict(cumE=0, n_fext=9, mask=-1), **kw))
        assert rc == _capi.E_INVALID and needle in msg, (kw, msg)


# ---- the references ----------------------------------------------------------------------------------------------------------------
def test_the_emission_series_meets_its_conditions():
    """fp32-exact amplitudes and series; zero at step 0; negative emissions; the cumulative sums before each step exact in fp32
    for dt = 1 and dt = 0.5; the 130-step series starts with the 12-step one."""
    f32_exact = lambda x: np.array_equal(x, np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64))   # noqa: E731
    assert f32_exact(mx.EMIS_AMPLITUDE)
    for name in mx.CASES:
        c, long = mx.case(name), mx.case(name, 130)
        assert c["pools"] == [4, 1, 1] and c["E"].shape == (12, 3)
        assert f32_exact(c["E"]) and f32_exact(long["E"]) and f32_exact(long["cum_shared"])
        assert np.all(c["E"][0] == 0) and c["E"].min() < 0 < c["E"].max()
        assert np.array_equal(long["E"][:12], c["E"]) and np.array_equal(long["cum_shared"][:12], c["cum_shared"])
        assert np.array_equal(long["target"][:12], c["target"]) and np.array_equal(c["target"], ir.case(name)["target"])
        exact = np.concatenate([[np.zeros(3)], np.cumsum(long["E"] * c["dt"], axis=0)[:-1]])
        assert np.array_equal(long["cum_shared"], exact)


@pytest.mark.parametrize("mask", mx.MASKS)
@pytest.mark.parametrize("name", mx.CASES)
def test_the_twin_agrees_with_the_50_digit_step_at_every_step(name, mask):
    """The NumPy twin, one step at a time from its own state, against the 50-digit mixed step from that state; worst units of
    eps64 x scale over 12 steps x 16 members (K_MIXED must cover them and not exceed them by more than a unit).  On the way
    every member stays finite with C > 0 in every gas and an un-clamped iIRF at every step, and the excursion of C of an
    emission-driven gas is of the size of the targets' (between a fifth of it and five times it): the condition the GPU test's
    inputs must meet, asserted here so that the reference alone is known to meet it.  Measured 2026-10-20 (X T R S cum):

        mask     4+1+1                               multigas dt=0.5
        0b001    0.452 0.427 1.860 0.503 0.014       0.471 0.427 1.378 0.441 0.008
        0b010    0.448 0.569 1.503 0.567 0.130       0.471 0.600 1.224 0.615 0.059
        0b011    0.445 0.424 1.309 0.452 0.102       0.471 0.433 1.463 0.430 0.055
        0b100    0.447 0.574 1.627 0.545 0.008       0.450 0.620 1.334 0.604 0.008
        0b101    0.371 0.368 1.373 0.390 0.019       0.343 0.367 1.046 0.387 0.011
        0b110    0.454 0.527 1.313 0.533 0.119       0.438 0.512 1.439 0.538 0.081
    """
    c = mx.case(name)
    worst, steps = mx.restated_anchored(name, mask)
    print(f"K_MIXED[{name!r}][{mask:#05b}] =", {k: round(v, 3) for k, v in worst.items()})
    iirf_max = float(c["params"]["iirf_max"])
    excursion = np.zeros(3)
    for got, ref in steps:
        assert all(np.isfinite(got[k]).all() for k in mx.OUTPUTS), (name, mask)
        assert np.all(ref["C"][0] > 0) and np.all(ref["iirf"] < iirf_max), (name, mask)
        excursion = np.maximum(excursion, np.abs(ref["C"][0] - c["target"][0][:, None]).max(axis=1))
    want = np.abs(c["target"] - c["target"][0]).max(axis=0)
    for g in range(3):
        assert 0.2 * want[g] <= excursion[g] <= 5.0 * want[g], (name, mask, g, excursion[g], want[g])
    for out, v in worst.items():
        assert v <= 4.0, (name, mask, out, v)       # two fp64 programs of ~10 roundings per output: a few units, or one is wrong
        assert v <= K_MIXED[name][mask][out] <= v + 1.0, (name, mask, out, v, K_MIXED[name][mask][out])


@pytest.mark.parametrize("name", mx.CASES)
def test_cum_of_an_emission_driven_gas_is_left_alone(name):
    """The twin and the 50-digit step return the cum row of an emission-driven gas as they got it — from a state where it is
    not zero, too — and the yardstick holds that row to exact equality (scale 0)."""
    c = mx.case(name)
    rng = np.random.default_rng(3)
    R, S, cum = rng.uniform(1.0, 30.0, (6, mx.M)), rng.uniform(0.1, 0.9, (2, mx.M)), rng.uniform(-5.0, 40.0, (3, mx.M))
    for mask in mx.MASKS:
        got, ref = mx.restated_step(c, mask, R, S, cum, 5), mx.step_reference(c, mask, R, S, cum, 5)
        for g in range(3):
            if not mask >> g & 1:
                assert np.array_equal(got["cum"][g], cum[g]) and np.array_equal(ref["cum"][0][g], cum[g]) and np.all(ref["scum"][g] == 0)
            else:
                assert np.all(got["cum"][g] != cum[g]) and np.all(ref["scum"][g] > 0)
        nudged = got["cum"] * np.where(np.arange(3)[:, None] == 0, 1.0 + sr.EPS["f64"], 1.0)      # one ulp off in gas 0's row
        u = mx.units(dict(got, cum=nudged), ref, sr.EPS["f64"])
        assert np.all(np.isinf(u["cum"][0])) == (not mask & 1) and np.all(np.isfinite(u["cum"][1:])), mask


VARIANT_OUTPUT = dict(zip(mx.VARIANTS, ("X", "cum", "X")))


# the first mistake needs a concentration-driven gas whose alpha knows cum: CO2 (rC of CH4 is zero, of N2O zero or a thousandth)
MISTAKES = [(mask, v) for v in mx.VARIANTS for mask in mx.MASKS if v != mx.VARIANTS[0] or mask & 1]


@pytest.mark.parametrize("mask,variant", MISTAKES)
@pytest.mark.parametrize("name", mx.CASES)
def test_the_yardstick_sees_each_mistake(name, mask, variant):
    """alpha of a concentration-driven gas taken from the shared drive column (seen in X, the diagnosed E — on the masks where
    CO2 is concentration-driven: rC of CH4 and N2O is zero or a thousandth, and their alpha hardly knows cum); cum advanced for
    an emission-driven gas (seen in cum: any change of that row is infinitely many units); the emission rate of an
    emission-driven gas read from column 3 + g (seen in X, its C).  Each misses BOUND max(K_MIXED, 1) in the output it corrupts
    in units of eps64 by more than a thousand times, and still misses it in units of eps32, the GPU tests' coarser yardstick."""
    c, out = mx.case(name), VARIANT_OUTPUT[variant]
    for prec in ("f64", "f32"):
        worst, _ = mx.anchored(c, mask, lambda *a: mx.restated_step(*a, variant=variant), eps=sr.EPS[prec])
        ratio = {o: worst[o] / (BOUND * max(K_MIXED[name][mask][o], 1.0)) for o in mx.OUTPUTS}
        print(f"{name}, {mask:#05b}, {variant}, {prec}: worst / bound", {o: float(f"{v:.3g}") for o, v in ratio.items()})
        assert ratio[out] > (1e3 if prec == "f64" else 1.0), (name, mask, variant, prec, ratio)


@pytest.mark.parametrize("name", mx.CASES)
def test_the_degenerate_masks_are_the_forward_and_the_inverse_step(name):
    """Mask 0: the twin's 12 steps are the oracle's forward run on the emission series bit for bit (C, T, R, S; cum untouched).
    Mask 0b111: each step is inverse_reference.restated_step bit for bit, from a zero state and from a drawn one, and the
    50-digit step is inverse_reference.step_reference."""
    c = mx.case(name)
    want = npo.run(c["E"], c["params"], mx.M, F_ext=c["F_ext"], dt=c["dt"])
    R, S, cum = np.zeros((6, mx.M)), np.zeros((2, mx.M)), np.zeros((3, mx.M))
    for t in range(mx.N_STEPS):
        got = mx.restated_step(c, 0, R, S, cum, t)
        assert np.array_equal(got["X"], want["C"][t]) and np.array_equal(got["T"], want["T"][t]), (name, t)
        assert not got["cum"].any()
        R, S = got["R"], got["S"]
    assert np.array_equal(R, np.concatenate(want["R"])) and np.array_equal(S, want["S"])
    rng = np.random.default_rng(5)
    states = [(np.zeros((6, mx.M)), np.zeros((2, mx.M)), np.zeros((3, mx.M))),
              (rng.uniform(1.0, 30.0, (6, mx.M)), rng.uniform(0.1, 0.9, (2, mx.M)), rng.uniform(-5.0, 40.0, (3, mx.M)))]
    for t, state in ((0, states[0]), (5, states[1])):
        got, inv = mx.restated_step(c, 0b111, *state, t), ir.restated_step(ir.case(name), *state, t)
        for k in mx.OUTPUTS:
            assert np.array_equal(got[k], inv["E" if k == "X" else k]), (name, t, k)
        a, b = mx.step_reference(c, 0b111, *state, t), ir.step_reference(ir.case(name), *state, t)
        for k in b:
            ka = {"E": "X", "sE": "sX"}.get(k, k)
            same = (all(np.array_equal(x, y) for x, y in zip(a[ka], b[k])) if isinstance(b[k], tuple) else np.array_equal(a[ka], b[k]))
            assert same, (name, t, k)


# ---- host plumbing -----------------------------------------------------------------------------------------------------------------
def test_make_drive_per_gas_form():
    E = np.arange(15, dtype=np.float64).reshape(5, 3) + 1.0
    C = 300.0 + np.arange(15, dtype=np.float64).reshape(5, 3)
    fwd, inv = emissions.make_drive(E, dt=0.5), emissions.make_drive(C, dt=0.5, concentration_driven=True)
    for mask in range(8):
        gases = mx.concentration_gases(mask)
        En, Cn = E.copy(), C.copy()
        En[:, list(gases)] = np.nan                                  # the ignored columns may hold anything
        Cn[:, [g for g in range(3) if g not in gases]] = np.nan
        d = emissions.make_drive(En, np.ones(5), 0.5, [1, 3], concentrations=Cn, concentration_gases=gases)
        assert d.shape == (5, 8) and np.isfinite(d).all()
        for g in range(3):
            src = inv if g in gases else fwd
            assert np.array_equal(d[:, g], src[:, g]) and np.array_equal(d[:, 3 + g], src[:, 3 + g]), (mask, g)
            if g in gases:
                assert not d[:, 3 + g].any()
            else:
                assert np.array_equal(d[1:, 3 + g], np.cumsum(E[:, g] * 0.5)[:-1]) and d[0, 3 + g] == 0
        assert np.all(d[:, 6] == 1.0) and d[:, 7].tolist() == [-1, 0, -1, 1, -1]
    assert np.array_equal(emissions.make_drive(E, dt=0.5, concentrations=None, concentration_gases=()), fwd)
    assert np.array_equal(emissions.make_drive(None, dt=0.5, concentrations=C, concentration_gases=(0, 1, 2)), inv)
    assert np.array_equal(emissions.make_drive(E, dt=0.5), fwd)      # the forms that existed are what they were
    for bad, needle in ((dict(concentration_gases=(3,)), "gas indices in 0..2"), (dict(concentration_gases=(1, 1)), "named twice"),
                        (dict(concentration_gases=(-1,)), "gas indices"), (dict(concentration_gases=(0.5,)), "gas indices"),
                        (dict(concentration_gases="x"), "gas indices"), (dict(concentration_gases=(1,), concentrations=C[:4]), "one shape"),
                        (dict(concentration_gases=(1,), concentrations=None), "concentrations is None"),
                        (dict(concentration_gases=(1,), concentration_driven=True), "per-gas form")):
        kw = dict(dict(concentrations=C), **bad)
        with pytest.raises(ValueError, match=needle):
            emissions.make_drive(E, **kw)
    with pytest.raises(ValueError, match="non-finite"):               # NaN in a column that IS used
        emissions.make_drive(np.where(np.arange(3) == 0, np.nan, E), concentrations=C, concentration_gases=(1, 2))
    with pytest.raises(ValueError, match="needs concentration_gases"):
        emissions.make_drive(E, concentrations=C)
    assert emissions.concentration_mask((2, 1), 3) == 0b110 and emissions.concentration_mask([], 3) == 0
    assert emissions.concentration_mask(np.array([0, 2]), 3) == 0b101


def test_the_engine_refuses_bad_arguments_before_it_asks_for_a_device():
    from fiveeqscm_amd.engine import ConcentrationDrivenEngine, MixedDriveEngine
    import fiveeqscm_amd
    assert fiveeqscm_amd.MixedDriveEngine is MixedDriveEngine and issubclass(MixedDriveEngine, ConcentrationDrivenEngine)
    p = prm.default_params("multigas")
    E, C = np.ones((6, 3)), np.full((6, 3), 300.0)
    for args, needle in (((E, C, (3,)), "gas indices in 0..2"), ((E, C, (0, 0)), "named twice"), ((E, C[:5], (0,)), "one shape"),
                         ((np.stack([E, E]), C, (0,)), "one scenario"), ((E, [C, C], (0,)), "one scenario"),
                         ((E * np.nan, C, (1, 2)), "non-finite"), ((E, C * np.nan, (1, 2)), "non-finite")):
        with pytest.raises(ValueError, match=needle):
            MixedDriveEngine(p, 4, *args)
    with pytest.raises(ValueError, match="F_ext has 5 steps"):
        MixedDriveEngine(p, 4, E, C, (1, 2), F_ext=np.zeros(5))
    with pytest.raises(TypeError, match="always concentration-driven"):
        MixedDriveEngine(p, 4, E, C, (1, 2), concentration_driven=True)


class _Stub(CheckpointMixin):
    """The attributes load_state_dict() reads before it validates the mask."""
    cumE = misfit = observations = forcing = R = S = None
    scenario_axis = collect_stats = False

    def __init__(self, mask):
        if mask is not None:
            self.conc_mask = mask


def test_a_checkpoint_of_another_mask_is_refused_by_name():
    for mine, theirs in ((0b110, 0b001), (0b110, 0b111), (0b110, None), (None, 0b110), (0, None)):
        state = {} if theirs is None else {"conc_mask": theirs}
        with pytest.raises(ValueError, match="conc_mask"):
            _Stub(mine).load_state_dict(state)
    for mask in (0b110, 0, None):                                     # the same mask passes the check and goes on to the state
        with pytest.raises(KeyError, match="'R'"):
            _Stub(mask).load_state_dict({} if mask is None else {"conc_mask": mask})
