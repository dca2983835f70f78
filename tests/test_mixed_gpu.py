"""The mixed drive on the device: fused_mixed_kernel<T, 4, 1, 1, CM, MISFIT, FORC> behind fiveeq_run_mixed_* and MixedDriveEngine
— some gases concentration-driven, the others emission-driven — in fp64 and fp32, on the cases of tests/mixed_reference.py.

ANCHORED ACCURACY (all six masks): one step per launch, the device state read back before each step, the 50-digit mixed step
evaluated from exactly that state; X (C of an emission-driven gas, E of a concentration-driven one), T, R, S and cum are held to
|got - ref| <= 8 max(K_MIXED, 1) eps(dtype) scale, in fp64 never past the project's tolerances (the rule of
tests/test_inverse_gpu.py); the cum row of an emission-driven gas stays exactly zero.
ONE ARITHMETIC (masks 0b110 and 0b001): every way of cutting a run gives the same bits.  THE DEGENERATE MASKS are the forward and
the inverse call bit for bit on the same drive table.

N = 323 = 256 + 64 + 3 members: two workgroups, the second with one full wave, one wave of 3 members and two idle waves.
"""
import ctypes
import functools

import numpy as np
import pytest

import inverse_forcing_reference as fr
import mixed_reference as mx
import step_reference as sr
from test_mixed_cpu import K_MIXED

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_step_edges_gpu import BOUND, PROJECT_TOL, _same_bits      # noqa: E402  (the bound's factor and the project's tolerances)

from fiveeqscm_amd import constrain                                 # noqa: E402
from fiveeqscm_amd.forcing import ExternalForcings                  # noqa: E402

N = 323
N_STEPS = mx.N_STEPS
DTYPE = {"f64": torch.float64, "f32": torch.float32}
PRECS = ("f64", "f32")
STATE = ("X", "T", "R", "S", "cum")
FLAGSHIP = "multigas dt=0.5"
ARITH_MASKS = (0b110, 0b001)


def _project_limit(mask, prec, out, ref, eps, shape):
    """The project's tolerance of an output in units of eps x scale ([rows, M]; inf where it sets none): each row of X takes
    the tolerance of what it holds, C or E."""
    kinds = [("E" if mask >> g & 1 else "C") for g in range(3)] if out == "X" else [out] * shape[0]
    limit = np.full(shape, np.inf)
    scale = sr.scale_of(ref, out, eps)
    for row, kind in enumerate(kinds):
        if (prec, kind) in PROJECT_TOL:
            rtol, atol = PROJECT_TOL[(prec, kind)]
            with np.errstate(divide="ignore"):
                limit[row] = np.where(scale[row] > 0, (rtol * np.abs(ref[out][0][row]) + atol) / (eps * scale[row]), np.inf)
    return limit


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from fiveeqscm_amd import _capi
    return _capi.load()                       # the HIP library must be the thing that runs: no fallback


@functools.lru_cache(maxsize=None)
def _obs(n_steps):
    t = np.arange(n_steps)
    at = t[(t >= 3) & (t % 5 != 0)]
    return constrain.Observations.from_years(t.astype(float), at.astype(float), 0.02 + 0.003 * at, 0.05, (1.0, 4.0))


def _engine(mask, n, prec, n_steps=N_STEPS, name=FLAGSHIP, scales=None, obs=False, **kw):
    """scales: None, or (f_scale [G, n] or [G], fx_scale or None, table [n_steps, K])."""
    from fiveeqscm_amd import MixedDriveEngine
    c = mx.case(name, n_steps)
    p = mx.tiled_params(c, n)
    fx = None
    if scales is not None:
        p = dict(p, f_scale=scales[0], **({} if scales[1] is None else {"fx_scale": scales[1]}))
        fx = ExternalForcings(scales[2])
    return MixedDriveEngine(p, n, c["E"], c["target"], mx.concentration_gases(mask), F_ext=c["F_ext"], dt=c["dt"],
                            dtype=DTYPE[prec], device="cuda:0", forcing=fx, observations=_obs(n_steps) if obs else None, **kw)


def _state(eng):
    torch.cuda.synchronize()
    out = {"X": eng.X.cpu().numpy(), "T": eng.T.cpu().numpy(), "R": eng.R.cpu().numpy(), "S": eng.S.cpu().numpy(),
           "cum": eng.cumE.cpu().numpy()}
    if eng.misfit is not None:
        out["misfit"] = eng.misfit.cpu().numpy()
    if eng.T_stats is not None:
        out["records"] = eng.T_stats.cpu().numpy()
    return out


def _run(mask, n, prec, cuts=(0, N_STEPS), n_steps=N_STEPS, **kw):
    eng = _engine(mask, n, prec, n_steps, **kw)
    for a, b in zip(cuts, cuts[1:]):
        eng.run(a, b)
    out = _state(eng)
    eng.close()
    return out


@functools.lru_cache(maxsize=None)
def _one_launch(mask, prec, collect_stats=False):
    """run(0, 12) of the N-member ensemble in one launch: computed once, shared, read-only."""
    out = _run(mask, N, prec, collect_stats=collect_stats)
    assert all(np.isfinite(out[k]).all() for k in STATE), (mask, prec)
    return out


def _assert_same(got, want, what, members=slice(None), names=STATE):
    for k in names:
        assert _same_bits(got[k][..., members], want[k][..., members]), (*what, k)


def _anchored(mask, prec, name, K, scales=None, ref_scales=None):
    """The anchored comparison of one engine: (worst units per output, failures)."""
    c = mx.case(name)
    eps, replica = sr.EPS[prec], np.arange(N) % mx.M
    emission_rows = [g for g in range(3) if not mask >> g & 1]
    eng = _engine(mask, N, prec, name=name, scales=scales)
    assert eng.conc_mask == mask and eng.out_kind == tuple("E" if mask >> g & 1 else "C" for g in range(3))
    worst, failures = dict.fromkeys(mx.OUTPUTS, 0.0), []
    before = _state(eng)
    for t in range(N_STEPS):
        eng.run(t, t + 1)
        after = _state(eng)
        got = {"X": after["X"][t], "T": after["T"][t][None, :], "R": after["R"], "S": after["S"], "cum": after["cum"]}
        for out, x in got.items():
            assert np.isfinite(x).all(), (mask, prec, t, out)
            assert _same_bits(x, x[:, replica]), (mask, prec, t, out, "a member differs from its replica")
        assert not got["cum"][emission_rows].any(), (mask, prec, t, "the cum row of an emission-driven gas was written")
        ref = mx.step_reference(c, mask, *(before[k][:, :mx.M].astype(np.float64) for k in ("R", "S", "cum")), t, scales=ref_scales)
        for out, u in mx.units({k: x[:, :mx.M].astype(np.float64) for k, x in got.items()}, ref, eps).items():
            # ... and never past the project's tolerance
            limit = np.minimum(np.full_like(u, BOUND * max(K[out], 1.0)), _project_limit(mask, prec, out, ref, eps, u.shape))
            worst[out] = max(worst[out], float(u.max()))
            if np.any(u > limit):
                row, m = np.unravel_index(np.argmax(u / limit), u.shape)
                failures.append((t, out, int(row), int(m), float(u[row, m]), float(limit[row, m])))
        before = after
    eng.close()
    return worst, failures


# ---- anchored accuracy --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mask", mx.MASKS)
def test_every_step_against_the_50_digit_step_from_the_device_state(lib, mask, prec):
    """Worst multiples of eps(dtype) x scale over the 12 steps x 16 members of "multigas dt=0.5" (bound: 8 max(K_MIXED, 1), that
    is 8 except R: 10 to 12), measured on the MI355X, 2026-10-20 (the test prints every figure):

        mask    fp64:  X      T      R      S     cum     fp32:  X      T      R      S     cum
        0b001         0.471  0.507  0.759  0.519  0.011         0.471  0.280  1.092  0.290  0.007
        0b010         0.471  0.802  1.003  0.808  0.085         0.471  0.582  0.698  0.579  0.073
        0b011         0.471  0.497  2.095  0.506  0.064         0.471  0.291  0.735  0.260  0.098
        0b100         0.442  0.782  1.287  0.757  0.008         0.448  0.567  1.206  0.546  0.005
        0b101         0.354  0.387  0.769  0.385  0.014         0.354  0.249  1.150  0.258  0.008
        0b110         0.435  0.753  1.163  0.737  0.087         0.448  0.494  0.868  0.513  0.056

    Members 16 .. 322 carry their replica's bits in every output at every step, and the cum rows of the emission-driven gases
    are exactly zero at every step."""
    worst, failures = _anchored(mask, prec, FLAGSHIP, K_MIXED[FLAGSHIP][mask])
    print(f"mask {mask:#05b} {prec}: worst x eps x scale " + " ".join(f"{out} {v:.3f}" for out, v in worst.items()))
    assert not failures, (mask, prec, failures)


# ---- one arithmetic -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mask", ARITH_MASKS)
def test_one_launch_equals_the_chain_of_single_step_launches(lib, mask, prec):
    """run(0, 12) == 12 launches of one step == run(0, 5); run(5, 12), in X, T, R, S and cum."""
    want = _one_launch(mask, prec)
    _assert_same(_run(mask, N, prec, cuts=range(N_STEPS + 1)), want, (mask, prec, "12 single steps"))
    _assert_same(_run(mask, N, prec, cuts=(0, 5, N_STEPS)), want, (mask, prec, "5 + 7"))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mask", ARITH_MASKS)
def test_a_launch_across_the_drive_refill_equals_launches_that_end_at_it(lib, mask, prec):
    """130 steps in one launch (the LDS drive chunk refilled at step 125) against (0, 125, 130) and (0, 124, 130)."""
    want = _run(mask, N, prec, cuts=(0, 130), n_steps=130)
    assert all(np.isfinite(want[k]).all() for k in STATE), (mask, prec)
    for cuts in ((0, 125, 130), (0, 124, 130)):
        _assert_same(_run(mask, N, prec, cuts=cuts, n_steps=130), want, (mask, prec, cuts))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mask", ARITH_MASKS)
def test_stored_steps_are_the_rows_of_the_full_run(lib, mask, prec):
    want = _one_launch(mask, prec)
    steps = [0, 4, 5, 11]
    got = _run(mask, N, prec, output_steps=steps)
    assert got["X"].shape[0] == got["T"].shape[0] == len(steps)
    _assert_same(got, {**want, "X": want["X"][steps], "T": want["T"][steps]}, (mask, prec, "output_steps"))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mask", ARITH_MASKS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_every_ensemble_size_gives_the_members_of_the_323_member_run(lib, n, mask, prec):
    got = _run(mask, n, prec)
    _assert_same(got, {k: v[..., :n] for k, v in _one_launch(mask, prec).items()}, (n, mask, prec))


# ---- a sub-range of a longer allocation, through the C ABI -------------------------------------------------------------------------
SENTINEL = -12345.0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mask", ARITH_MASKS)
@pytest.mark.parametrize("ld", [330, 331])
def test_a_member_sub_range_of_a_longer_allocation(lib, ld, mask, prec):
    """fiveeq_run_mixed_* on members [3, 260) of rows of length ld, every row pointer offset by 3 members: the range gets the
    bits of a stand-alone 257-member run and every word outside it keeps its sentinel.  THE WHOLE cumE ROW OF EACH
    EMISSION-DRIVEN GAS KEEPS ITS SENTINEL, inside the range too: the kernel neither reads nor writes it (the state rows of the
    range are zeroed, that row is not — a kernel that read it would compute from the sentinel and miss the stand-alone bits)."""
    n, m0 = 257, 3
    alone = _engine(mask, n, prec)
    alone.run(0, N_STEPS)
    want = _state(alone)
    G, SP, dtype = alone.n_gas, alone.sum_pools, DTYPE[prec]
    rows = {"r": 3 * G, "q": 2, "R": SP, "S": 2, "cum": G, "X": alone.n_rows * G, "T": alone.n_rows}
    buf = {k: torch.full((k_rows, ld), SENTINEL, dtype=dtype, device="cuda:0") for k, k_rows in rows.items()}
    buf["r"][:, m0:m0 + n], buf["q"][:, m0:m0 + n] = alone.r, alone.q
    conc = list(mx.concentration_gases(mask))
    emis = [g for g in range(G) if g not in conc]
    for k in ("R", "S"):
        buf[k][:, m0:m0 + n] = 0.0
    buf["cum"][conc, m0:m0 + n] = 0.0
    at = lambda t: ctypes.c_void_p(t.data_ptr() + m0 * t.element_size())          # noqa: E731
    with torch.cuda.device(alone.device):
        rc = getattr(lib, f"fiveeq_run_mixed_{prec}")(
            ctypes.byref(alone.model), n, ld, ctypes.c_void_p(alone.drive.data_ptr()), alone.n_steps, 0, N_STEPS, at(buf["r"]),
            at(buf["q"]), at(buf["R"]), at(buf["S"]), at(buf["cum"]), at(buf["X"]), at(buf["T"]), alone.n_rows, None, mask,
            None, None, 0, None, None, alone._stream())
    assert rc == 0, lib.fiveeq_last_error()
    torch.cuda.synchronize()
    outside = np.ones(ld, dtype=bool)
    outside[m0:m0 + n] = False
    for k in STATE:
        x = buf[k].cpu().numpy()
        assert np.all(x[:, outside] == SENTINEL), (ld, mask, prec, k, "a word outside the range was written")
        if k == "cum":
            assert np.all(x[emis] == SENTINEL), (ld, mask, prec, "the cumE row of an emission-driven gas was written")
            assert _same_bits(x[conc][:, m0:m0 + n], want[k][conc]), (ld, mask, prec, k)
        else:
            assert _same_bits(x[:, m0:m0 + n].reshape(want[k].shape), want[k]), (ld, mask, prec, k)
    assert not want["cum"][emis].any()
    alone.close()


# ---- the degenerate masks ------------------------------------------------------------------------------------------------------------
def _c_call(lib, eng, fn, t_end, *tail, cumE=True):
    eng.reset_state()
    eng._wave_stats()
    with torch.cuda.device(eng.device):
        rc = eng._fn(fn)(*eng._run_args(0, t_end, cumE=eng._ptr(eng.cumE) if cumE else ctypes.c_void_p(0)), *tail, eng._stream())
    assert rc == 0, lib.fiveeq_last_error()
    return _state(eng)


@pytest.mark.parametrize("carrier", ["plain", "forc", "misfit", "forc+misfit"])
@pytest.mark.parametrize("prec", PRECS)
def test_the_degenerate_masks_are_the_forward_and_the_inverse_call(lib, prec, carrier):
    """On ONE drive table (that of mask 0, and that of mask 0b111, as make_drive builds them): fiveeq_run_mixed_* with mask 0
    equals fiveeq_run_fused_* (plain), fiveeq_run_forc_* with FIVEEQ_FORM_FUSED, k_steps = 0 (with scales) and fiveeq_run_obs_*
    likewise (the misfit alone); with mask 0b111 it equals fiveeq_run_inverse_forc_* — bit for bit in the rows, the state, cumE
    (untouched under mask 0), the misfit and the wave records.  130 steps: the drive chunk is refilled."""
    from fiveeqscm_amd import _capi
    n_steps = 130
    c = fr.case(FLAGSHIP, n_steps)
    forc, obs = "forc" in carrier, "misfit" in carrier
    scales = (fr.tiled_params(c, N)["f_scale"], fr.tiled_params(c, N)["fx_scale"], c["X"]) if forc else None
    names = STATE + ("records",) + (("misfit",) if obs else ())
    for mask in (0, 0b111):
        eng = _engine(mask, N, prec, n_steps, scales=scales, obs=obs, collect_stats=True)
        assert eng.conc_mask == mask
        eng.run()
        got = _state(eng)
        assert all(np.isfinite(got[k]).all() for k in names)
        f_args = (eng._ptr(eng.fscale), eng._ptr(eng.fext), 3) if forc else (None, None, 0)
        o_args = eng._obs_args() if obs else (None, None)
        if mask:
            want = _c_call(lib, eng, "run_inverse_forc", n_steps, *f_args, *o_args)
            assert got["cum"].all()
        else:
            args = eng._run_args(0, n_steps)
            eng.reset_state()
            with torch.cuda.device(eng.device):
                if forc:
                    rc = eng._fn("run_forc")(*args, *f_args, *o_args, _capi.FORM_FUSED, 0, eng._stream())
                elif obs:
                    rc = eng._fn("run_obs")(*args, *o_args, _capi.FORM_FUSED, 0, eng._stream())
                else:
                    rc = eng._fn("run_fused")(*args, eng._stream())
            assert rc == 0, lib.fiveeq_last_error()
            want = _state(eng)
            assert not got["cum"].any()
            # ... and mask 0 takes a NULL cumE
            again = _c_call(lib, eng, "run_mixed", n_steps, 0, *f_args, *o_args, cumE=False)
            _assert_same(again, want, (prec, carrier, "NULL cumE"), names=names)
        _assert_same(got, want, (prec, carrier, mask), names=names)
        eng.close()


# ---- the carriers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_unit_scales_are_the_plain_mixed_run_bit_for_bit(lib, prec):
    """Mask 0b110.  Unit gas scales with n_fext = 0, and the case's category scales on an all-zero table with unit gas scales:
    the bits of the plain mixed run, wave records included."""
    n_steps, mask = 130, 0b110
    want = _run(mask, N, prec, cuts=(0, n_steps), n_steps=n_steps, collect_stats=True)
    sx = fr.tiled_params(fr.case(FLAGSHIP, n_steps), N)["fx_scale"]
    for what, scales in (("K = 0", (np.ones(3), None, np.zeros((n_steps, 0)))), ("zero table", (np.ones(3), sx, np.zeros((n_steps, 3))))):
        got = _run(mask, N, prec, cuts=(0, n_steps), n_steps=n_steps, scales=scales, collect_stats=True)
        _assert_same(got, want, (prec, what), names=STATE + ("records",))


@pytest.mark.parametrize("prec", PRECS)
def test_scaled_steps_against_the_50_digit_step(lib, prec):
    """Mask 0b110 with the scale rows and the table of inverse_forcing_reference (none of them 1, three categories): every step
    against the 50-digit step of each member's own model, the thermal scales widened by the cancellation among the external
    terms as inverse_forcing_reference._widen_thermal_scales has it.  Bound: 8 max(K, 1) with, per output, the larger of K_MIXED
    and the K of tests/test_inverse_forcing_cpu.py for this case (the twin with scales was measured there, not here).  Measured
    on the MI355X, 2026-10-20 (X T R S cum): fp64 0.450 0.624 0.952 0.597 0.062; fp32 0.451 0.508 0.826 0.515 0.080."""
    from test_inverse_forcing_cpu import K as K_FORC
    c = fr.case(FLAGSHIP)
    p = fr.tiled_params(c, N)
    K = {o: max(K_MIXED[FLAGSHIP][0b110][o], K_FORC[FLAGSHIP]["E" if o == "X" else o]) for o in mx.OUTPUTS}
    worst, failures = _anchored(0b110, prec, FLAGSHIP, K, scales=(p["f_scale"], p["fx_scale"], c["X"]),
                                ref_scales=(c["sg"], c["sx"], c["X"]))
    print(f"scaled, mask 0b110 {prec}: worst x eps x scale " + " ".join(f"{out} {v:.3f}" for out, v in worst.items()))
    assert not failures, (prec, failures)


@pytest.mark.parametrize("forc", [False, True], ids=["misfit", "forc+misfit"])
@pytest.mark.parametrize("prec", PRECS)
def test_observations_change_nothing_and_the_misfit_is_that_of_the_stored_T(lib, prec, forc):
    """Mask 0b110: observations= changes none of X, T, R, S, cum; misfit == score_rows of the stored T rows (eng.score) ==
    constrain.misfit_numpy, bit for bit; chi2() is chi2_from_misfit of it."""
    mask, obs = 0b110, _obs(N_STEPS)
    c = fr.case(FLAGSHIP)
    scales = (fr.tiled_params(c, N)["f_scale"], fr.tiled_params(c, N)["fx_scale"], c["X"]) if forc else None
    without = _run(mask, N, prec, scales=scales)
    eng = _engine(mask, N, prec, scales=scales, obs=True)
    eng.run()
    got = _state(eng)
    _assert_same(got, without, (prec, forc, "observations= changed the run"))
    want = constrain.misfit_numpy(got["T"], obs.table)
    assert got["misfit"].any() and _same_bits(got["misfit"], want), (prec, forc)
    assert _same_bits(eng.score({"T": obs}).misfit["T"].cpu().numpy(), want)
    assert _same_bits(eng.chi2().cpu().numpy(), constrain.chi2_from_misfit(want, obs.P))
    with pytest.raises(RuntimeError, match="no stored C rows"):
        eng.gather_summary([3], gas=0)                                # the rows mix C and E: refused as on every inverse engine
    eng.close()


# ---- isolation, checkpoint, reset ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nan_members", [(321,), (64,)])
def test_a_nan_member_touches_neither_its_neighbours_nor_their_records(lib, nan_members, prec):
    mask = 0b110
    want = _one_launch(mask, prec, True)
    R0 = np.zeros((6, N))
    R0[:, list(nan_members)] = np.nan
    got = _run(mask, N, prec, R0=R0, collect_stats=True)
    others = np.setdiff1d(np.arange(N), nan_members)
    _assert_same(got, want, (nan_members, prec), members=others)
    assert np.isnan(got["T"][..., list(nan_members)]).all() and np.isnan(got["R"][..., list(nan_members)]).all()
    clean = [r for r in range(want["records"].shape[0]) if r not in {m // 64 for m in nan_members}]
    assert _same_bits(got["records"][clean], want["records"][clean]), (nan_members, prec, "records")


def test_a_resumed_fp32_checkpoint_continues_the_run(lib):
    mask = 0b110
    want = _one_launch(mask, "f32")
    first = _engine(mask, N, "f32")
    first.run(0, 5)
    state = first.state_dict()
    assert state["t_next"] == 5 and state["conc_mask"] == mask and np.any(state["cumE"][1:] != 0) and not state["cumE"][0].any()
    first.close()
    other = _engine(0b001, N, "f32")
    with pytest.raises(ValueError, match="conc_mask"):
        other.load_state_dict(state)
    other.close()
    second = _engine(mask, N, "f32")
    second.load_state_dict(state)
    second.run(state["t_next"], N_STEPS)
    got = _state(second)
    second.close()
    _assert_same(got, want, ("resumed",), names=("R", "S", "cum"))
    _assert_same({k: got[k][5:] for k in ("X", "T")}, {k: want[k][5:] for k in ("X", "T")}, ("resumed",), names=("X", "T"))


@pytest.mark.parametrize("prec", PRECS)
def test_reset_state_zeroes_the_cumulative_emissions(lib, prec):
    mask = 0b110
    want = _one_launch(mask, prec)
    eng = _engine(mask, N, prec)
    eng.run(0, N_STEPS)
    assert bool((eng.cumE[1:] != 0).any()) and not bool(eng.cumE[0].any())
    eng.reset_state()
    assert not bool(eng.cumE.any()) and not bool(eng.R.any()) and eng.t_next == 0
    eng.run(0, N_STEPS)
    _assert_same(_state(eng), want, (prec, "second run"))
    eng.close()
