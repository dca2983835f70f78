"""Concentration-driven runs with per-member forcing scales and the in-loop misfit — ConcentrationDrivenEngine over
fiveeq_run_inverse_forc_*, fused_kernel<.., INV = true, .., MISFIT, .., FORC> — in fp64 and fp32 and both pool layouts that carry
the features, on the cases of tests/inverse_forcing_reference.py (the inverse cases of tests/inverse_reference.py with gas scales
in 0.75 .. 1.25, K = 3 categories scaled by 0.25 .. 2, every input exact in fp32).

ANCHORED ACCURACY as tests/test_inverse_gpu.py has it: the device runs one step at a time, the 50-digit step of each member's
own model is evaluated from the state the device holds, and E, T, R, S and cumE of the step are held to
|got - ref| <= 8 max(K, 1) eps(dtype) scale (K: tests/test_inverse_forcing_cpu.py), in fp64 never past the project's tolerances.
ONE ARITHMETIC: every other run equals those bits.

N = 323 = 256 + 64 + 3 members: two workgroups, the second with one full wave, one wave of 3 members and two idle waves.  130
steps where a refill of the staged drive and table chunks must be crossed: the fp64 4 + 1 + 1 forms with scales stage 25 steps
(refills at 25, 50, ..), every other form 125.
"""
import ctypes
import functools

import numpy as np
import pytest

import inverse_forcing_reference as fr
import step_reference as sr
from test_inverse_forcing_cpu import K

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_step_edges_gpu import BOUND, PROJECT_TOL, _same_bits      # noqa: E402  (the bound's factor and the project's tolerances)

from fiveeqscm_amd import constrain                                 # noqa: E402
from fiveeqscm_amd.forcing import ExternalForcings                  # noqa: E402
from oracle import fiveeq_oracle as npo                             # noqa: E402

N = 323
N_STEPS = fr.N_STEPS
DTYPE = {"f64": torch.float64, "f32": torch.float32}
PRECS = ("f64", "f32")
STATE = ("E", "T", "R", "S", "cum")
FLAGSHIP = "multigas dt=0.5"
BOTH_LAYOUTS = (FLAGSHIP, "co2 dt=1")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from fiveeqscm_amd import _capi
    return _capi.load()                       # the HIP library must be the thing that runs: no fallback


@functools.lru_cache(maxsize=None)
def _obs(n_steps):
    """Observed warming at steps 3 .. n - 1 except every fifth (gaps: steps the kernel skips), baseline steps 1 .. 4."""
    t = np.arange(n_steps)
    at = t[(t >= 3) & (t % 5 != 0)]
    return constrain.Observations.from_years(t.astype(float), at.astype(float), 0.02 + 0.003 * at, 0.05, (1.0, 4.0))


def _engine(name, n, prec, n_steps=N_STEPS, forc=True, obs=False, params=None, table=None, **kw):
    from fiveeqscm_amd import ConcentrationDrivenEngine
    c = fr.case(name, n_steps)
    p = fr.tiled_params(c, n) if params is None else params
    if not forc:
        p = {k: v for k, v in p.items() if k not in ("f_scale", "fx_scale")}
    fx = (ExternalForcings(c["X"] if table is None else table) if forc else None)
    return ConcentrationDrivenEngine(p, n, c["target"], F_ext=c["F_ext"], dt=c["dt"], dtype=DTYPE[prec], device="cuda:0",
                                     forcing=fx, observations=_obs(n_steps) if obs else None, **kw)


def _plain_engine(name, n, prec, n_steps=N_STEPS, **kw):
    from fiveeqscm_amd.engine import EnsembleEngine
    c = fr.case(name, n_steps)
    p = {k: v for k, v in fr.tiled_params(c, n).items() if k not in ("f_scale", "fx_scale")}
    return EnsembleEngine(p, n, c["target"], F_ext=c["F_ext"], dt=c["dt"], dtype=DTYPE[prec], concentration_driven=True,
                          device="cuda:0", **kw)


def _state(eng):
    torch.cuda.synchronize()
    out = {"E": eng.E.cpu().numpy(), "T": eng.T.cpu().numpy(), "R": eng.R.cpu().numpy(), "S": eng.S.cpu().numpy(),
           "cum": eng.cumE.cpu().numpy()}
    if eng.misfit is not None:
        out["misfit"] = eng.misfit.cpu().numpy()
    if eng.T_stats is not None:
        out["records"] = eng.T_stats.cpu().numpy()
    return out


def _run(name, n, prec, cuts=(0, N_STEPS), n_steps=N_STEPS, **kw):
    eng = _engine(name, n, prec, n_steps, **kw)
    for a, b in zip(cuts, cuts[1:]):
        eng.run(a, b)
    out = _state(eng)
    eng.close()
    return out


@functools.lru_cache(maxsize=None)
def _one_launch(name, prec, n_steps=N_STEPS, obs=True, collect_stats=False):
    """run(0, n_steps) of the N-member ensemble with scales (and the misfit) in one launch: computed once, shared, read-only."""
    out = _run(name, N, prec, cuts=(0, n_steps), n_steps=n_steps, obs=obs, collect_stats=collect_stats)
    assert all(np.isfinite(out[k]).all() for k in STATE), (name, prec)
    return out


def _assert_same(got, want, what, members=slice(None), names=STATE):
    for k in names:
        assert _same_bits(got[k][..., members], want[k][..., members]), (*what, k)


ALL = STATE + ("misfit",)


# ---- 1. anchored accuracy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obs", [False, True], ids=["forc", "forc+misfit"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", fr.CASES)
def test_every_step_against_the_50_digit_step_from_the_device_state(lib, name, prec, obs):
    """Worst multiples of eps(dtype) x scale over the 12 steps x 16 members (bound: 8 max(K, 1)); the test prints every figure.
    Measured on the MI355X, 2026-10-20 (with and without the misfit: the same figures, the misfit touches no output):

        case              fp64:  E      T      R      S     cumE    fp32:  E      T      R      S     cumE
        {4}                     0.021  0.875  0.982  0.698  0.020          0.009  0.604  0.644  0.623  0.013
        4+1+1                   0.102  0.488  2.156  0.612  0.100          0.153  0.332  1.042  0.388  0.172
        multigas dt=0.5         0.055  0.448  0.745  0.407  0.058          0.067  0.377  1.141  0.434  0.067
        co2 dt=1                0.012  1.520  1.047  2.015  0.012          0.008  3.784  1.158  4.038  0.008

    Every figure is at most 0.5 of its bound (8 max(K, 1): 8, except R of 4+1+1, multigas and co2 9.6, 12 and 12; T and S of
    co2 14 and 14.8).  T and S of co2 dt=1 in fp32 (3.8, 4.0) are the figures of the form without scales
    (tests/test_inverse_gpu.py: 4.1): f1 ln(C / C0) at C within 4 % of C0.

    Members 16 .. 322 carry the bits of their replica among the first 16 in every output at every step."""
    c = fr.case(name)
    eps, replica = sr.EPS[prec], np.arange(N) % fr.M
    eng = _engine(name, N, prec, obs=obs)
    worst, failures = dict.fromkeys(fr.OUTPUTS, 0.0), []
    before = _state(eng)
    for t in range(N_STEPS):
        eng.run(t, t + 1)
        after = _state(eng)
        got = {"E": after["E"][t], "T": after["T"][t][None, :], "R": after["R"], "S": after["S"], "cum": after["cum"]}
        for out, x in got.items():
            assert np.isfinite(x).all(), (name, prec, t, out)
            assert _same_bits(x, x[:, replica]), (name, prec, t, out, "a member differs from its replica")
        ref = fr.step_reference(c, *(before[k][:, :fr.M].astype(np.float64) for k in ("R", "S", "cum")), t)
        for out, u in fr.units({k: x[:, :fr.M].astype(np.float64) for k, x in got.items()}, ref, eps).items():
            limit = np.full_like(u, BOUND * max(K[name][out], 1.0))
            if (prec, out) in PROJECT_TOL:                              # ... and never past the project's tolerance
                rtol, atol = PROJECT_TOL[(prec, out)]
                scale = sr.scale_of(ref, out, eps)
                with np.errstate(divide="ignore"):
                    limit = np.minimum(limit, np.where(scale > 0, (rtol * np.abs(ref[out][0]) + atol) / (eps * scale), np.inf))
            worst[out] = max(worst[out], float(u.max()))
            if np.any(u > limit):
                row, m = np.unravel_index(np.argmax(u / limit), u.shape)
                failures.append((t, out, int(row), int(m), float(u[row, m]), float(limit[row, m])))
        before = after
    eng.close()
    print(f"{name} {prec} obs={obs}: worst x eps x scale " + " ".join(f"{out} {v:.3f}" for out, v in worst.items()))
    assert not failures, (name, prec, failures)


# ---- 2. the whole run against the oracle, member by member ------------------------------------------------------------------------
@pytest.mark.parametrize("name", BOTH_LAYOUTS)
def test_fp64_whole_run_against_the_oracle_run_member_by_member(lib, name):
    """130 steps, N = 48 (the 16 members three times): each member against oracle.run_inverse run alone on its scaled f and its
    summed external forcing.  Bounds: those tests/test_engine_gpu.py::test_inverse_mode_matches_oracle_and_round_trips holds
    the plain inverse form to — E rtol 1e-8 atol 1e-9, T 1e-10 / 1e-13, cumE 1e-9 / 1e-9, R 1e-10 / 1e-11."""
    n, n_steps = 48, 130
    want = fr.oracle_run(name, n_steps)
    got = _run(name, n, "f64", cuts=(0, n_steps), n_steps=n_steps, obs=True)
    idx = np.arange(n) % fr.M
    for k, rtol, atol in (("E", 1e-8, 1e-9), ("T", 1e-10, 1e-13), ("cum", 1e-9, 1e-9), ("R", 1e-10, 1e-11)):
        ref = want[k][..., idx]
        err = np.abs(got[k] - ref) / (rtol * np.abs(ref) + atol)
        print(f"{name} {k}: worst err / bound {err.max():.3g}")
        assert np.isfinite(got[k]).all() and err.max() <= 1.0, (name, k, float(err.max()))


# ---- 3. bit identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", BOTH_LAYOUTS)
def test_unit_scales_are_the_plain_inverse_run_bit_for_bit(lib, name, prec):
    """Unit gas scales with K = 0; with a NULL table (through the C ABI); with an all-zero table under the case's category
    scales; and the class without forcing= and observations=: E, T, R, S, cumE and the wave records of
    EnsembleEngine(concentration_driven=True)."""
    n_steps = 130
    plain = _plain_engine(name, N, prec, n_steps, collect_stats=True)
    plain.run()
    want = _state(plain)
    c = fr.case(name, n_steps)
    ones = dict(fr.tiled_params(c, N), f_scale=np.ones(c["n_gas"]))
    zero_table = dict(ones, fx_scale=fr.tiled_params(c, N)["fx_scale"])
    no_cat = {k: v for k, v in ones.items() if k != "fx_scale"}
    runs = {"K = 0": dict(params=no_cat, table=np.zeros((n_steps, 0))), "zero table": dict(params=zero_table, table=np.zeros((n_steps, 3))),
            "no feature": dict(forc=False)}
    for what, kw in runs.items():
        eng = _engine(name, N, prec, n_steps, collect_stats=True, **kw)
        eng.run()
        _assert_same(_state(eng), want, (name, prec, what), names=STATE + ("records",))
        eng.close()
    eng = _engine(name, N, prec, n_steps, params=no_cat, table=np.zeros((n_steps, 0)), collect_stats=True)
    eng._wave_stats()
    with torch.cuda.device(eng.device):
        rc = eng._fn("run_inverse_forc")(*eng._run_args(0, n_steps, cumE=eng._ptr(eng.cumE)), eng._ptr(eng.fscale), None, 0, None, None,
                                         eng._stream())
    assert rc == 0, lib.fiveeq_last_error()
    _assert_same(_state(eng), want, (name, prec, "NULL table"), names=STATE + ("records",))
    eng.close()
    plain.close()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", BOTH_LAYOUTS)
def test_observations_change_nothing_and_the_misfit_is_that_of_the_stored_T(lib, name, prec):
    """observations= changes none of E, T, R, S, cumE — with scales and without; misfit == constrain.misfit_numpy(stored T,
    table) == eng.score({"T": ...}).misfit["T"], bit for bit; chi2() is chi2_from_misfit of it."""
    obs = _obs(N_STEPS)
    for forc in (True, False):
        without = _run(name, N, prec, forc=forc)
        eng = _engine(name, N, prec, forc=forc, obs=True)
        eng.run()
        got = _state(eng)
        _assert_same(got, without, (name, prec, forc, "observations= changed the run"))
        want = constrain.misfit_numpy(got["T"], obs.table)
        assert got["misfit"].any() and _same_bits(got["misfit"], want), (name, prec, forc)
        score = eng.score({"T": obs})
        assert _same_bits(score.misfit["T"].cpu().numpy(), want)
        assert _same_bits(eng.chi2().cpu().numpy(), constrain.chi2_from_misfit(want, obs.P))
        eng.close()
    assert _same_bits(_one_launch(name, prec)["misfit"], constrain.misfit_numpy(_one_launch(name, prec)["T"], obs.table))


@pytest.mark.parametrize("obs", [False, True], ids=["forc", "forc+misfit"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", BOTH_LAYOUTS)
def test_one_launch_equals_the_chain_of_single_step_launches(lib, name, prec, obs):
    want = _one_launch(name, prec, obs=obs)
    names = ALL if obs else STATE
    _assert_same(_run(name, N, prec, cuts=range(N_STEPS + 1), obs=obs), want, (name, prec, "12 single steps"), names=names)
    _assert_same(_run(name, N, prec, cuts=(0, 5, N_STEPS), obs=obs), want, (name, prec, "5 + 7"), names=names)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", BOTH_LAYOUTS)
def test_one_launch_equals_every_split_at_and_across_the_refills(lib, name, prec):
    """130 steps: one launch refills its staged chunks at step 25 (the fp64 4 + 1 + 1 form with scales: every 25 steps) or at
    step 125 (every other form); splits that end at, one before and one after both steps, with the misfit."""
    want = _one_launch(name, prec, n_steps=130)
    for cuts in ((0, 25, 125, 130), (0, 24, 124, 130), (0, 26, 126, 130), (0, 25, 130), (0, 125, 130)):
        _assert_same(_run(name, N, prec, cuts=cuts, n_steps=130, obs=True), want, (name, prec, cuts), names=ALL)
    # ... and without the misfit (the FORC-only kernel) the same E, T, R, S, cumE
    _assert_same(_run(name, N, prec, cuts=(0, 25, 125, 130), n_steps=130), want, (name, prec, "FORC only"))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_every_ensemble_size_gives_the_members_of_the_323_member_run(lib, n, prec):
    got = _run(FLAGSHIP, n, prec, obs=True)
    _assert_same(got, {k: v[..., :n] for k, v in _one_launch(FLAGSHIP, prec).items()}, (n, prec), names=ALL)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", BOTH_LAYOUTS)
def test_stored_steps_are_the_rows_of_the_full_run(lib, name, prec):
    want = _one_launch(name, prec)
    steps = [0, 4, 5, 11]
    eng = _engine(name, N, prec, output_steps=steps)
    eng.run()
    got = _state(eng)
    eng.close()
    assert got["E"].shape[0] == got["T"].shape[0] == len(steps)
    _assert_same(got, {**want, "E": want["E"][steps], "T": want["T"][steps]}, (name, prec, "output_steps"))


SENTINEL = -12345.0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ld", [330, 331])
def test_a_member_sub_range_of_a_longer_allocation(lib, ld, prec):
    """fiveeq_run_inverse_forc_* on members [3, 260) of rows of length ld = 330 and 331, every row pointer — cumE, the scale rows
    and the misfit rows included — offset by 3 members: the range gets the bits of a stand-alone 257-member run, every other word
    keeps its sentinel."""
    n, m0 = 257, 3
    alone = _engine(FLAGSHIP, n, prec, obs=True)
    alone.run(0, N_STEPS)
    want = _state(alone)
    G, SP, dtype = alone.n_gas, alone.sum_pools, DTYPE[prec]
    rows = {"r": 3 * G, "q": 2, "R": SP, "S": 2, "cum": G, "E": alone.n_rows * G, "T": alone.n_rows, "fscale": G + 3}
    buf = {k: torch.full((k_rows, ld), SENTINEL, dtype=dtype, device="cuda:0") for k, k_rows in rows.items()}
    buf["misfit"] = torch.full((3, ld), SENTINEL, dtype=torch.float64, device="cuda:0")
    buf["r"][:, m0:m0 + n], buf["q"][:, m0:m0 + n], buf["fscale"][:, m0:m0 + n] = alone.r, alone.q, alone.fscale
    for k in ("R", "S", "cum", "misfit"):
        buf[k][:, m0:m0 + n] = 0.0
    assert m0 + n <= ld and all(t.is_contiguous() for t in buf.values())
    at = lambda t: ctypes.c_void_p(t.data_ptr() + m0 * t.element_size())          # noqa: E731
    with torch.cuda.device(alone.device):
        rc = getattr(lib, f"fiveeq_run_inverse_forc_{prec}")(
            ctypes.byref(alone.model), n, ld, ctypes.c_void_p(alone.drive.data_ptr()), alone.n_steps, 0, N_STEPS, at(buf["r"]),
            at(buf["q"]), at(buf["R"]), at(buf["S"]), at(buf["cum"]), at(buf["E"]), at(buf["T"]), alone.n_rows, None,
            at(buf["fscale"]), ctypes.c_void_p(alone.fext.data_ptr()), 3, ctypes.c_void_p(alone.obs.data_ptr()), at(buf["misfit"]),
            alone._stream())
    assert rc == 0, lib.fiveeq_last_error()
    torch.cuda.synchronize()
    outside = np.ones(ld, dtype=bool)
    outside[m0:m0 + n] = False
    for k in ALL:
        x = buf[k].cpu().numpy()
        assert _same_bits(x[:, m0:m0 + n].reshape(want[k].shape), want[k]), (ld, prec, k)
        assert np.all(x[:, outside] == SENTINEL), (ld, prec, k, "a word outside the range was written")
    x = buf["fscale"].cpu().numpy()
    assert np.all(x[:, outside] == SENTINEL) and _same_bits(x[:, m0:m0 + n], alone.fscale.cpu().numpy())     # read-only
    alone.close()


# ---- 4. isolation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("where", ["pools", "scale row"])
def test_a_nan_member_touches_neither_its_neighbours_nor_their_records(lib, where, prec):
    """NaN pools in members 64 and 321 — or a NaN in one scale row entry of each (a gas scale of 64, a category scale of 321):
    every other member keeps the clean run's bits in E, T, R, S, cumE and misfit, and so does every wave record without them."""
    bad = (64, 321)
    want = _one_launch(FLAGSHIP, prec, collect_stats=True)
    if where == "pools":
        R0 = np.zeros((sum(fr.case(FLAGSHIP)["pools"]), N))
        R0[:, list(bad)] = np.nan
        eng = _engine(FLAGSHIP, N, prec, obs=True, collect_stats=True, R0=R0)
    else:
        eng = _engine(FLAGSHIP, N, prec, obs=True, collect_stats=True)
        eng.fscale[1, 64] = float("nan")
        eng.fscale[eng.n_gas + 2, 321] = float("nan")
    eng.run()
    got = _state(eng)
    eng.close()
    others = np.setdiff1d(np.arange(N), bad)
    _assert_same(got, want, (where, prec), members=others, names=ALL)
    for k in ("T", "S", "misfit"):                                    # the member itself: NaN where the forcing reaches
        assert np.isnan(got[k][..., list(bad)]).any(axis=tuple(range(got[k].ndim - 1))).all(), (where, prec, k)
    clean = [r for r in range(want["records"].shape[0]) if r not in {m // 64 for m in bad}]
    assert len(clean) == want["records"].shape[0] - 2
    assert _same_bits(got["records"][clean], want["records"][clean]), (where, prec, "records")


# ---- 5. host ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_a_checkpoint_round_trip_mid_run_continues_bit_for_bit(lib, prec):
    """... carrying cumE, misfit and the forcing identity; a checkpoint of another forcing set is refused."""
    want = _one_launch(FLAGSHIP, prec)
    first = _engine(FLAGSHIP, N, prec, obs=True)
    first.run(0, 5)
    state = first.state_dict()
    assert state["t_next"] == 5 and state["cumE"].shape == (3, N) and np.any(state["cumE"] != 0) and np.any(state["misfit"] != 0)
    assert state["forcing_sha256"] == first.forcing.sha256 and len(state["fscale_sha256"]) == 64
    first.close()
    second = _engine(FLAGSHIP, N, prec, obs=True)
    second.load_state_dict(state)
    second.run(state["t_next"], N_STEPS)
    got = _state(second)
    second.close()
    _assert_same(got, want, ("resumed", prec), names=("R", "S", "cum", "misfit"))
    _assert_same({k: got[k][5:] for k in ("E", "T")}, {k: want[k][5:] for k in ("E", "T")}, ("resumed", prec), names=("E", "T"))
    other = _engine(FLAGSHIP, N, prec, obs=True, table=fr.case(FLAGSHIP)["X"] * 0.5)
    with pytest.raises(ValueError, match="forcing set"):
        other.load_state_dict(state)
    other.close()


def test_reset_state_parameter_rows_accounting_and_refusals(lib):
    from fiveeqscm_amd import ConcentrationDrivenEngine
    from fiveeqscm_amd.engine import EnsembleEngine
    want = _one_launch(FLAGSHIP, "f64")
    eng = _engine(FLAGSHIP, N, "f64", obs=True)
    assert isinstance(eng, EnsembleEngine) and eng.concentration_driven and tuple(eng.fscale.shape) == (6, N)
    eng.run()
    assert bool((eng.cumE != 0).any()) and bool((eng.misfit != 0).any())
    eng.reset_state()
    assert not bool(eng.cumE.any()) and not bool(eng.misfit.any()) and not bool(eng.R.any()) and eng.t_next == 0
    eng.run()
    _assert_same(_state(eng), want, ("second run",), names=ALL)
    names, rows = eng.parameter_rows()
    assert names[-6:] == ["f_scale[0]", "f_scale[1]", "f_scale[2]", "fx_scale[0]", "fx_scale[1]", "fx_scale[2]"]
    assert torch.equal(rows[-6:], eng.fscale)
    sens = eng.drivers(eng.T[-1:], names=names[-6:])                     # the scale rows as drivers of the last stored T
    assert np.isfinite(np.asarray(sens.eta2.cpu() if hasattr(sens.eta2, "cpu") else sens.eta2)).all()
    bare = _engine(FLAGSHIP, N, "f64", forc=False)
    assert eng.bytes_per_member_step("fused") > bare.bytes_per_member_step("fused")       # the scale rows and the accumulators
    summary = eng.gather_summary([3, 11])
    assert np.allclose(summary["mean"], eng.T[[3, 11]].mean(1).cpu().numpy(), rtol=1e-12)
    c = fr.case(FLAGSHIP)
    p, fx = fr.tiled_params(c, N), ExternalForcings(c["X"])
    kw = dict(F_ext=c["F_ext"], dt=c["dt"], device="cuda:0")
    with pytest.raises(ValueError, match="mode 'small'"):
        eng.run(mode="small")
    with pytest.raises(ValueError, match="mode 'small'"):
        bare.run(mode="small")
    with pytest.raises(ValueError, match="EMISSIONS"):
        eng.forcing_rows()
    with pytest.raises(ValueError, match="cumE"):
        eng.resampled(None)
    with pytest.raises(ValueError, match="several emission scenarios"):
        ConcentrationDrivenEngine(p, N, np.stack([c["target"]] * 2), forcing=fx, **kw)
    with pytest.raises(ValueError, match="histograms are not available in concentration-driven mode"):
        ConcentrationDrivenEngine(p, N, c["target"], forcing=fx, hist=(-1.0, 3.0, 64), **kw)
    with pytest.raises(ValueError, match="compensated=True is an fp32 form of the emission-driven step"):
        ConcentrationDrivenEngine(p, N, c["target"], forcing=fx, compensated=True, dtype=torch.float32, **kw)
    with pytest.raises(TypeError, match="always concentration-driven"):
        ConcentrationDrivenEngine(p, N, c["target"], forcing=fx, concentration_driven=False, **kw)
    with pytest.raises(ValueError, match="need forcing="):
        ConcentrationDrivenEngine(p, N, c["target"], **kw)
    # ... and the plain class refuses the combination as before
    with pytest.raises(ValueError, match="concentration_driven"):
        EnsembleEngine(p, N, c["target"], forcing=fx, concentration_driven=True, **kw)
    with pytest.raises(ValueError, match="concentration_driven"):
        EnsembleEngine({k: v for k, v in p.items() if "scale" not in k}, N, c["target"], observations=_obs(N_STEPS),
                       concentration_driven=True, **kw)
    eng.close()
    bare.close()


def test_the_history_is_scored_and_branches_into_an_emission_driven_projection(lib):
    """chi2() of the concentration-driven history feeds importance_weights; a forward forcing= engine started from the history's
    R and S (R0 / S0) with the same scale rows continues T without a jump: its first step is the forward step from that state —
    held to the project's fp64 tolerance (1e-10 |T| + 1e-13) against the oracle's step functions from the host copy of the
    state, and bit for bit the same in the per-step and the fused kernel."""
    from fiveeqscm_amd.engine import EnsembleEngine
    c = fr.case(FLAGSHIP)
    hist = _engine(FLAGSHIP, N, "f64", obs=True)
    hist.run()
    chi2 = hist.chi2()
    w = constrain.importance_weights(chi2)
    assert w.dtype == torch.int64 and int(w.max()) == 1 << 32 and int((w > 0).sum()) > 1 and len(torch.unique(w)) > 8
    R, S = hist.R.cpu().numpy(), hist.S.cpu().numpy()
    p, G, n_p = fr.tiled_params(c, N), c["n_gas"], 6
    E = np.tile(np.round(hist.E[-1].mean(1).cpu().numpy() * 1024) / 1024, (n_p, 1))
    Xp, Fp = fr.table(N_STEPS + n_p)[N_STEPS:], np.full(n_p, 0.25)
    kw = dict(F_ext=Fp, dt=c["dt"], forcing=ExternalForcings(Xp), R0=hist.R, S0=hist.S, device="cuda:0")
    proj, single = EnsembleEngine(p, N, E, **kw), EnsembleEngine(p, N, E, **kw)
    proj.run(mode="fused")
    single.step(0)
    torch.cuda.synchronize()
    assert torch.equal(proj.T[0], single.T[0]) and torch.equal(proj.C[0], single.C[0])
    # the forward step from (R, S) in NumPy: cumulative emissions 0 before the projection's first step, as its drive table says
    pp = c["params"]
    a, tau = np.asarray(pp["a"], float), np.asarray(pp["tau"], float)
    T_old, F, off = S[0] + S[1], np.full(N, Fp[0]), 0
    for k in range(3):
        F = F + p["fx_scale"][k] * Xp[0, k]
    for g, P in enumerate(c["pools"]):
        Rg = R[off:off + P]
        off += P
        G_a = Rg.sum(0) / pp["emis2conc"][g]
        al = npo.alpha_val(0.0 - G_a, G_a, T_old, p["r0"][g], p["rC"][g], p["rT"][g], pp["ra"][g], float(npo.g_0(a[g], tau[g])),
                           float(npo.g_1(a[g], tau[g])), float(pp["iirf_max"]))
        _, C = npo.step_conc(Rg, al, E[0, g] * pp["emis2conc"][g], a[g, :P], tau[g, :P], pp["PI_conc"][g], c["dt"])
        F = F + p["f_scale"][g] * npo.step_forc(C, pp["PI_conc"][g], np.asarray(pp["f"], float).reshape(G, 3)[g])
    _, T1 = npo.step_temp(S, F, np.asarray(p["q"], float), np.expm1(-c["dt"] / np.asarray(pp["d"], float)))
    got = proj.T[0].cpu().numpy()
    err = np.abs(got - T1) / (1e-10 * np.abs(T1) + 1e-13)
    print(f"first projected step against the NumPy forward step: worst err / bound {err.max():.3g}")
    assert err.max() <= 1.0
    # no jump: the step moved T by what one step can (|em1_d| (|S| + |q F|) summed over the boxes), from the history's last T
    em1 = np.abs(np.expm1(-c["dt"] / np.asarray(pp["d"], float)))[:, None]
    assert np.all(np.abs(got - hist.T[-1].cpu().numpy()) <= (em1 * (np.abs(S) + np.abs(np.asarray(p["q"], float) * F))).sum(0) * (1 + 1e-9))
    for e in (hist, proj, single):
        e.close()
