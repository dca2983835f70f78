"""The concentration-driven (inverse) form, fused_kernel<.., INV = true>, in fp64 and fp32 and in every compiled pool layout — all
22 instantiations — on the cases of tests/inverse_reference.py (12-step target series that start at C0, rise, are held, fall
through C0, sit below it with E < 0 and cum < 0, and return; dt = 1, 0.5, 0.25 and 2; 16 distinct fp32-exact members tiled to the
ensemble size).

ANCHORED ACCURACY: the device runs one step at a time; before each step the state it holds (R, S, cumE) is read back and the
guarded 50-digit step (tests/step_reference.py, step_inverse) is evaluated from exactly that state; E, T, R, S and cumE of the
step are held to  |got - ref| <= 8 max(K, 1) eps(dtype) scale  (K: tests/test_inverse_cpu.py, the NumPy oracle's own figure;
the 8: tests/test_step_edges_gpu.py), in fp64 never more than the project's tolerances.  Errors do not accumulate, so no
allowance for a trajectory is needed — and none is made:

ONE ARITHMETIC: one launch over the 12 steps equals the chain of 12 single-step launches bit for bit in E, T, R, S and cumE, as
does every split, a run across the drive table's LDS refill at step FIVEEQ_FUSED_CHUNK = 125, every ensemble size, a sub-range
of a longer allocation (ld > n) through the C ABI, a resumed checkpoint and a run after reset_state().

N = 323 = 256 + 64 + 3 members: two workgroups, the second with one full wave, one wave of 3 members and two idle waves,
whose lanes shadow member 0 and store nothing.
"""
import ctypes
import functools

import numpy as np
import pytest

import inverse_reference as ir
import step_reference as sr
from test_inverse_cpu import K

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_step_edges_gpu import BOUND, PROJECT_TOL, _same_bits      # noqa: E402  (the bound's factor and the project's tolerances)

N = 323
N_STEPS = ir.N_STEPS
DTYPE = {"f64": torch.float64, "f32": torch.float32}
PRECS = ("f64", "f32")
STATE = ("E", "T", "R", "S", "cum")
FLAGSHIP = "multigas dt=0.5"                      # the default 4 + 1 + 1 set (the 1e6-year pool) at a dt that is not 1


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from fiveeqscm_amd import _capi
    return _capi.load()                       # the HIP library must be the thing that runs: no fallback


def _engine(name, n, prec, n_steps=N_STEPS, **kw):
    from fiveeqscm_amd.engine import EnsembleEngine
    c = ir.case(name)
    return EnsembleEngine(ir.tiled_params(c, n), n, ir.target_series(c["params"]["PI_conc"], n_steps),
                          F_ext=ir.f_ext_series(n_steps), dt=c["dt"], dtype=DTYPE[prec], concentration_driven=True,
                          device="cuda:0", **kw)


def _state(eng):
    """E [n_rows, G, n], T [n_rows, n] and the state R [SP, n], S [2, n], cum [G, n] as host arrays in the engine's precision."""
    torch.cuda.synchronize()
    return {"E": eng.E.cpu().numpy(), "T": eng.T.cpu().numpy(), "R": eng.R.cpu().numpy(), "S": eng.S.cpu().numpy(),
            "cum": eng.cumE.cpu().numpy()}


def _run(name, n, prec, cuts=(0, N_STEPS), n_steps=N_STEPS, **kw):
    """The state after run(cuts[0], cuts[1]); run(cuts[1], cuts[2]); ... on a fresh engine."""
    eng = _engine(name, n, prec, n_steps, **kw)
    for a, b in zip(cuts, cuts[1:]):
        eng.run(a, b)
    out = _state(eng)
    if kw.get("collect_stats"):
        out["records"] = eng.T_stats.cpu().numpy()                   # [ceil(n / 64), n_steps, 4]
        out["moments"] = {k: v.cpu().numpy() for k, v in eng.stats().items()}
    eng.close()
    return out


@functools.lru_cache(maxsize=None)
def _one_launch(name, prec, collect_stats=False):
    """run(0, 12) of the N-member ensemble in one launch: computed once, shared, read-only."""
    out = _run(name, N, prec, collect_stats=collect_stats)
    assert all(np.isfinite(out[k]).all() for k in STATE), (name, prec)
    return out


def _assert_same(got, want, what, members=slice(None), names=STATE):
    for k in names:
        assert _same_bits(got[k][..., members], want[k][..., members]), (*what, k)


# ---- anchored accuracy --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ir.CASES)
def test_every_step_against_the_50_digit_step_from_the_device_state(lib, name, prec):
    """Worst multiples of eps(dtype) x scale over the 12 steps x 16 members, measured on the MI355X, 2026-10-18 (bound:
    8 max(K, 1), that is 8 except E and cumE of 4+1: 19 and 18; R of {2}, 4+4+1 and co2 dt=1: 21, 27 and 17; T and S of the
    co2 sets: 27 to 31):

        case              fp64:  E      T      R      S     cumE    fp32:  E      T      R      S     cumE
        {1}                     0.017  0.827  0.511  0.842  0.015          0.018  0.587  0.503  0.594  0.018
        {2}                     0.021  1.058  2.850  1.008  0.023          0.011  0.646  0.944  0.578  0.011
        {3}                     0.011  1.013  1.074  1.009  0.013          0.016  0.654  0.834  0.581  0.016
        {4}                     0.022  0.888  0.907  0.916  0.022          0.014  0.491  0.718  0.686  0.015
        1+1                     0.124  0.587  0.704  0.578  0.098          0.084  0.432  0.922  0.434  0.118
        4+1                     2.396  0.613  1.042  0.599  2.249          0.083  0.398  0.889  0.399  0.114
        4+4                     0.095  0.598  1.561  0.599  0.108          0.110  0.445  1.435  0.425  0.108
        1+1+1                   0.071  0.374  0.893  0.364  0.095          0.089  0.226  1.004  0.245  0.080
        4+1+1                   0.108  0.365  2.267  0.355  0.125          0.110  0.227  0.753  0.248  0.129
        4+4+1                   0.255  0.382  3.568  0.395  0.261          0.073  0.258  1.503  0.231  0.098
        4+4+4                   0.094  0.420  1.291  0.405  0.107          0.076  0.222  1.233  0.223  0.085
        multigas dt=1           0.081  0.409  1.560  0.394  0.080          0.057  0.225  1.334  0.235  0.058
        multigas dt=0.5         0.079  0.429  0.889  0.389  0.072          0.076  0.240  0.972  0.231  0.075
        co2 dt=1                0.009  4.522  1.463  4.558  0.009          0.013  4.071  1.608  4.129  0.013
        co2 dt=0.5              0.011  4.078  1.131  3.933  0.011          0.008  3.629  1.099  3.644  0.008

    fp32 is no worse than fp64 in these units anywhere: nothing in the inverse step cancels beyond what its scales carry, and
    num - (target - C0) in particular does not (target - C0 is exact for these targets; E sits at a tenth of a unit because
    its scale carries (|C*| + |C0|) / den).  The three figures that stand out are the oracle's own (K) and have its causes:
    E and cumE of 4+1 in fp64 (2.396 and 2.249, the oracle's to the digit) are the host's fp64 g0 and g1 of a one-pool gas
    with tau = 359 yr, shared with the oracle, and vanish in fp32 units; T and S of the CO2-only sets (4.6 against the
    oracle's 3.9) are f1 ln(C / C0) at C within 4 % of C0, whose T scale counts the log's 0.04 f1 where the rounding of C
    weighs f1 eps.  The test prints every figure.

    Members 16 .. 322 carry the bits of their replica among the first 16 in every output at every step, and step 0 (a zero
    state and a target equal to C0) diagnoses E == 0 exactly."""
    c = ir.case(name)
    eps, replica = sr.EPS[prec], np.arange(N) % ir.M
    eng = _engine(name, N, prec)
    worst, failures = dict.fromkeys(ir.OUTPUTS, 0.0), []
    before = _state(eng)
    for t in range(N_STEPS):
        eng.run(t, t + 1)
        after = _state(eng)
        got = {"E": after["E"][t], "T": after["T"][t][None, :], "R": after["R"], "S": after["S"], "cum": after["cum"]}
        for out, x in got.items():
            assert np.isfinite(x).all(), (name, prec, t, out)
            assert _same_bits(x, x[:, replica]), (name, prec, t, out, "a member differs from its replica")
        if t == 0:
            assert np.all(got["E"] == 0), (name, prec, "E at step 0")
        ref = ir.step_reference(c, *(before[k][:, :ir.M].astype(np.float64) for k in ("R", "S", "cum")), t)
        for out, u in ir.units({k: x[:, :ir.M].astype(np.float64) for k, x in got.items()}, ref, eps).items():
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
    print(f"{name} {prec}: worst x eps x scale " + " ".join(f"{out} {v:.3f}" for out, v in worst.items()))
    assert not failures, (name, prec, failures)


# ---- one arithmetic -------------------------------------------------------------------------------------------------------------
ONE_ARITHMETIC_CASES = (FLAGSHIP, "co2 dt=1", "{2}", "4+4+4")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ONE_ARITHMETIC_CASES)
def test_one_launch_equals_the_chain_of_single_step_launches(lib, name, prec):
    """run(0, 12) == 12 launches of one step == run(0, 5); run(5, 12), in E, T, R, S and cumE."""
    want = _one_launch(name, prec)
    _assert_same(_run(name, N, prec, cuts=range(N_STEPS + 1)), want, (name, prec, "12 single steps"))
    _assert_same(_run(name, N, prec, cuts=(0, 5, N_STEPS)), want, (name, prec, "5 + 7"))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ONE_ARITHMETIC_CASES)
def test_a_launch_across_the_drive_refill_equals_launches_that_end_at_it(lib, name, prec):
    """130 steps (the 12-step shape repeated): one launch refills its LDS drive chunk at step 125; (0, 125), (125, 130) never
    refills, (0, 124), (124, 130) starts its second chunk one step earlier."""
    want = _run(name, N, prec, cuts=(0, 130), n_steps=130)
    assert all(np.isfinite(want[k]).all() for k in STATE), (name, prec)
    for cuts in ((0, 125, 130), (0, 124, 130)):
        _assert_same(_run(name, N, prec, cuts=cuts, n_steps=130), want, (name, prec, cuts))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ONE_ARITHMETIC_CASES)
def test_stored_steps_are_the_rows_of_the_full_run(lib, name, prec):
    """output_steps = a subset: the stored E and T rows are the full run's rows of those steps; R, S and cumE are unchanged."""
    want = _one_launch(name, prec)
    steps = [0, 4, 5, 11]
    got = _run(name, N, prec, output_steps=steps)
    assert got["E"].shape[0] == got["T"].shape[0] == len(steps)
    _assert_same(got, {**want, "E": want["E"][steps], "T": want["T"][steps]}, (name, prec, "output_steps"))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_every_ensemble_size_gives_the_members_of_the_323_member_run(lib, n, prec):
    """1 member; a wave less one, a full wave, a wave and one; a workgroup and one: every member has the bits of the same
    member of the 323-member run."""
    got = _run(FLAGSHIP, n, prec)
    _assert_same(got, {k: v[..., :n] for k, v in _one_launch(FLAGSHIP, prec).items()}, (n, prec))


# ---- a sub-range of a longer allocation, through the C ABI -------------------------------------------------------------------------
SENTINEL = -12345.0


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("ld", [330, 331])
def test_a_member_sub_range_of_a_longer_allocation(lib, ld, prec):
    """fiveeq_run_inverse_f32 / _f64 on members [3, 260) of rows of length ld = 330 (even: an fp32 forward call would pack) and
    331, every row pointer — cumE included — offset by 3 members: the members of the range get the bits of a stand-alone
    257-member run, every other word of R, S, cumE, E_traj and T_traj keeps its sentinel."""
    n, m0 = 257, 3
    alone = _engine(FLAGSHIP, n, prec)
    alone.run(0, N_STEPS)
    want = _state(alone)
    G, SP, dtype = alone.n_gas, alone.sum_pools, DTYPE[prec]
    rows = {"r": 3 * G, "q": 2, "R": SP, "S": 2, "cum": G, "E": alone.n_rows * G, "T": alone.n_rows}
    buf = {k: torch.full((k_rows, ld), SENTINEL, dtype=dtype, device="cuda:0") for k, k_rows in rows.items()}
    buf["r"][:, m0:m0 + n], buf["q"][:, m0:m0 + n] = alone.r, alone.q
    for k in ("R", "S", "cum"):
        buf[k][:, m0:m0 + n] = 0.0
    assert m0 + n <= ld and all(t.is_contiguous() for t in buf.values())
    at = lambda t: ctypes.c_void_p(t.data_ptr() + m0 * t.element_size())          # noqa: E731
    with torch.cuda.device(alone.device):
        rc = getattr(lib, f"fiveeq_run_inverse_{prec}")(
            ctypes.byref(alone.model), n, ld, ctypes.c_void_p(alone.drive.data_ptr()), alone.n_steps, 0, N_STEPS, at(buf["r"]),
            at(buf["q"]), at(buf["R"]), at(buf["S"]), at(buf["cum"]), at(buf["E"]), at(buf["T"]), alone.n_rows, None,
            alone._stream())
    assert rc == 0, lib.fiveeq_last_error()
    torch.cuda.synchronize()
    outside = np.ones(ld, dtype=bool)
    outside[m0:m0 + n] = False
    for k in STATE:
        x = buf[k].cpu().numpy()
        assert _same_bits(x[:, m0:m0 + n].reshape(want[k].shape), want[k]), (ld, prec, k)
        assert np.all(x[:, outside] == SENTINEL), (ld, prec, k, "a word outside the range was written")
    alone.close()


# ---- statistics ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_statistics_of_the_inverse_run(lib, prec):
    """collect_stats=True: the mean against the exactly summed fp64 mean of the stored T rows to rtol 1e-13, min and max exact,
    the records of the one-launch run and of the 5 + 7 split identical, and T, E and the state as without statistics."""
    import math
    one = _one_launch(FLAGSHIP, prec, True)
    _assert_same(one, _one_launch(FLAGSHIP, prec), (prec, "collect_stats changed the run"))
    T = one["T"].astype(np.float64)
    mean = np.array([math.fsum(row) for row in T]) / N
    print(f"{prec}: mean, worst relative difference {np.max(np.abs(one['moments']['mean'] - mean) / np.abs(mean)):.3g}")
    np.testing.assert_allclose(one["moments"]["mean"], mean, rtol=1e-13, atol=0)
    assert np.array_equal(one["moments"]["min"], T.min(1)) and np.array_equal(one["moments"]["max"], T.max(1))
    assert np.all(one["moments"]["count"] == N)
    split = _run(FLAGSHIP, N, prec, cuts=(0, 5, N_STEPS), collect_stats=True)
    assert _same_bits(split["records"], one["records"]), (prec, "records of the 5 + 7 split")


# ---- isolation of a non-finite member ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("nan_members", [(321,), (64,), (64, 321)])
def test_a_nan_member_touches_neither_its_neighbours_nor_their_records(lib, nan_members, prec):
    """Pools of NaN in member 321 (the 3-member last wave), in member 64 (first of the second record), in both: every other
    member keeps the bits of the clean run in E, T, R, S and cumE, and so does every statistics record without a NaN member."""
    want = _one_launch(FLAGSHIP, prec, True)
    R0 = np.zeros((sum(ir.case(FLAGSHIP)["pools"]), N))
    R0[:, list(nan_members)] = np.nan
    got = _run(FLAGSHIP, N, prec, R0=R0, collect_stats=True)
    others = np.setdiff1d(np.arange(N), nan_members)
    _assert_same(got, want, (nan_members, prec), members=others)
    for k in STATE:
        assert np.isnan(got[k][..., list(nan_members)]).all(), (nan_members, prec, k)      # (and the member itself stays NaN)
    clean = [r for r in range(want["records"].shape[0]) if r not in {m // 64 for m in nan_members}]
    assert len(clean) == want["records"].shape[0] - len(nan_members)
    assert _same_bits(got["records"][clean], want["records"][clean]), (nan_members, prec, "records")


# ---- checkpoint, reset ----------------------------------------------------------------------------------------------------------------
def test_a_resumed_fp32_checkpoint_continues_the_run(lib):
    """An fp32 inverse engine run to step 5, its state_dict() loaded into a fresh engine, run to 12: the bits of the
    uninterrupted run — cumE, which only this form carries, included."""
    want = _one_launch(FLAGSHIP, "f32")
    first = _engine(FLAGSHIP, N, "f32")
    first.run(0, 5)
    state = first.state_dict()
    assert state["t_next"] == 5 and state["cumE"].shape == (3, N) and np.any(state["cumE"] != 0)
    first.close()
    second = _engine(FLAGSHIP, N, "f32")
    second.load_state_dict(state)
    second.run(state["t_next"], N_STEPS)
    got = _state(second)
    second.close()
    _assert_same(got, want, ("resumed",), names=("R", "S", "cum"))
    _assert_same({k: got[k][5:] for k in ("E", "T")}, {k: want[k][5:] for k in ("E", "T")}, ("resumed",), names=("E", "T"))


@pytest.mark.parametrize("prec", PRECS)
def test_reset_state_zeroes_the_cumulative_emissions(lib, prec):
    """... and a second run reproduces the first."""
    want = _one_launch(FLAGSHIP, prec)
    eng = _engine(FLAGSHIP, N, prec)
    eng.run(0, N_STEPS)
    assert bool((eng.cumE != 0).any())
    eng.reset_state()
    assert not bool(eng.cumE.any()) and not bool(eng.R.any()) and eng.t_next == 0
    eng.run(0, N_STEPS)
    _assert_same(_state(eng), want, (prec, "second run"))
    eng.close()
