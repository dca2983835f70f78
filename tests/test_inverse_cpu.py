"""The inverse-form cases of tests/inverse_reference.py on the CPU: the conditions their inputs are built to meet, the NumPy
oracle's own anchored-step error in units of eps64 x scale (K: the yardstick of tests/test_inverse_gpu.py), and the proof that
the yardstick sees the mistakes it is there for."""
import numpy as np
import pytest

import inverse_reference as ir
import step_reference as sr
from oracle import fiveeq_oracle as npo

# The oracle's worst anchored-step error over the 12 steps x 16 members of each case, in units of eps64 x scale (measured
# 2026-10-18; printed by test_the_oracle_agrees_with_the_50_digit_step_at_every_step, which holds the figures to these
# constants).  E and cum sit far below a unit because their scale carries |C*| + |C0| over the denominator, against a numerator
# of a few ppm; the case 4+1 stands out because its one-pool second gas drew tau = 359 yr, where g1 = tau (1 - (1 + H/tau)
# exp(-H/tau)) cancels thirty-fold and g0 = exp(-7.5) magnifies that in alpha.  T and S of the CO2-only sets reach 3.9: their
# forcing is f1 ln(C / C0) alone, at C within 4 % of C0, where the rounding of C / C0 weighs f1 eps against a term sum of 0.04 f1.
K = {
    "{1}": {"E": 0.05, "T": 1.05, "R": 0.70, "S": 1.00, "cum": 0.05},              # measured 0.014 1.008 0.675 0.962 0.016
    "{2}": {"E": 0.05, "T": 1.05, "R": 2.65, "S": 1.00, "cum": 0.05},              # measured 0.024 1.008 2.635 0.966 0.024
    "{3}": {"E": 0.05, "T": 0.90, "R": 1.10, "S": 0.95, "cum": 0.05},              # measured 0.009 0.876 1.059 0.919 0.013
    "{4}": {"E": 0.05, "T": 1.00, "R": 0.95, "S": 1.00, "cum": 0.05},              # measured 0.014 0.955 0.918 0.976 0.017
    "1+1": {"E": 0.15, "T": 0.55, "R": 1.25, "S": 0.60, "cum": 0.15},              # measured 0.103 0.521 1.222 0.576 0.116
    "4+1": {"E": 2.40, "T": 0.50, "R": 1.30, "S": 0.50, "cum": 2.25},              # measured 2.396 0.489 1.288 0.500 2.249
    "4+4": {"E": 0.15, "T": 0.50, "R": 1.35, "S": 0.55, "cum": 0.15},              # measured 0.122 0.498 1.332 0.504 0.120
    "1+1+1": {"E": 0.10, "T": 0.40, "R": 1.00, "S": 0.40, "cum": 0.10},            # measured 0.097 0.353 0.991 0.352 0.097
    "4+1+1": {"E": 0.15, "T": 0.40, "R": 1.10, "S": 0.40, "cum": 0.15},            # measured 0.144 0.369 1.073 0.372 0.142
    "4+4+1": {"E": 0.25, "T": 0.35, "R": 3.40, "S": 0.35, "cum": 0.30},            # measured 0.247 0.350 3.373 0.341 0.251
    "4+4+4": {"E": 0.15, "T": 0.35, "R": 1.35, "S": 0.40, "cum": 0.15},            # measured 0.123 0.338 1.350 0.352 0.120
    "multigas dt=1": {"E": 0.10, "T": 0.35, "R": 1.20, "S": 0.40, "cum": 0.10},    # measured 0.081 0.334 1.173 0.359 0.081
    "multigas dt=0.5": {"E": 0.10, "T": 0.35, "R": 1.10, "S": 0.35, "cum": 0.10},  # measured 0.066 0.346 1.094 0.346 0.069
    "co2 dt=1": {"E": 0.05, "T": 3.85, "R": 2.15, "S": 3.85, "cum": 0.05},         # measured 0.014 3.821 2.120 3.806 0.014
    "co2 dt=0.5": {"E": 0.05, "T": 3.35, "R": 0.95, "S": 3.90, "cum": 0.05},       # measured 0.008 3.327 0.926 3.850 0.008
}
BOUND = 8.0            # the single-step bound's factor (tests/test_step_edges_gpu.py): |got - ref| <= 8 max(K, 1) eps scale


def test_the_cases_cover_every_compiled_layout_and_every_dt():
    names = [ir.layout_name(p) for p in ir.LAYOUTS]
    assert len(ir.LAYOUTS) == 11 and [ir.case(n)["pools"] for n in names] == [list(p) for p in ir.LAYOUTS]
    assert {ir.case(n)["dt"] for n in names} == {1.0, 0.5, 0.25, 2.0}
    assert ir.case("multigas dt=0.5")["pools"] == [4, 1, 1] and ir.case("co2 dt=1")["pools"] == [4]
    assert sorted(c["dt"] for c in map(ir.case, ir.DEFAULT_CASES)) == [0.5, 0.5, 1.0, 1.0]
    for name in ir.DEFAULT_CASES:                                   # the 1e6-year pool is there
        assert np.asarray(ir.case(name)["params"]["tau"], dtype=np.float64).reshape(-1, 4)[0, 0] == 1.0e6
    assert set(K) == set(ir.CASES)


@pytest.mark.parametrize("name", ir.CASES)
def test_the_inputs_meet_their_conditions(name):
    """Conditions on the inputs, not measurements: fp32-exact members, targets and F_ext on the 2^-10 grid, 16 distinct members,
    a target series that starts at C0, rises, is held, falls through C0, sits below it and returns; every member in domain at
    every step (C > 1e-3 C0, iIRF not within 1e-3 iirf_max of the clamp and below it); E of both signs, and E == 0 at step 0."""
    c = ir.case(name)
    p, G = c["params"], c["n_gas"]
    f32_exact = lambda x: np.array_equal(x, np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64))   # noqa: E731
    for k in ("r0", "rC", "rT", "q"):
        assert f32_exact(p[k]) and p[k].shape[1] == ir.M, k
    rows = np.concatenate([p[k] for k in ("r0", "rC", "rT", "q")])
    assert len({tuple(col) for col in rows.T}) == ir.M                                 # 16 DISTINCT members
    tiled = ir.tiled_params(c, 323)
    assert all(np.array_equal(tiled[k][:, i], p[k][:, i % ir.M]) for k in ("r0", "rC", "rT", "q") for i in (0, 16, 17, 322))
    C0 = np.asarray(p["PI_conc"], dtype=np.float64).reshape(G)
    assert f32_exact(C0)
    for n_steps in (ir.N_STEPS, 130):
        tgt, F = ir.target_series(C0, n_steps), ir.f_ext_series(n_steps)
        assert tgt.shape == (n_steps, G) and f32_exact(tgt) and f32_exact(F)
        assert np.array_equal(tgt * 1024, np.round(tgt * 1024)) and np.array_equal(F * 1024, np.round(F * 1024))
        assert np.all(np.abs(tgt) < 2.0 ** 14) and np.all(F != 0) and F.min() < 0 < F.max()
        assert np.array_equal(tgt[:ir.N_STEPS], c["target"]) and np.array_equal(tgt[12:24], tgt[:min(12, n_steps - 12)])
    x = c["target"] - C0[None, :]
    for g in range(G):
        s = x[:, g]
        assert s[0] == 0 and np.all(np.diff(s[:4]) > 0) and s[3] == s[4]              # from C0; rising; held flat
        assert s[6] > 0 > s[7] and np.all(np.diff(s[4:9]) < 0)                        # falling through C0
        assert s[8] == s[9] < 0 and s[11] > s[10] > s[9]                              # sitting below C0; returning
    worst, steps = ir.oracle_anchored(name)
    imax = float(p["iirf_max"])
    for t, (got, ref) in enumerate(steps):
        C, iirf = ref["C"][0], ref["iirf"]
        assert np.all(C >= 1e-3 * C0[:, None]), (name, t)
        assert np.all(iirf < imax) and np.all(np.abs(iirf - imax) >= 1e-3 * imax), (name, t, iirf.max())
        np.testing.assert_allclose(C, np.broadcast_to(c["target"][t][:, None], C.shape), rtol=1e-13)   # the target IS reached
    E_ref = np.array([ref["E"][0] for _, ref in steps])                               # [12, G, M]
    E_got = np.array([got["E"] for got, _ in steps])
    assert np.all(E_ref[0] == 0) and np.all(E_got[0] == 0)                            # step 0: E == 0 exactly
    assert np.all((E_ref < 0).any(axis=0)) and np.all((E_ref > 0).any(axis=0))        # both signs, every gas of every member
    cum = np.array([ref["cum"][0] for _, ref in steps])
    assert (cum < 0).any() and (cum > 0).any()                                        # ... and the feedback sees both


@pytest.mark.parametrize("name", ir.CASES)
def test_the_oracle_agrees_with_the_50_digit_step_at_every_step(name):
    """The NumPy oracle, one step at a time from its own state, against the 50-digit step from that state: E, T, R, S and cum
    of every member at every step within a few units of eps64 x scale; the worst figures are K[name] (printed; the recorded
    constants must cover them and not exceed them by more than a unit)."""
    worst, _ = ir.oracle_anchored(name)
    print(f"K[{name!r}] =", {k: round(v, 3) for k, v in worst.items()})
    for out, v in worst.items():
        assert v <= 4.0, (name, out, v)             # two fp64 programs of ~10 roundings per output: a few units, or one is wrong
        assert v <= K[name][out] <= v + 1.0, (name, out, v, K[name][out])


def test_the_restated_step_is_the_oracle_step():
    """restated_step(variant=None) — the carrier of the wrong variants below — gives the oracle's bits."""
    for name in ("multigas dt=0.5", "4+4+1", "{2}"):
        c = ir.case(name)
        _, steps = ir.anchored(c, ir.restated_step)
        for (got, _), (want, _) in zip(steps, ir.oracle_anchored(name)[1]):
            for out in ir.OUTPUTS:
                assert np.array_equal(got[out], want[out]), (name, out)


@pytest.mark.parametrize("variant,out", list(zip(ir.VARIANTS, ("cum", "E", "E"))))
@pytest.mark.parametrize("name", ["multigas dt=0.5", "4+4+4"])
def test_the_yardstick_sees_a_wrong_step(name, variant, out):
    """cum += E without dt; alpha from the shared cumulative emissions (here the ensemble MEAN of cum, the mildest form of that
    mistake: the members' own differ from it by a few per cent); one a tau c of the denominator from the neighbouring pool.
    The anchored comparison that the oracle passes with figures below 4 misses the bound of the output each mistake is made in
    by more than a thousand times (measured: 1e8 to 1e14 times) in units of eps64, the units K is measured in.
    In units of eps32, the coarser yardstick the GPU tests also use, every variant still fails, by these factors (printed):
    cum without dt 7e4 / 3e5 in cum; the neighbouring pool 3e3 / 6e3 in E and 2e5 in R; the mean cum 4 / 0.2 in E — its
    scale carries (|C*| + |C0|) / den, a thousand times the E of these series — but 1e3 / 12 in R, the pools the wrong E is
    advanced with: the reason the state is part of every comparison."""
    c = ir.case(name)
    assert c["dt"] != 1.0 and c["pools"][0] > 1
    for prec in ("f64", "f32"):
        worst, _ = ir.anchored(c, lambda *a: ir.restated_step(*a, variant=variant), eps=sr.EPS[prec])
        ratio = {o: worst[o] / (BOUND * max(K[name][o], 1.0)) for o in ir.OUTPUTS}
        print(f"{name}, {variant}, {prec}: worst / bound", {o: float(f"{v:.3g}") for o, v in ratio.items()})
        assert ratio[out] > 1e3 if prec == "f64" else max(ratio.values()) > 1.0, (name, variant, prec, ratio)


def test_step_inverse_returns_the_cumulative_emissions_after_the_step():
    """cum + E dt and |cum| + dt sE, beside the keys the edge tests use (whose bits tests/test_step_edges_cpu.py holds)."""
    import mpmath as mp
    c = ir.case("multigas dt=0.5")
    p = c["params"]
    r = [[p[k][g, 3] for k in ("r0", "rC", "rT")] for g in range(3)]
    cum = [2.5, -40.0, 0.125]
    out = sr.step_inverse(c["mc"], r, list(p["q"][:, 3]), [[1.0, 2.0, 3.0, 0.5], [-30.0], [0.25]], [0.3, 0.2], cum,
                          list(c["target"][5]), -0.25)
    with mp.workdps(sr.DPS):
        for g in range(3):
            assert out["cum"][g] == mp.mpf(cum[g]) + out["E"][g] * mp.mpf(0.5)
            assert out["scum"][g] == abs(mp.mpf(cum[g])) + mp.mpf(0.5) * out["sE"][g]
    one = npo.run_inverse(c["target"][5:6], {k: (v[:, 3:4] if k in ("r0", "rC", "rT", "q") else v) for k, v in p.items()}, 1,
                          F_ext=[-0.25], dt=0.5, R0=[np.array([[1.0], [2.0], [3.0], [0.5]]), np.array([[-30.0]]), np.array([[0.25]])],
                          S0=np.array([[0.3], [0.2]]), cumE0=np.array(cum)[:, None])
    np.testing.assert_allclose(one["cumE"][:, 0], [float(v) for v in out["cum"]], rtol=1e-12)
