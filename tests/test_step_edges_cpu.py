"""The guarded 50-digit step (tests/step_reference.py) against the fp64 oracle on the edge ensemble, the oracle's own error in
units of eps64 x scale (K_ORACLE: the yardstick of tests/test_step_edges_gpu.py), and the conditions the ensemble is built
to meet: every ordered pair of classes in one packed lane, mixed quads, octets and record boundaries, and NO member near
either decision."""
import numpy as np
import pytest

import step_reference as sr
from oracle import fiveeq_oracle as npo

# The oracle's worst error over the 202 members, in units of eps64 x scale (measured 2026-10-18; printed by
# test_reference_agrees_with_the_oracle_step, which also holds the figures to these constants).  NumPy's libm-backed step is
# good to about one unit: the yardstick max(K_ORACLE, 1) of the GPU module is 1 for every output.
K_ORACLE = {
    "multigas": {"C": 0.65, "T": 0.50, "E": 0.60},      # measured 0.636, 0.496, 0.567
    "co2": {"C": 0.65, "T": 0.85, "E": 0.15},           # measured 0.606, 0.837, 0.108
}
KINDS = ("multigas", "co2")


def _oracle_forward(kind):
    ens = sr.edge_ensemble(kind)
    offs = np.concatenate([[0], np.cumsum(ens["pools"])])
    R0 = [ens["R0"][offs[g]:offs[g + 1]] for g in range(ens["n_gas"])]
    return npo.run(ens["E"][:sr.T0 + 1], ens["params"], sr.N_MAX, F_ext=ens["F_ext"][:sr.T0 + 1], R0=R0, S0=ens["S0"],
                   t_start=sr.T0)


def _oracle_inverse(kind):
    ens = sr.edge_ensemble(kind)
    offs = np.concatenate([[0], np.cumsum(ens["pools"])])
    R0 = [ens["R0"][offs[g]:offs[g + 1]] for g in range(ens["n_gas"])]
    cum = np.repeat(sr.cum_before(ens)[:, None], sr.N_MAX, axis=1)
    return npo.run_inverse(ens["target"][None, :], ens["params"], sr.N_MAX, F_ext=ens["F_ext"][sr.T0:sr.T0 + 1], R0=R0,
                           S0=ens["S0"], cumE0=cum)


@pytest.mark.parametrize("kind", KINDS)
def test_reference_agrees_with_the_oracle_step(kind):
    """One oracle step from the prescribed state (run(..., R0=, S0=, t_start=) and run_inverse) against the 50-digit step:
    every output of every member within a few units of eps64 x scale; the worst figures for C, T and the inverse step's E
    are K_ORACLE (printed; the recorded constants must cover them and not exceed them by more than a unit)."""
    eps = sr.EPS["f64"]
    fwd, inv = _oracle_forward(kind), _oracle_inverse(kind)
    ref_f, ref_i = sr.reference(kind), sr.reference(kind, inverse=True)
    got = {"C": sr.err_units(fwd["C"][sr.T0], ref_f, "C", eps).max(),
           "T": sr.err_units(fwd["T"][sr.T0], ref_f, "T", eps).max(),
           "E": sr.err_units(inv["E"][0], ref_i, "E", eps).max()}
    others = {"R": sr.err_units(np.concatenate(fwd["R"]), ref_f, "R", eps).max(),
              "S": sr.err_units(fwd["S"], ref_f, "S", eps).max(),
              "inverse C": sr.err_units(inv["C"][0], ref_i, "C", eps).max(),
              "inverse T": sr.err_units(inv["T"][0], ref_i, "T", eps).max(),
              "inverse R": sr.err_units(np.concatenate(inv["R"]), ref_i, "R", eps).max()}
    print(f"K_oracle[{kind}] =", {k: round(float(v), 3) for k, v in got.items()},
          "others:", {k: round(float(v), 3) for k, v in others.items()})
    for name, v in {**got, **others}.items():
        assert v <= 4.0, (kind, name, v)          # two fp64 programs of ~10 roundings per output: a few units, or one is wrong
    for name, v in got.items():
        assert v <= K_ORACLE[kind][name] <= v + 1.0, (kind, name, v, K_ORACLE[kind][name])


@pytest.mark.parametrize("kind", KINDS)
def test_no_member_is_near_a_decision(kind):
    """|C_g| >= 1e-3 C0 and |iIRF - iirf_max| >= 1e-3 iirf_max for EVERY member and gas, forward and inverse (a condition on
    the inputs, not a measurement: nobody is excluded), and every class is what it says: the guarded members' guarded gas
    is at C ~ -0.5 C0, the clamped members' clamped gas is past iirf_max, nothing else is out of domain."""
    ens = sr.edge_ensemble(kind)
    C0 = np.asarray(ens["params"]["PI_conc"], dtype=np.float64).reshape(-1, 1)
    imax = float(ens["params"]["iirf_max"])
    for inverse in (False, True):
        ref = sr.reference(kind, inverse)
        C, iirf = ref["C"][0], ref["iirf"]
        assert np.all(np.abs(C) >= 1e-3 * C0), (kind, inverse, np.min(np.abs(C) / C0))
        assert np.all(np.abs(iirf - imax) >= 1e-3 * imax), (kind, inverse, np.min(np.abs(iirf - imax)))
    C, iirf = sr.reference(kind)["C"][0], sr.reference(kind)["iirf"]
    g_idx = np.arange(ens["n_gas"])[:, None]
    want_guard = np.isin(ens["cls"], (sr.GUARDED, sr.BOTH))[None, :] & (ens["guard_gas"][None, :] == g_idx)
    want_clamp = np.isin(ens["cls"], (sr.CLAMPED, sr.BOTH))[None, :] & (ens["clamp_gas"][None, :] == g_idx)
    assert np.array_equal(C <= 0, want_guard) and np.array_equal(iirf > imax, want_clamp)
    offs = np.concatenate([[0], np.cumsum(ens["pools"])])
    for g in range(ens["n_gas"]):                                    # pools summing to -1.5 C0 (to their fp32 rounding) ...
        np.testing.assert_allclose(ens["R0"][offs[g]:offs[g + 1], want_guard[g]].sum(0), -1.5 * C0[g, 0], rtol=1e-6)
    ratio = C[want_guard] / np.broadcast_to(C0, C.shape)[want_guard]
    # ... leave C ~ -0.5 C0 after the step: -0.49 .. -0.41 for CO2 and N2O; CH4's 9-year pool relaxes (faster the smaller its
    # alpha) and takes up 100 ppb of emissions within the step: -0.38 .. -0.10.  All a hundred times the 1e-3 C0 above.
    assert np.all((ratio > -0.55) & (ratio < -0.1)), (ratio.min(), ratio.max())
    assert np.all(iirf[want_clamp] > 1.1 * imax)                                                      # WELL above
    # the inverse step reaches the shared targets: N2O's is negative, so every member's sqrt guard engages there
    Ci = sr.reference(kind, True)["C"][0]
    assert np.allclose(Ci, ens["target"][:, None], rtol=1e-12)
    # (e): the slow pool holds the excess, so the step's increment is ~1e-6 of the state
    slow = ens["cls"] == sr.SLOW
    assert np.all(ens["R0"][0, slow] > 0.99 * ens["R0"][:4, slow].sum(0))
    # every per-member input is an fp32 number, every emission a multiple of 2^-10
    for x in (ens["R0"], ens["S0"], *(ens["params"][k] for k in ("r0", "rC", "rT", "q"))):
        assert np.array_equal(x, x.astype(np.float32).astype(np.float64))
    assert np.array_equal(ens["E"] * 1024, np.round(ens["E"] * 1024)) and np.all(sr.cum_before(ens) != 0)


def test_the_layout_puts_every_pair_of_classes_in_one_packed_lane_and_mixes_every_group():
    for N in (200, 201):
        cls = sr.member_classes(N)
        assert np.array_equal(cls, sr.member_classes()[:N])
        lanes = {(int(a), int(b)) for a, b in zip(cls[0:N - 1:2], cls[1:N:2])}
        assert lanes == {(a, b) for a in range(5) for b in range(5)}
        edge = np.isin(cls, (sr.GUARDED, sr.CLAMPED, sr.BOTH))
        for width in (4, 8):                                           # quads and octets of members: never of one class; an
            groups = [slice(m0, m0 + width) for m0 in range(0, N - width + 1, width)]     # octet never without an out-of-domain
            assert all(len(set(cls[g])) > 1 for g in groups), (N, width)                  # member nor without an in-domain one,
            mixed = [edge[g].any() and not edge[g].all() for g in groups]                 # seven quads in ten likewise
            assert all(mixed) if width == 8 else np.mean(mixed) >= 0.7, (N, width, np.mean(mixed))
        for b in (64, 128):                                            # the statistics records' boundaries
            assert cls[b - 1] != cls[b] and (edge[b - 1] or edge[b]), (N, b)
        assert edge[0] and edge[N - 1] or N == 200
    assert sr.member_classes(201)[200] == sr.GUARDED                   # alone in the last packed lane of 201
    # every (class, gas) combination of the guarded and of the clamped gas occurs in both slots of a packed lane
    ens = sr.edge_ensemble("multigas")
    for slot in (0, 1):
        sel = np.arange(sr.N_MAX) % 2 == slot
        for c in (sr.GUARDED, sr.BOTH):
            assert set(ens["guard_gas"][sel & (ens["cls"] == c)]) == {0, 1, 2}
        for c in (sr.CLAMPED, sr.BOTH):
            assert set(ens["clamp_gas"][sel & (ens["cls"] == c)]) == {0, 1, 2}
    both = ens["cls"] == sr.BOTH
    assert (ens["guard_gas"][both] == ens["clamp_gas"][both]).any() and (ens["guard_gas"][both] != ens["clamp_gas"][both]).any()
