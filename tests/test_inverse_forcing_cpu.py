"""Concentration-driven runs with forcing scales and the in-loop misfit (include/fiveeq.h, fiveeq_run_inverse_forc_*), the parts
that need no GPU: the new symbols and their host-side validation in the order they report, the references of
tests/inverse_forcing_reference.py against each other and against the 50-digit step (K: the yardstick of
tests/test_inverse_forcing_gpu.py), and the proof that the yardstick sees a scale in the wrong place."""
import ctypes

import numpy as np
import pytest

import inverse_forcing_reference as fr
import step_reference as sr
from fiveeqscm_amd import _capi
from fiveeqscm_amd import params as prm

# The restatement's worst anchored-step error over the 12 steps x 16 members of each case, in units of eps64 x scale (printed by
# test_the_restatement_agrees_with_the_50_digit_step_at_every_step, which holds the figures to these constants).  E, cum and R
# keep the size of the step without scales (tests/test_inverse_cpu.py: the gas step does not see the scales, only the state it
# starts from differs); T and S of the CO2-only set fall from 3.8 to 1.8 because the category terms widen the scale that
# f1 ln(C / C0) alone made narrow.
K = {
    "{4}": {"E": 0.05, "T": 0.95, "R": 0.90, "S": 0.90, "cum": 0.05},              # measured 0.014 0.945 0.897 0.876 0.013
    "4+1+1": {"E": 0.15, "T": 0.65, "R": 1.20, "S": 0.65, "cum": 0.15},            # measured 0.102 0.642 1.162 0.612 0.100
    "multigas dt=0.5": {"E": 0.10, "T": 0.50, "R": 1.50, "S": 0.55, "cum": 0.10},  # measured 0.051 0.460 1.491 0.516 0.050
    "co2 dt=1": {"E": 0.05, "T": 1.75, "R": 1.50, "S": 1.85, "cum": 0.05},         # measured 0.009 1.743 1.450 1.842 0.009
}
BOUND = 8.0            # the single-step bound's factor (tests/test_step_edges_gpu.py): |got - ref| <= 8 max(K, 1) eps scale


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = _capi.load()
    assert hasattr(lib, "fiveeq_run_inverse_forc_f64") and hasattr(lib, "fiveeq_run_inverse_forc_f32")
    for sfx in ("f64", "f32"):
        name = "fiveeq_run_inverse_forc_" + sfx
        assert name in _capi.SIGNATURES
        # the arguments of fiveeq_run_inverse_*, then fscale, fext, n_fext, obs, misfit before stream
        inv = _capi.SIGNATURES["fiveeq_run_inverse_" + sfx][1]
        assert _capi.SIGNATURES[name][1] == inv[:-1] + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                                         ctypes.c_void_p] + inv[-1:]
    assert lib.fiveeq_abi_version() == 13 and lib.fiveeq_sizeof_model() == 448      # additive: nothing existing changed


def _call(lib, sfx, n_gas=3, n=8, ld=8, n_steps=4, t0=0, t1=4, ptr=0x1000, cumE=0x1800, fscale=0x2000, fext=0x3000, n_fext=2,
          obs=0x4000, misfit=0x5000):
    model = prm.make_model(prm.default_params("multigas"))
    model.n_gas = n_gas                              # 2: pools 4 + 1, a compiled layout with neither the forcing nor the misfit form
    p, vp = ctypes.c_void_p(ptr), ctypes.c_void_p
    rc = getattr(lib, "fiveeq_run_inverse_forc_" + sfx)(ctypes.byref(model), n, ld, p, n_steps, t0, t1, p, p, p, p, vp(cumE), None,
                                                        None, 0, None, vp(fscale), vp(fext), n_fext, vp(obs), vp(misfit), None)
    return rc, lib.fiveeq_last_error().decode()


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_the_refusals_come_in_the_order_of_the_forward_families(sfx):
    """Every call is refused on the host with FIVEEQ_E_INVALID: the (fake) pointers are never dereferenced and nothing is
    launched, so this runs without a GPU.  The list starts with EVERY argument wrong and mends the one just reported: the order of
    the messages is the order of the checks — base arguments, cumE, the forcing rows, obs and misfit together, the misfit rows."""
    lib = _capi.load()
    wrong = dict(n=0, cumE=0, n_fext=5, fscale=0, fext=0, n_gas=2, obs=0, misfit=0x5004)
    steps = [
        ("n_members", dict(n=8)),                                    # the base arguments (make_args)
        ("cumE is NULL", dict(cumE=0x1800)),
        ("n_fext=5 outside 0..4", dict(n_fext=2)),                   # check_forcing, in its own order
        ("fscale is NULL", dict(fscale=0x2001)),
        ("fscale must be", dict(fscale=0x2000)),
        ("fext is NULL with n_fext=2", dict(fext=0x3001)),
        ("fext must be", dict(fext=0x3000)),
        ("has no forcing form", dict(fscale=0, n_fext=0)),           # (the 4 + 1 layout stays: the misfit has no form for it either)
        ("obs and misfit go together", dict(obs=0x4000)),
        ("8-byte aligned", dict(misfit=0x5000)),
        ("has no misfit form", dict(n_gas=3)),
    ]
    for needle, mend in steps:
        rc, msg = _call(lib, sfx, t0=1, t1=1, **wrong)
        assert rc == _capi.E_INVALID and needle in msg, (needle, rc, msg)
        wrong.update(mend)
    # mended: valid arguments and an EMPTY step range — accepted, and nothing to launch (with scales, with the misfit, with neither)
    for kw in (wrong, dict(wrong, fscale=0x2000, fext=0x3000, n_fext=3), dict(wrong, obs=0, misfit=0),
               dict(wrong, fscale=0x2000, n_fext=0, fext=0)):
        rc, msg = _call(lib, sfx, t0=1, t1=1, **kw)
        assert rc == _capi.OK, (kw, msg)
    # the base arguments as fiveeq_run_inverse_* reports them, whatever the rest
    for kw, needle in ((dict(ld=4), "ld="), (dict(ptr=0), "NULL device pointer"), (dict(t0=3, t1=2), "step range"),
                       (dict(t1=5), "step range")):
        rc, msg = _call(lib, sfx, **dict(dict(cumE=0, n_fext=9), **kw))
        assert rc == _capi.E_INVALID and needle in msg, (kw, msg)
    rc, msg = _call(lib, sfx, fscale=0, n_fext=1, t0=1, t1=1)         # a count without rows
    assert rc == _capi.E_INVALID and "fscale is NULL" in msg, msg


# ---- the references ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fr.CASES)
def test_the_inputs_meet_their_conditions(name):
    """Gas scales in 0.75 .. 1.25, category scales in 0.25 .. 2, all multiples of 2^-6 and none equal to 1; a member's gas scales
    pairwise different; K = 3 categories with entries on the 2^-10 grid, all fp32-exact; the table of a longer run starts with the
    shorter one's; every category takes non-zero values and the table is not of one sign; the tiling carries the scale rows."""
    c = fr.case(name)
    f32_exact = lambda x: np.array_equal(x, np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64))   # noqa: E731
    sg, sx, X = c["sg"], c["sx"], c["X"]
    assert sg.shape == (c["n_gas"], fr.M) and sx.shape == (fr.K_CAT, fr.M) == (3, 16) and X.shape == (fr.N_STEPS, 3)
    assert sg.min() >= 0.75 and sg.max() <= 1.25 and sx.min() >= 0.25 and sx.max() <= 2.0
    for s in (sg, sx):
        assert np.array_equal(s * 64, np.round(s * 64)) and np.all(s != 1.0) and f32_exact(s)
    assert all(np.all(sg[g] != sg[h]) for g in range(c["n_gas"]) for h in range(g))
    assert np.array_equal(X * 1024, np.round(X * 1024)) and f32_exact(X) and np.abs(X).max() < 4.0
    assert np.all((X != 0).any(axis=0)) and X.min() < 0 < X.max()
    long = fr.case(name, 130)
    assert np.array_equal(long["X"][:fr.N_STEPS], X) and np.array_equal(long["target"][:fr.N_STEPS], c["target"])
    assert long["X"].shape == (130, 3) and f32_exact(long["X"])
    p = fr.tiled_params(c, 323)
    assert all(np.array_equal(p[k][:, i], row[:, i % fr.M]) for k, row in (("f_scale", sg), ("fx_scale", sx)) for i in (0, 16, 17, 322))


@pytest.mark.parametrize("name", fr.CASES)
def test_the_restatement_against_the_oracle_run_member_by_member(name):
    """For each member the oracle's run_inverse runs alone with f[g] multiplied by the member's gas scale and F_ext + X @ sx as
    its external forcing: no step code shared with the restatement.  E, T and the final R, S and cumE within a hundredth of
    |a - b| <= 1e-10 |b| + 1e-13, the margin tests/test_forcing_gpu.py::test_fp64_against_the_oracle_run_member_by_member holds the
    forward restatement to.  130 steps: the run the GPU test compares."""
    n_steps = 130
    want, got = fr.oracle_run(name, n_steps), fr.restated_run(fr.case(name, n_steps))
    assert int((np.sign(want["T"][1:]) != np.sign(want["T"][:-1])).sum()) > 0        # T goes through zero: the absolute term is used
    for k in ("E", "T", "R", "S", "cum"):
        err = np.abs(got[k] - want[k]) / (1e-10 * np.abs(want[k]) + 1e-13)
        print(f"{name} {k}: worst err / bound {err.max():.3g}")
        assert np.isfinite(got[k]).all() and err.max() <= 1e-2, (name, k, float(err.max()))


@pytest.mark.parametrize("name", fr.CASES)
def test_the_restatement_agrees_with_the_50_digit_step_at_every_step(name):
    """The restatement, one step at a time from its own state, against the 50-digit step of each member's own model from that
    state; worst units of eps64 x scale over 12 steps x 16 members (the recorded constants K must cover them and not exceed them by
    more than a unit).  Measured 2026-10-20:

        case               E      T      R      S      cum
        {4}               0.014  0.945  0.897  0.876  0.013
        4+1+1             0.102  0.642  1.162  0.612  0.100
        multigas dt=0.5   0.051  0.460  1.491  0.516  0.050
        co2 dt=1          0.009  1.743  1.450  1.842  0.009
    """
    worst, _ = fr.restated_anchored(name)
    print(f"K[{name!r}] =", {k: round(v, 3) for k, v in worst.items()})
    for out, v in worst.items():
        assert v <= 4.0, (name, out, v)             # two fp64 programs of ~10 roundings per output: a few units, or one is wrong
        assert v <= K[name][out] <= v + 1.0, (name, out, v, K[name][out])


def test_unit_scales_and_a_zero_table_are_the_step_without_scales():
    """The references themselves: with sg = 1 and X = 0 the restatement gives the bits of inverse_reference.restated_step (the
    oracle's step) and the 50-digit step is inverse_reference.step_reference, scales included."""
    import inverse_reference as ir
    for name in ("multigas dt=0.5", "co2 dt=1"):
        c = dict(fr.case(name))
        c["sg"], c["sx"], c["X"] = np.ones_like(c["sg"]), c["sx"], np.zeros_like(c["X"])
        rng = np.random.default_rng(5)
        R, S = rng.uniform(1.0, 30.0, (sum(c["pools"]), fr.M)), rng.uniform(0.1, 0.9, (2, fr.M))
        cum = rng.uniform(-5.0, 40.0, (c["n_gas"], fr.M))
        got, want = fr.restated_step(c, R, S, cum, 5), ir.restated_step(ir.case(name), R, S, cum, 5)
        for k in fr.OUTPUTS:
            assert np.array_equal(got[k], want[k]), (name, k)
        a, b = fr.step_reference(c, R, S, cum, 5), ir.step_reference(ir.case(name), R, S, cum, 5)
        for k in a:
            same = (all(np.array_equal(x, y) for x, y in zip(a[k], b[k])) if isinstance(a[k], tuple) else np.array_equal(a[k], b[k]))
            assert same, (name, k)


@pytest.mark.parametrize("variant,out", list(zip(fr.VARIANTS, ("T", "T", "E"))))
@pytest.mark.parametrize("name", ["multigas dt=0.5", "4+1+1"])
def test_the_yardstick_sees_a_scale_in_the_wrong_place(name, variant, out):
    """A gas's forcing scaled by its neighbour's factor; F_ext multiplied by a category's factor; the gas factors multiplied into
    T_old and left off F.  The anchored comparison the restatement passes with figures near 1 misses the bound
    BOUND max(K, 1) of the output each mistake is made in — T for the first two, E (through the feedback's T_old) for the third —
    by more than a thousand times in units of eps64, and is still missed in units of eps32, the coarser yardstick of the GPU
    tests (every ratio is printed)."""
    c = fr.case(name)
    assert c["n_gas"] == 3
    for prec in ("f64", "f32"):
        worst, _ = fr.anchored(c, lambda *a: fr.restated_step(*a, variant=variant), eps=sr.EPS[prec])
        ratio = {o: worst[o] / (BOUND * max(K[name][o], 1.0)) for o in fr.OUTPUTS}
        print(f"{name}, {variant}, {prec}: worst / bound", {o: float(f"{v:.3g}") for o, v in ratio.items()})
        assert ratio[out] > (1e3 if prec == "f64" else 1.0), (name, variant, prec, ratio)
