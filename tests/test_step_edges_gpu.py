"""The model step's two data-dependent decisions — the C <= 0 guard and the iIRF clamp — and the isolation of a non-finite
member, in every kernel form, on the edge ensemble of tests/step_reference.py: members of five classes ((a) in-domain,
(b) a gas at C ~ -0.5 C0, (c) iIRF far past iirf_max, (d) both, (e) in-domain with the slow pool dominant) laid out so that
every ordered pair of classes shares a packed lane and every quad, octet and statistics-record boundary is mixed; pools
4 + 1 + 1 (CO2 carries the log term, CH4 / N2O the sqrt term) and {4} (the quad kernel); 200 and 201 members.

ACCURACY: one step from the prescribed state, run(T0, T0 + 1), against the guarded 50-digit step, per output and per member,
nobody excluded:  |got - ref| <= 8 max(K_ORACLE, 1) eps(dtype) scale  (K_ORACLE: tests/test_step_edges_cpu.py; the 8: the
device primitives' 2 ulp (2.5 for the fp32 log) against libm's <= 1, the host's pre-rounded folded constants, the FMAs'
other association), never more than the project's own tolerances.

MEASURED (MI355X): at most 1.5 eps x scale in every form, class and output — the table is in the docstring of
test_one_step_against_the_50_digit_reference.

ONE ARITHMETIC: every other launch shape and feature carrier gives the bits of the matching accuracy run, for that step and
for four more (decisions then flip on state the kernels produced themselves).

ISOLATION: a member whose pools are NaN leaves every other member's bits and every other statistics record alone; its own
record has NaN sums and the extrema of its finite members — the same words by the DPP ladder (per-step), the flush's
full-wave and partial-wave paths (fused, small), packed or not; a record of NaN members only has min = +inf, max = -inf by
every route.
"""
import functools

import numpy as np
import pytest

import step_reference as sr
from test_step_edges_cpu import K_ORACLE

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

T0, N_STEPS = sr.T0, sr.N_STEPS
BOUND = 8.0
# the project's own tolerances (tests/test_engine_gpu.py): the bound never exceeds them
PROJECT_TOL = {("f64", "C"): (1e-10, 1e-13), ("f64", "T"): (1e-10, 1e-13), ("f64", "E"): (1e-8, 1e-9),
               ("f32", "C"): (5e-6, 2e-4), ("f32", "T"): (3e-5, 2e-6)}
KINDS = ("multigas", "co2")


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from fiveeqscm_amd import _capi
    return _capi.load()                       # the HIP library must be the thing that runs: no fallback


class _Packing:
    """fiveeq_set_f32_packing for the block, restored on exit."""

    def __init__(self, lib, on):
        self.lib, self.on = lib, int(on)

    def __enter__(self):
        self.lib.fiveeq_set_f32_packing(self.on)

    def __exit__(self, *exc):
        self.lib.fiveeq_set_f32_packing(1)


def _engine(kind, N, *, R0=None, inverse=False, scenarios=0, **kw):
    from fiveeqscm_amd.engine import EnsembleEngine
    ens = sr.edge_ensemble(kind)
    E = np.repeat(ens["target"][None, :], N_STEPS, axis=0) if inverse else ens["E"]
    if scenarios:
        E = np.stack([E] * scenarios)
    eng = EnsembleEngine(sr.member_params(ens, N), N, E, F_ext=ens["F_ext"], R0=ens["R0"][:, :N] if R0 is None else R0,
                         S0=ens["S0"][:, :N], concentration_driven=inverse, device="cuda:0", **kw)
    if inverse:                                   # the member's own cumulative emissions before the step: the forward run's
        eng.cumE.copy_(torch.from_numpy(np.repeat(sr.cum_before(ens)[:, None], N, axis=1)).to(eng.cumE.dtype))
    return eng


def _rows(eng, t0, t1, scenario=None):
    """C, T of steps [t0, t1) and the state R, S as host arrays (of scenario `scenario` of an engine with that axis)."""
    torch.cuda.synchronize()
    pick = (lambda x: x) if scenario is None else (lambda x: x[scenario])
    return {"C": pick(eng.C)[t0:t1].cpu().numpy(), "T": pick(eng.T)[t0:t1].cpu().numpy(),
            "R": pick(eng.R).cpu().numpy(), "S": pick(eng.S).cpu().numpy()}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    word = {8: np.int64, 4: np.int32}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(word), b.view(word))


# ---- accuracy -----------------------------------------------------------------------------------------------------------------
ACCURACY_FORMS = {
    "f64 per-step": dict(prec="f64", kw=dict(dtype=torch.float64), mode="per_step", packing=1),
    "f32 per-step, packing off": dict(prec="f32", kw=dict(dtype=torch.float32), mode="per_step", packing=0),
    "f32 compensated fused": dict(prec="f32", kw=dict(dtype=torch.float32, compensated=True), mode="fused", packing=1),
    "f64 inverse per-step": dict(prec="f64", kw=dict(dtype=torch.float64), mode="per_step", packing=1, inverse=True),
    "f32 inverse per-step": dict(prec="f32", kw=dict(dtype=torch.float32), mode="per_step", packing=1, inverse=True),
}


def _accuracy_run(lib, kind, N, form):
    f = ACCURACY_FORMS[form]
    with _Packing(lib, f["packing"]):
        eng = _engine(kind, N, inverse=f.get("inverse", False), **f["kw"])
        eng.run(T0, T0 + 1, mode=f["mode"])
        out = _rows(eng, T0, T0 + 1)
        if f.get("inverse"):
            out["E"] = out.pop("C")                      # the inverse form stores the diagnosed E in the C rows
        eng.close()
    return out


@pytest.mark.parametrize("form", list(ACCURACY_FORMS))
@pytest.mark.parametrize("N", [200, 201])
@pytest.mark.parametrize("kind", KINDS)
def test_one_step_against_the_50_digit_reference(lib, kind, N, form):
    """Worst multiples of eps(dtype) x scale measured on the MI355X, 2026-10-18 (bound: 8; N = 200 and 201 agree):

        form                         layout    C      T      R      S      E
        f64 per-step                 4+1+1   0.557  0.584  0.629  0.542
                                     {4}     0.606  0.836  0.664  0.918
        f32 per-step, packing off    4+1+1   0.546  0.459  0.681  0.438
                                     {4}     0.575  0.779  0.563  1.063
        f32 compensated fused        4+1+1   0.546  0.459  0.681  0.438
                                     {4}     0.575  0.697  0.682  0.503
        f64 inverse per-step         4+1+1          0.501  0.668  0.444  0.513
                                     {4}            0.980  0.844  1.234  0.106
        f32 inverse per-step         4+1+1          0.523  0.652  0.567  0.463
                                     {4}            0.933  0.845  1.491  0.108

    No class stands out (the worst figure of a class is between 0.3 and 1.5 everywhere, but for E of the {4} inverse forms:
    0.02 to 0.11): a single step from exact inputs is dominated by the last rounding of each output, and the bound of 8 is
    not approached.  The test prints every figure, per class."""
    f = ACCURACY_FORMS[form]
    prec, inverse = f["prec"], bool(f.get("inverse"))
    eps = sr.EPS[prec]
    ref = sr.reference(kind, inverse)
    got = _accuracy_run(lib, kind, N, form)
    cls = sr.edge_ensemble(kind)["cls"][:N]
    yard = {"C": "C", "R": "C", "T": "T", "S": "T", "E": "E"}      # the state rows take their output's yardstick
    worst, failures = {}, []
    for name, rows in got.items():
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, N)
        assert np.all(np.isfinite(rows)), (form, name)
        units = sr.err_units(rows, ref, name, eps)
        limit = np.full_like(units, BOUND * max(K_ORACLE[kind][yard[name]], 1.0))
        if (prec, name) in PROJECT_TOL:                              # ... and never past the project's tolerance
            rtol, atol = PROJECT_TOL[(prec, name)]
            limit = np.minimum(limit, (rtol * np.abs(ref[name][0][:, :N]) + atol) / (eps * sr.scale_of(ref, name, eps)[:, :N]))
        worst[name] = float(units.max())
        by_class = [float(units[:, cls == c].max()) for c in range(5)]
        print(f"{kind} N={N} {form}: {name} worst {worst[name]:.3f} x eps x scale; by class (a..e) "
              + " ".join(f"{v:.3f}" for v in by_class))
        if np.any(units > limit):
            row, m = np.unravel_index(np.argmax(units / limit), units.shape)
            failures.append((name, int(row), int(m), sr.CLASSES[cls[m]], float(units[row, m]), float(limit[row, m])))
    assert not failures, (kind, N, form, failures)


# ---- one arithmetic -----------------------------------------------------------------------------------------------------------
def _shapes(kind):
    """(label, engine keywords, run keywords) of every launch shape and feature carrier of the plain step."""
    from fiveeqscm_amd.constrain import Observations
    from fiveeqscm_amd.forcing import ExternalForcings
    wide = 8 if kind == "multigas" else 4
    obs = Observations(np.stack([np.full(N_STEPS, 0.5), np.full(N_STEPS, 4.0), np.full(N_STEPS, 1.0 / N_STEPS),
                                 np.zeros(N_STEPS)], axis=1))
    none = ExternalForcings(np.zeros((N_STEPS, 0)))
    out = [("fused", {}, dict(mode="fused")), ("ksteps k=1", {}, dict(mode="ksteps", k_steps=1)), ("graph", {}, dict(mode="graph")),
           ("small, 1 lane", dict(small_lanes=1), dict(mode="small")),
           (f"small, {wide} lanes", dict(small_lanes=wide), dict(mode="small"))]
    for mode in ("per_step", "fused"):
        out += [(f"2 scenarios, {mode}", dict(scenarios=2), dict(mode=mode)),
                (f"forcing= unit scales, K=0, {mode}", dict(forcing=none), dict(mode=mode)),
                (f"observations= {mode}", dict(observations=obs), dict(mode=mode))]
    return out


def _two_segments(eng, run, scenarios=(None,)):
    """The step under test, then four more: per scenario, the rows of each segment and the state after it."""
    run(T0, T0 + 1)
    first = [_rows(eng, T0, T0 + 1, s) for s in scenarios]
    run(T0 + 1, T0 + 5)
    return list(zip(first, [_rows(eng, T0, T0 + 5, s) for s in scenarios]))


def _assert_same(got, want, what):
    for seg, (g, w) in enumerate(zip(got, want)):
        for name in ("C", "T", "R", "S"):
            assert _same_bits(g[name], w[name]), (*what, "one step" if seg == 0 else "five steps", name)


def _scalar_per_step(lib, kind, N, dtype):
    with _Packing(lib, 0):
        ref = _engine(kind, N, dtype=dtype)
        want = _two_segments(ref, lambda a, b: ref.run(a, b, mode="per_step"))[0]
        ref.close()
    assert np.isfinite(want[1]["T"]).all() and np.isfinite(want[1]["C"]).all()
    return want


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("N", [200, 201])
@pytest.mark.parametrize("kind", KINDS)
def test_every_shape_gives_the_bits_of_the_per_step_run(lib, kind, N, prec):
    """fused, ksteps (k = 1), graph, small with 1 and 4 / 8 lanes, a 2-scenario engine, forcing= with unit scales and K = 0,
    observations= — bit for bit the per-step run's C, T, R and S, for the step under test and after four more.  In fp32
    every shape runs PACKED where it has a packed form (even row strides: N = 200) and is held to the SCALAR per-step run
    (packing off): a packed lane whose two members disagree about the guard or the clamp must give each its own branch."""
    dtype = torch.float64 if prec == "f64" else torch.float32
    want = _scalar_per_step(lib, kind, N, dtype)
    shapes = _shapes(kind) + ([("packed per-step", {}, dict(mode="per_step"))] if prec == "f32" else [])
    for label, eng_kw, run_kw in shapes:
        eng = _engine(kind, N, dtype=dtype, **eng_kw)
        scenarios = tuple(range(eng_kw["scenarios"])) if "scenarios" in eng_kw else (None,)
        for s, got in zip(scenarios, _two_segments(eng, lambda a, b: eng.run(a, b, **run_kw), scenarios)):
            _assert_same(got, want, (kind, N, prec, label, s))
        eng.close()


@pytest.mark.parametrize("kind", KINDS)
def test_the_half_filled_last_packed_lane(lib, kind):
    """201 members of a 202-member allocation (even row strides, so the fp32 entry points take the packed kernels): the last
    packed lane holds a guarded member alone.  Members 0 .. 200 get the bits of the scalar 201-member run, per-step and
    fused; member 201's rows are not touched."""
    want = _scalar_per_step(lib, kind, 201, torch.float32)
    for fn_name in ("fiveeq_run_f32", "fiveeq_run_fused_f32"):
        eng = _engine(kind, 202, dtype=torch.float32)
        before = _rows(eng, T0, T0 + 5)

        def run(a, b):
            rc = getattr(lib, fn_name)(*eng._run_args(a, b, 0, 201), eng._stream())
            assert rc == 0, lib.fiveeq_last_error()

        got = _two_segments(eng, run)[0]
        _assert_same([{k: v[..., :201] for k, v in seg.items()} for seg in got], want, (kind, fn_name))
        for name in ("C", "T", "R", "S"):
            assert _same_bits(got[1][name][..., 201], before[name][..., 201]), (kind, fn_name, name)
        eng.close()


@pytest.mark.parametrize("N", [200, 201])
@pytest.mark.parametrize("kind", KINDS)
def test_compensated_small_gives_the_bits_of_compensated_fused(lib, kind, N):
    """The compensated form's guarded branch (its own log1p and sumN / (sqrt C + sqrt C0) algebra, -sqrt C0 under the guard) in
    its two kernels: packed lanes in the fused kernel, one member per lane in the small one."""
    runs = []
    for mode in ("fused", "small"):
        eng = _engine(kind, N, dtype=torch.float32, compensated=True, small_lanes=1)
        runs.append(_two_segments(eng, lambda a, b: eng.run(a, b, mode=mode))[0])
        eng.close()
    assert np.isfinite(runs[0][1]["T"]).all()
    _assert_same(runs[1], runs[0], (kind, N, "compensated small"))


# ---- isolation of a non-finite member ------------------------------------------------------------------------------------------
N_ISO = 202                                       # three full records and a last one of 10 members; even: fp32 lanes pack
ISO_STEPS = (T0, T0 + 9)                          # the fused kernels flush their statistics after 8 steps, then a ragged rest
ISO_MEMBERS = [0, 10, 11, 20, 21, 23, 37, 63, 201]      # first; even / odd in a packed lane; lanes 0, mid, 3 of a quad; inside
                                                        # an octet; last of a record; last of all, in the partial record


def _iso_forms(kind):
    wide = 8 if kind == "multigas" else 4
    f64, f32 = torch.float64, torch.float32
    return {"f64 per-step": dict(kw=dict(dtype=f64), mode="per_step", packing=1, group="f64"),
            "f64 fused": dict(kw=dict(dtype=f64), mode="fused", packing=1, group="f64"),
            "f64 small, 1 lane": dict(kw=dict(dtype=f64, small_lanes=1), mode="small", packing=1, group="f64"),
            # (the octet form writes no statistics records: state and rows only)
            f"f64 small, {wide} lanes": dict(kw=dict(dtype=f64, small_lanes=wide), mode="small", packing=1, group="f64",
                                             stats=wide == 4),
            "f32 per-step, packing off": dict(kw=dict(dtype=f32), mode="per_step", packing=0, group="f32"),
            "f32 packed per-step": dict(kw=dict(dtype=f32), mode="per_step", packing=1, group="f32"),
            "f32 packed fused": dict(kw=dict(dtype=f32), mode="fused", packing=1, group="f32")}


def _iso_run(lib, kind, form, nan_members=()):
    f = _iso_forms(kind)[form]
    R0 = np.array(sr.edge_ensemble(kind)["R0"][:, :N_ISO])
    R0[:, list(nan_members)] = np.nan
    stats = f.get("stats", True)
    with _Packing(lib, f["packing"]):
        eng = _engine(kind, N_ISO, R0=R0, collect_stats=stats, **f["kw"])
        eng.run(*ISO_STEPS, mode=f["mode"])
        out = _rows(eng, *ISO_STEPS)
        out["stats"] = eng.T_stats[:, ISO_STEPS[0]:ISO_STEPS[1]].cpu().numpy() if stats else None      # [4 records, 9, 4]
        eng.close()
    return out


_healthy = functools.lru_cache(maxsize=None)(lambda lib, kind, form: _iso_run(lib, kind, form))


def _check_isolated(kind, form, got, want, nan_members):
    """Every other member and record as in the healthy run; returns the (min, max) words of the NaN members' records."""
    others = np.setdiff1d(np.arange(N_ISO), nan_members)
    for name in ("C", "T", "R", "S"):
        assert _same_bits(got[name][..., others], want[name][..., others]), (kind, form, name)
        assert np.isnan(got[name][..., nan_members]).all(), (kind, form, name)      # (and the member itself stays NaN)
    if got["stats"] is None:
        return None
    recs = sorted({m // 64 for m in nan_members})
    rest = [r for r in range(got["stats"].shape[0]) if r not in recs]
    assert _same_bits(got["stats"][rest], want["stats"][rest]), (kind, form, "records")
    T = got["T"].astype(np.float64)
    for r in recs:
        sums, lo, hi = got["stats"][r, :, :2], got["stats"][r, :, 2], got["stats"][r, :, 3]
        assert np.isnan(sums).all(), (kind, form, r)
        mine = T[:, 64 * r:64 * (r + 1)]
        finite = np.where(np.isnan(mine), np.inf, mine).min(1), np.where(np.isnan(mine), -np.inf, mine).max(1)
        assert np.array_equal(lo, finite[0]) and np.array_equal(hi, finite[1]), (kind, form, r, lo, finite[0])
    return got["stats"][recs][:, :, 2:]


@pytest.mark.parametrize("k", ISO_MEMBERS)
@pytest.mark.parametrize("kind", KINDS)
def test_a_nan_member_touches_neither_its_neighbours_nor_their_records(lib, kind, k):
    words = {}
    for form, f in _iso_forms(kind).items():
        got = _iso_run(lib, kind, form, (k,))
        w = _check_isolated(kind, form, got, _healthy(lib, kind, form), [k])
        if w is not None:
            words.setdefault(f["group"], []).append((form, w))
    for group, runs in words.items():             # the DPP ladder, the flush's full- and partial-wave paths, packed or not
        assert len(runs) >= 3
        for form, w in runs[1:]:
            assert _same_bits(w, runs[0][1]), (kind, k, group, form, "against", runs[0][0])


@pytest.mark.parametrize("kind", KINDS)
def test_a_record_of_nan_members_only_has_the_neutral_extrema_by_every_route(lib, kind):
    """Members 64 .. 127 (a full record: the flush's full-wave path, in the packed kernels the second half of a full wave) and
    192 .. 201 (the partial last record) all NaN: sums NaN, min = +inf, max = -inf by the DPP ladder and by both paths of the
    flush alike (the full-wave path started its folds from the first value and gave NaN extrema), everything else untouched."""
    nan_members = list(range(64, 128)) + list(range(192, N_ISO))
    for form in _iso_forms(kind):
        got = _iso_run(lib, kind, form, nan_members)
        w = _check_isolated(kind, form, got, _healthy(lib, kind, form), nan_members)
        if w is not None:
            assert np.all(w[..., 0] == np.inf) and np.all(w[..., 1] == -np.inf), (kind, form, w[:, 0])
