"""Carbon rows on the MI355X (include/fiveeq.h, "CARBON ROWS"; fiveeqscm_amd/carbon.py): the outputs against the NumPy twin bit
for bit (alpha within the bound of fe_exp), the cumulative emissions of concentration-driven runs against the engine's own
cumE with zero tolerance, alpha against the oracle's, the invariances (split of the rows and of the members over calls, element
accesses, the order of `want`, the launch form), the guards, a planted NaN, the scenario axis and the rows downstream.

Shapes are named by the kernel's edges: with tile = fiveeq_carbon_rows_tile(elem), N in {1, lane - 1, tile - 1, tile, tile + 1,
2 tile + 3}; with UN the rows in flight of each kernel form and Y the rows per workgroup of the row-parallel form, K in
{1, UN - 1, UN, UN + 1, Y - 1, Y + 1, FIVEEQ_BLOCK + 1} (the last crosses the LDS chunk of shared records).  Rows as an engine
lays them out (row stride N) and embedded in 16-byte aligned rows (16-byte accesses with a ragged tail)."""
import functools
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import carbon_reference as cref  # noqa: E402
from fiveeqscm_amd import _capi, _carbon_host as twin  # noqa: E402
from fiveeqscm_amd import carbon, constrain, emissions, params  # noqa: E402
from fiveeqscm_amd.distributed import gather_summary  # noqa: E402
from oracle import fiveeq_oracle as npo  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = {"f64": torch.float64, "f32": torch.float32}
NP = {"f64": np.float64, "f32": np.float32}
ALL = twin.WANT
# fp32 alpha of the golden members' run against the fp64 twin evaluated on the widened fp32 stored rows: the worst relative
# difference MEASURED on the MI355X, recorded in profiles/r28/NOTES.md; the test allows 4 times that (headroom for other members).
FP32_ALPHA_MEASURED = 4.9572e-07     # the 24 golden multigas members, 60 steps, per-step kernel
FP32_ALPHA_BOUND = 4.0 * FP32_ALPHA_MEASURED


def _edges(sfx):
    lib = _capi.load()
    elem = 8 if sfx == "f64" else 4
    tile, lane = lib.fiveeq_carbon_rows_tile(elem), 16 // elem
    un = sorted({lib.fiveeq_carbon_rows_unroll(w, s) for w in (0, 1) for s in (0, 1)})
    Y, block = lib.fiveeq_carbon_rows_yrows(), lib.fiveeq_joint_tile(7)
    Ns = sorted({1, lane - 1, tile - 1, tile, tile + 1, 2 * tile + 3} - {0})
    Ks = sorted({1, Y - 1, Y + 1, block + 1} | {u + d for u in un for d in (-1, 0, 1)} - {0})
    return tile, lane, Ns, [k for k in Ks if k >= 1], block


def _embed(a, dtype, ld=None, offset=0):
    """Host array [.., N] as a device view: as an engine lays it out (ld None), or as columns [offset, offset + N) of rows of
    stride ld filled with NaN elsewhere."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", dtype)
    if ld is None:
        return t
    buf = torch.full(tuple(t.shape[:-1]) + (ld,), float("nan"), dtype=dtype, device="cuda:0")
    view = buf[..., offset:offset + t.shape[-1]]
    view.copy_(t)
    return view


def _aligned(N):
    return (N + 3) // 4 * 4 + 4


def _dev(case, sfx, want, ld=None, offset=0, rows=slice(None), members=slice(None), **kw):
    """carbon.carbon_rows on (a row / member range of) a synthetic case."""
    dt = DTYPES[sfx]
    put = lambda a: _embed(a, dt, ld, offset)[..., members]                          # noqa: E731
    return carbon.carbon_rows(put(case["rows"])[rows], case["steps"][rows], case["params"], r=put(case["r"]), drive=case["drive"],
                              dt=case["dt"], T_rows=put(case["T"])[rows], concentration_gases=case["conc"], want=want, **kw)


def _same(a, b):
    """torch.equal with NaN equal to NaN."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _np(t):
    return t.cpu().numpy()


# ---- 1. bits against the twin -------------------------------------------------------------------------------------------------
def _against_twin(sfx, G, conc, K, N, layouts):
    case = cref.synthetic(G, K, N, NP[sfx], conc)
    ref = cref.host(case, ALL)
    for ld in layouts:
        res = _dev(case, sfx, ALL, ld=ld)
        for w in ("airborne", "cumE", "uptake", "fraction", "sink", "iirf"):
            assert np.array_equal(_np(getattr(res, w)), ref[w], equal_nan=True), (w, K, N, ld)
        excess = cref.alpha_excess(_np(res.alpha), _np(res.iirf), case["params"], range(G), case["dt"], NP[sfx])
        assert excess <= 1.0, ("alpha", K, N, ld, excess)
        if conc:
            assert np.array_equal(_np(res.cum_end), ref["cum_end"])
        assert np.array_equal(_np(res.airborne_end), ref["airborne_end"])
    return case


@pytest.mark.parametrize("conc", [False, True], ids=["emission", "driven"])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_every_member_edge_equals_the_twin_bit_for_bit(sfx, G, conc):
    """airborne, cumE, uptake, fraction, sink and iirf in bits, alpha within fe_exp's bound plus one ulp per product, at every N
    edge, for rows of stride N (16-byte accesses only where N allows them) and in aligned rows (16-byte launch + ragged tail)."""
    tile, lane, Ns, Ks, block = _edges(sfx)
    mask = () if not conc else (0,) if G == 1 else (1, 2)
    for N in Ns:
        _against_twin(sfx, G, mask, 3, N, (None, _aligned(N)))


@pytest.mark.parametrize("conc", [False, True], ids=["emission", "driven"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_every_row_edge_equals_the_twin_bit_for_bit(sfx, conc):
    tile, lane, Ns, Ks, block = _edges(sfx)
    for K in Ks:
        _against_twin(sfx, 3, (1, 2) if conc else (), K, lane + 1, (None, _aligned(lane + 1)))


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_the_row_parallel_form_equals_the_twin_at_every_row_edge(sfx):
    """Without sink and without a driven gas the rows are spread over grid.y: the same bits, at every K edge, and equal to the
    carried form of the same outputs (airborne0 = 0 asks for it)."""
    tile, lane, Ns, Ks, block = _edges(sfx)
    want = ("airborne", "cumE", "uptake", "fraction", "iirf", "alpha")
    for K in Ks:
        case = cref.synthetic(3, K, tile + 1, NP[sfx])
        par = _dev(case, sfx, want, ld=_aligned(tile + 1))
        seq = _dev(case, sfx, want, ld=_aligned(tile + 1), airborne0=torch.zeros((3, tile + 1), dtype=DTYPES[sfx], device="cuda:0"))
        assert par.sink is None and par.airborne_end is None and seq.airborne_end is not None
        for w in want:
            assert _same(getattr(par, w), getattr(seq, w)), (w, K)
        ref = cref.host(case, ("fraction", "uptake"), members=slice(0, 9))
        assert np.array_equal(_np(par.fraction[..., :9]), ref["fraction"]) and np.array_equal(_np(par.uptake[..., :9]), ref["uptake"])


# ---- 2. the proof for concentration-driven gases ------------------------------------------------------------------------------
def _pathway(kind, n_steps):
    base = params.default_params(kind)
    G = params.n_gas_of(base)
    E = emissions.rcp_like_emissions(n_steps, G)
    return base, G, E, npo.run(E, base, 1)["C"][:, :, 0]


@pytest.mark.parametrize("form", ["inverse-4", "inverse-411", "mixed-411"])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_cumE_of_the_last_row_is_the_engines_cumE(sfx, form):
    """Zero tolerance: the pass repeats the stepping kernel's own fma on the stored emissions."""
    from fiveeqscm_amd.engine import ConcentrationDrivenEngine, MixedDriveEngine
    tile = _edges(sfx)[0]
    N, n_steps = tile + 1, 40
    base, G, E, C = _pathway("co2" if form == "inverse-4" else "multigas", n_steps)
    p = params.sample_ensemble_shard(base, N)
    if form == "mixed-411":
        eng, driven = MixedDriveEngine(p, N, E, C, (1, 2), dtype=DTYPES[sfx], device="cuda:0"), [1, 2]
    else:
        eng, driven = ConcentrationDrivenEngine(p, N, C, dtype=DTYPES[sfx], device="cuda:0"), list(range(G))
    eng.run()
    torch.cuda.synchronize()
    res = eng.carbon_rows(want=("cumE",))
    assert res.cumE.shape == (n_steps, G, N)
    assert torch.equal(res.cumE[-1][driven], eng.cumE[driven]), form
    assert torch.equal(res.cum_end[driven], eng.cumE[driven])
    assert bool(torch.isfinite(eng.cumE[driven]).all()) and bool((eng.cumE[driven] != 0).any())
    if form == "mixed-411":                                    # the emission-driven gas reads the shared table
        table = torch.from_numpy(eng._cum_end[:, 0]).to("cuda:0", DTYPES[sfx])
        assert torch.equal(res.cumE[:, 0], table[:, None].expand(n_steps, N))
    only = eng.carbon_rows(want=("cumE", "fraction"), gases=driven[-1:])
    assert only.gases == (driven[-1],) and torch.equal(only.cumE[:, 0], res.cumE[:, driven[-1]])
    with pytest.raises(ValueError, match="need rows from step 0"):
        eng.carbon_rows(want=("cumE",), rows=slice(3, None))
    eng.close()


# ---- 3. against the run, forward ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden_run(sfx):
    from fiveeqscm_amd.engine import EnsembleEngine
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import fiveeq_cases as cases
    p, N = cases.members("multigas")
    E = cases.scenario("multigas")[:60]
    eng = EnsembleEngine(p, N, E, dtype=DTYPES[sfx], device="cuda:0")
    eng.run(mode="per_step")
    torch.cuda.synchronize()
    return eng, p, N, E


def test_alpha_of_a_forward_run_against_the_oracle_fp64():
    eng, p, N, E = _golden_run("f64")
    ref = npo.run(E, p, N, keep=("alpha",))["alpha"]
    got = _np(eng.carbon_rows(want=("alpha",)).alpha)
    err = np.abs(got[:-1] - ref[1:]) / np.abs(ref[1:])
    print("fp64 alpha of row t against the oracle's alpha[t + 1]: worst relative difference", err.max())
    assert err.max() <= 1e-10


def test_alpha_of_a_forward_run_fp32_against_the_fp64_twin_on_the_same_rows():
    """There is no bound to derive for fp32 rows: the measured worst difference is recorded in profiles/r28/NOTES.md and the
    test allows FP32_ALPHA_BOUND = 4 times it."""
    eng, p, N, E = _golden_run("f32")
    got = _np(eng.carbon_rows(want=("alpha",)).alpha).astype(np.float64)
    ref = twin.carbon_rows_host(_np(eng.C).astype(np.float64), eng.out_steps, p, r=_np(eng.r).astype(np.float64), drive=E, dt=1.0,
                                T_rows=_np(eng.T).astype(np.float64), want=("alpha",), cum_table=eng._cum_end)["alpha"]
    err = np.abs(got - ref) / np.abs(ref)
    print("fp32 alpha against the fp64 twin on the widened fp32 rows: worst relative difference", err.max())
    assert err.max() <= FP32_ALPHA_BOUND


# ---- 4. invariance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_no_bit_depends_on_how_rows_and_members_are_split(sfx):
    tile, lane, Ns, Ks, block = _edges(sfx)
    N, K = tile + 1, block + 3
    case = cref.synthetic(3, K, N, NP[sfx], (1, 2))
    ld = _aligned(N)
    whole = _dev(case, sfx, ALL, ld=ld)
    # the rows in two calls at every K edge, the state carried
    for k in Ks:
        a = _dev(case, sfx, ALL, ld=ld, rows=slice(0, k))
        b = _dev(case, sfx, ALL, ld=ld, rows=slice(k, K), cum0=a.cum_end, airborne0=a.airborne_end)
        for w in ALL:
            assert _same(torch.cat([getattr(a, w), getattr(b, w)]), getattr(whole, w)), (w, k)
        assert _same(b.cum_end[1:], whole.cum_end[1:]) and _same(b.airborne_end, whole.airborne_end), k
    # the members in two calls: at tile - 1 and at an odd column
    for cut in (tile - 1, 7):
        lo, hi = _dev(case, sfx, ALL, ld=ld, members=slice(0, cut)), _dev(case, sfx, ALL, ld=ld, members=slice(cut, N))
        for w in ALL:
            assert _same(torch.cat([getattr(lo, w), getattr(hi, w)], dim=-1), getattr(whole, w)), (w, cut)
    # element accesses forced by a one-element column offset; rows of stride N
    for kw in (dict(ld=ld + 4, offset=1), dict(ld=None)):
        other = _dev(case, sfx, ALL, **kw)
        for w in ALL:
            assert _same(getattr(other, w), getattr(whole, w)), (w, kw)
    # a permuted want, and a subset: what is not asked for stays None
    perm = _dev(case, sfx, ("sink", "alpha", "cumE", "fraction", "iirf", "uptake", "airborne"), ld=ld)
    for w in ALL:
        assert _same(getattr(perm, w), getattr(whole, w)), w
    few = _dev(case, sfx, ("alpha", "airborne"), ld=ld, gases=(0, 2))
    assert [w for w in ALL if getattr(few, w) is not None] == ["airborne", "alpha"] and few.gases == (0, 2)
    assert _same(few.alpha, whole.alpha[:, [0, 2]]) and _same(few.airborne, whole.airborne[:, [0, 2]])


# ---- 5. guards ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_guard_columns_and_guard_rows_keep_their_sentinel(sfx):
    """The C entry point on buffers of this test's own: columns [N, ld_out) of every output row and the rows before and after
    every output keep the sentinel, and so do columns [N, ld) of the carried state."""
    import ctypes

    from fiveeqscm_amd._rowargs import call, ptr, steps_i32
    tile = _edges(sfx)[0]
    dt, G, K, N = DTYPES[sfx], 3, 5, tile + 1
    ld = ld_out = _aligned(N)
    case = cref.synthetic(G, K, N, NP[sfx], (1, 2))
    SENT = -7777.0
    x, T, r = _embed(case["rows"], dt, ld), _embed(case["T"], dt, ld), _embed(case["r"], dt, ld)
    outs = [torch.full((K + 2, G, ld_out), SENT, dtype=dt, device="cuda:0") for _ in ALL]
    state = [torch.full((G, ld), SENT, dtype=dt, device="cuda:0") for _ in range(2)]
    for s in state:
        s[:, :N] = 0
    drive = torch.from_numpy(case["drive"]).to("cuda:0", dt)
    ce = np.zeros((case["drive"].shape[0], 3))
    ce[:, :G] = twin.cum_end_table(case["drive"][:, :G], 1.0)
    ce = torch.from_numpy(ce).to("cuda:0", dt)
    st = steps_i32(case["steps"].astype(np.int64), x.device)
    model = params.make_model(case["params"], 1.0)
    call(_capi.load(), _capi, "fiveeq_carbon_rows", dt, x.device, ctypes.byref(model), K, N, ld, ptr(x), G * ld, ld, ptr(T), ld, ptr(st),
         ptr(drive), ptr(ce), int(drive.shape[0]), ptr(r), 0b110, 0b111, *(ptr(o[1]) for o in outs), ld_out, ptr(state[0]), ptr(state[1]))
    torch.cuda.synchronize()
    ref = _dev(case, sfx, ALL, ld=ld)
    for w, o in zip(ALL, outs):
        assert _same(o[1:K + 1, :, :N], getattr(ref, w)), w
        assert bool((o[0] == SENT).all()) and bool((o[K + 1] == SENT).all()) and bool((o[:, :, N:] == SENT).all()), w
    assert bool((state[0][:, N:] == SENT).all()) and bool((state[1][:, N:] == SENT).all())
    assert _same(state[0][1:, :N], ref.cum_end[1:]) and bool((state[0][0, :N] == 0).all()) and _same(state[1][:, :N], ref.airborne_end)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_one_planted_nan_touches_its_row_and_the_next_sink(sfx):
    tile = _edges(sfx)[0]
    K, N, k, m = 6, tile + 1, 2, tile - 3
    case = cref.synthetic(3, K, N, NP[sfx], (2,))
    clean = _dev(case, sfx, ALL, ld=_aligned(N))
    case["rows"][k, 0, m] = np.nan                             # a stored C of the emission-driven gas 0
    case["rows"][k + 1, 2, m + 1] = np.nan                     # a stored E of the concentration-driven gas 2
    res = _dev(case, sfx, ALL, ld=_aligned(N))
    nans = {w: int(getattr(res, w).isnan().sum()) for w in ALL}
    # gas 0: airborne, uptake, fraction of row k, sink of rows k and k + 1; cumE is the shared table; iirf and alpha read the
    # cap (IEEE minNum, as in the stepping kernel).  gas 2: E enters cum and stays: cumE, uptake, fraction of rows k + 1 .. K - 1,
    # sink of row k + 1 only (G_a comes from the shared target); iirf and alpha read the cap on those rows
    tail = K - (k + 1)
    assert nans == dict(airborne=1, cumE=tail, uptake=1 + tail, fraction=1 + tail, iirf=0, alpha=0, sink=2 + 1), nans
    assert bool(res.airborne[k, 0, m].isnan()) and bool(res.sink[k + 1, 0, m].isnan()) and bool(res.cumE[K - 1, 2, m + 1].isnan())
    cap = float(NP[sfx](params.make_model(case["params"], 1.0).iirf_max))
    assert float(res.iirf[k, 0, m]) == cap and float(res.iirf[K - 1, 2, m + 1]) == cap
    for w in ALL:                                              # everything else is what it was
        a, b = getattr(res, w), getattr(clean, w)
        keep = torch.ones_like(a, dtype=torch.bool)
        keep[k:, 0, m] = False
        keep[k + 1:, 2, m + 1] = False
        assert torch.equal(a[keep], b[keep]), w


# ---- 6. the scenario axis, the engine's refusals ------------------------------------------------------------------------------
def test_the_scenario_axis_is_the_stack_of_its_scenarios_and_sink_closes_the_budget():
    from fiveeqscm_amd.engine import EnsembleEngine
    N, n_steps = 131, 24
    base = params.default_params("multigas")
    p = params.sample_ensemble_shard(base, N)
    E = emissions.rcp_like_emissions(n_steps, 3)
    E2 = np.stack([E, E])
    E2[1, 10:, 0] *= 1.5
    eng = EnsembleEngine(p, N, E2, device="cuda:0")
    eng.run(mode="fused")
    torch.cuda.synchronize()
    want = ("fraction", "sink", "alpha", "cumE")
    both = eng.carbon_rows(want=want)
    for s in range(2):
        one = eng.carbon_rows(want=want, scenario=s)
        for w in want:
            assert getattr(both, w).shape == (2, n_steps, 3, N) and torch.equal(getattr(both, w)[s], getattr(one, w)), (w, s)
        assert both.uptake is None and both.iirf is None
        # the budget closes: dt * the sum of the sink flux is the cumulative uptake (to rounding)
        res = eng.carbon_rows(want=("sink", "uptake"), scenario=s)
        total = _np(res.sink.sum(0))
        assert np.allclose(total, _np(res.uptake[-1]), rtol=1e-9, atol=1e-9)
    single = EnsembleEngine(p, N, E2[1], device="cuda:0")
    single.run(mode="per_step")
    torch.cuda.synchronize()
    assert torch.equal(single.carbon_rows(want=("alpha",)).alpha, both.alpha[1])
    with pytest.raises(ValueError, match="need rows from step 0"):
        single.carbon_rows(want=("sink",), rows=slice(2, None))
    later = single.carbon_rows(want=("fraction",), rows=slice(2, 10))     # nothing carried: rows may start anywhere
    assert later.fraction.shape == (8, 3, N) and torch.equal(later.fraction, both.fraction[1, 2:10])
    nostore = EnsembleEngine(p, N, E, device="cuda:0", store_concentrations=False)
    with pytest.raises(ValueError, match="no stored concentrations"):
        nostore.carbon_rows()
    comp = EnsembleEngine(p, N, E, device="cuda:0", dtype=torch.float32, compensated=True)
    with pytest.raises(ValueError, match="compensated=True"):
        comp.carbon_rows()
    for e in (eng, single, nostore, comp):
        e.close()


# ---- 7. downstream ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_the_rows_go_where_stored_rows_go(sfx):
    eng = _golden_run(sfx)[0]
    res = eng.carbon_rows(want=("sink", "fraction"))
    years = 1765.0 + np.arange(eng.n_steps)
    sink = res.sink[:, 0]
    sm = _np(sink).astype(np.float64).mean(1)
    obs = constrain.Observations.absolute(years, years[20::7], sm[20::7] + 0.05, 0.4)
    got = constrain.score_rows(sink, eng.out_steps, obs)
    assert np.array_equal(_np(got), constrain.misfit_numpy(_np(sink), obs.table))
    k = eng.n_rows - 1
    row = res.fraction[k:k + 1, 0]
    summ = gather_summary(row, (5.0, 50.0, 95.0))
    want = np.percentile(_np(row).astype(np.float64)[0], (5.0, 50.0, 95.0))
    assert np.array_equal(summ["percentiles"].numpy()[0], want)
