"""Pulse response on the MI355X (include/fiveeq.h, "PULSE RESPONSE"; fiveeqscm_amd/pulse.py): the five outputs against an
explicit row-order loop over the engine's own forcing rows bit for bit, the invariances (row split, member range, stride,
tail, repetition), the values against the oracle, the horizons, NaN containment, the ratios, the engine's refusals and the rows
downstream in gather_summary.

Shapes: N at the edges of a lane (M members) and of a workgroup's tile, taken from the library; 1, 2, 3 and FIVEEQ_BLOCK + 4
rows (one row step is in flight per lane, so 1 is the unroll; the last crosses one LDS staging chunk); G in {1, 3}; P in {1, 3}."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fiveeqscm_amd import _capi, emissions, params, pulse  # noqa: E402
from fiveeqscm_amd.forcing import ScenarioForcings  # noqa: E402
from oracle import fiveeq_oracle as npo  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = {"f64": torch.float64, "f32": torch.float32}
BLOCK = 256                                        # FIVEEQ_BLOCK: rows per LDS staging chunk
ROWS = (1, 2, 3, BLOCK + 4)
K_MAX, T0 = BLOCK + 4, 3
SIZES = {0: 100.0, 1: 10000.0, 2: 800.0}          # GtC, Mt CH4, Mt N2O-N: pulses of comparable forcing (0.5 to 1.5 W m-2 at first)


def _tile(sfx):
    lib = _capi.load()
    tile = int(lib.fiveeq_metrics_tile(8 if sfx == "f64" else 4))
    return tile, (2 if sfx == "f64" else 4)


def _sizes(sfx):
    tile, M = _tile(sfx)
    return (1, M - 1, M + 1, tile - 1, tile, tile + 1, 2 * tile + 3)


def _table(S, n_steps):
    t = np.arange(n_steps)
    one = np.stack([-0.9 * (t + 1.0) / n_steps, np.where(t % 7 == 3, -2.5, 0.0)], 1)
    return np.stack([one * (1.0 + 0.25 * s) for s in range(S)])


def _horizons(K):
    return tuple(sorted({1, min(2, K), max(1, K // 2), K})) + (K + 5,)


@functools.lru_cache(maxsize=None)
def _case(sfx, G, P, forc):
    """One scenario engine on a pulse experiment, run once in per_step at the largest N and row count, with the reference
    every test reads: F of every scenario from eng.forcing_rows, then F, C and T on the CPU widened to fp64, the differences and
    the running sums formed in an explicit row-order loop.  Nothing writes into it afterwards."""
    from fiveeqscm_amd.engine import EnsembleEngine
    N = _sizes(sfx)[-1]
    kind = "co2" if G == 1 else "multigas"
    base = params.default_params(kind)
    p = params.sample_ensemble_shard(base, N, 0, N)
    n_steps = T0 + K_MAX
    E = emissions.rcp_like_emissions(n_steps, G)
    if G >= P:
        exp = pulse.pulse_experiment(E, T0, [(g, SIZES[g]) for g in range(P)], K_MAX)
        Es, names = exp.emissions, exp.scenario_names
        table = [(1 + i, g, size) for i, (g, size) in enumerate(exp.pulses)]
    else:                                          # more pulses than gases: pulses of one gas, of different sizes
        Es = np.repeat(E[None], 1 + P, axis=0)
        table = [(1 + i, 0, 50.0 * (1 + i)) for i in range(P)]
        for s, g, size in table:
            Es[s, T0, g] += size
        names = None
    kw = {}
    if forc:
        sc = params.sample_forcing_scales(base, N, 0, N, ranges=[(0.8, 1.2)] * G + [(0.3, 2.0), (0.5, 1.5)])
        p["f_scale"], p["fx_scale"] = sc[:G], sc[G:]
        kw["forcing"] = ScenarioForcings(_table(1 + P, n_steps))
    eng = EnsembleEngine(p, N, Es, dtype=DTYPES[sfx], device="cuda:0", scenario_names=names, output_steps=range(T0, n_steps), **kw)
    eng.run(mode="per_step")
    torch.cuda.synchronize()
    F = torch.stack([eng.forcing_rows(want=("F",), scenario=s).F for s in range(1 + P)]).cpu().double()
    C, T = eng.C.cpu().double(), eng.T.cpu().double()
    ref = torch.empty((5, P, K_MAX, N), dtype=torch.float64)
    for i, (s, g, _) in enumerate(table):
        d = (F[s] - F[0], T[s] - T[0], C[s, :, g] - C[0, :, g])
        run = [torch.zeros(N, dtype=torch.float64) for _ in range(3)]
        for k in range(K_MAX):
            for j in range(3):
                run[j] = run[j] + d[j][k]
                ref[j, i, k] = run[j]
        ref[3, i], ref[4, i] = d[1], d[2]
    return eng, table, ref


def _call(eng, table, N, K, horizons, ld=None, cols=None, rows=None, state=None):
    """pulse.pulse_response on columns [:N] (or `cols`) and rows [:K] (or `rows`) of the engine's rows: copied to contiguous
    rows of their own (row stride N: 16-byte accesses wherever N allows), or embedded in rows of stride ld."""
    cols = slice(0, N) if cols is None else cols
    rows = slice(0, K) if rows is None else rows

    def put(t):
        t = t[..., cols]
        if ld is None:
            return t.contiguous()
        buf = torch.full(tuple(t.shape[:-1]) + (ld,), float("nan"), dtype=t.dtype, device=t.device)
        view = buf[..., :t.shape[-1]]
        view.copy_(t)
        return view

    return pulse.pulse_response(put(eng.C[:, rows]), put(eng.T[:, rows]), eng.out_steps[rows], eng.params, q=None, F_ext=eng.drive,
                                dt=eng.dt, base=0, pulses=table, horizons=horizons,
                                fscale=None if eng.fscale is None else put(eng.fscale), X=eng.fext, state=state)


NAMES = ("I_F", "I_T", "I_C", "dT", "dC")


def _same(a, b):
    """torch.equal with NaN equal to NaN (a horizon not reached is NaN)."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _expect(ref, N, K, horizons):
    """The reference's rows at the horizons, NaN beyond the K rows given."""
    want = torch.full((5, ref.shape[1], len(horizons), N), float("nan"), dtype=torch.float64)
    for h, n_h in enumerate(horizons):
        if n_h <= K:
            want[:, :, h] = ref[:, :, n_h - 1, :N]
    return want


# ---- 1. the exact reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forc", [False, True], ids=["plain", "scales"])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_outputs_equal_the_row_order_loop_over_the_forcing_rows_bit_for_bit(sfx, G, P, forc):
    """dF is the difference of the two runs' OWN forcings (eng.forcing_rows is proven against a replay) and every sum one fp64
    addition per row in row order: the explicit loop on the CPU gives all five outputs in every bit, at every horizon, for
    plain runs and for forcing=ScenarioForcings runs with non-unit scales and K = 2 categories."""
    eng, table, ref = _case(sfx, G, P, forc)
    for N in _sizes(sfx):
        for K in ROWS:
            hz = _horizons(K)
            res = _call(eng, table, N, K, hz)
            want = _expect(ref, N, K, hz)
            for i, name in enumerate(NAMES):
                got = getattr(res, name)
                assert got.dtype == torch.float64 and tuple(got.shape) == (P, len(hz), N)
                assert _same(got.cpu(), want[i]), (name, N, K)
            assert torch.equal(res.state.sums.cpu(), ref[0:3, :, K - 1, :N]) and res.state.rows == K, (N, K)
            assert bool(res.I_F[:, -1].isnan().all()) and not bool(res.I_F[:, :-1].isnan().any())


# ---- 2. independence of the launch form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_outputs_do_not_depend_on_row_split_member_range_stride_tail_or_repetition(sfx):
    eng, table, ref = _case(sfx, 3, 3, True)
    tile, M = _tile(sfx)
    K, hz = 6, (1, 3, 4, 6)
    N = tile + 1
    whole = _call(eng, table, N, K, hz)
    out = lambda r: torch.stack([getattr(r, n) for n in NAMES])                                 # noqa: E731
    assert not bool(out(whole).isnan().any())
    # the rows split over two calls at every row boundary, the state carried
    for k in range(1, K):
        a = _call(eng, table, N, K, hz, rows=slice(0, k))
        b = _call(eng, table, N, K, hz, rows=slice(k, K), state=a.state)
        assert torch.equal(out(b), out(whole)) and torch.equal(b.state.sums, whole.state.sums) and b.state.rows == K, k
        assert bool(out(a)[:, :, [h for h, n_h in enumerate(hz) if n_h > k]].isnan().all())
    # one row a call
    st = None
    for k in range(K):
        r = _call(eng, table, N, K, hz, rows=slice(k, k + 1), state=st)
        st = r.state
    assert torch.equal(out(r), out(whole)) and torch.equal(st.sums, whole.state.sums)
    # a member sub-range [a, b), in place (odd a: element accesses; a multiple of M: 16-byte accesses)
    for a_, b_ in ((3, N - 2), (M, 2 * M), (2 * M, N)):
        part = _call(eng, table, N, K, hz, cols=slice(a_, b_), ld=None)
        assert torch.equal(out(part), out(whole)[..., a_:b_]), (a_, b_)
        inplace = pulse.pulse_response(eng.C[:, :K, :, a_:b_], eng.T[:, :K, a_:b_], eng.out_steps[:K], eng.params, F_ext=eng.drive,
                                       dt=eng.dt, base=0, pulses=table, horizons=hz, fscale=eng.fscale[:, a_:b_], X=eng.fext)
        assert torch.equal(out(inplace), out(whole)[..., a_:b_]), (a_, b_)
    # padded rows: an odd stride (element accesses) and a multiple of M (16-byte accesses with a ragged tail)
    for ld in ((N + 5) | 1, (N + M - 1) // M * M + M):
        assert torch.equal(out(_call(eng, table, N, K, hz, ld=ld)), out(whole)), ld
    # an odd tail against the same members inside a larger ensemble
    big = _call(eng, table, 2 * tile + 3, K, hz)
    for n in (1, M - 1, M + 1, tile - 1):
        assert torch.equal(out(_call(eng, table, n, K, hz)), out(big)[..., :n]), n
    # repetition
    assert torch.equal(out(_call(eng, table, N, K, hz)), out(whole))


# ---- 3. values against the oracle ---------------------------------------------------------------------------------------------
N_ROWS_O, T0_O = 100, 5


@functools.lru_cache(maxsize=None)
def _oracle_case():
    """The 24 golden members of the default three-gas set (16 of the Latin hypercube, 8 corners of the perturbation box) under
    a CO2 pulse of 100 GtC and CH4 and N2O pulses of comparable forcing: the oracle's run() on each emission set, and from its
    rows the five outputs at the horizons with their bounds."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import fiveeq_cases as cases
    p, N = cases.members("multigas")
    E = emissions.rcp_like_emissions(T0_O + N_ROWS_O, 3)
    exp = pulse.pulse_experiment(E, T0_O, [(g, SIZES[g]) for g in range(3)], N_ROWS_O)
    runs = [npo.run(exp.emissions[s], p, N, keep=("C", "T", "F")) for s in range(4)]
    rows = slice(T0_O, T0_O + N_ROWS_O)
    F, T, C = (np.stack([r[k][rows] for r in runs]) for k in ("F", "T", "C"))
    hz = (20, 50, 100)
    # per value: |got - ref| <= 1e-10 |ref| + 1e-13 — for F twice the bound test_forcing_values (tests/test_forcing_rows_gpu.py)
    # holds F to; for T and C the engine's fp64 parity bound against the oracle (tests/test_engine_gpu.py:25-26 RTOL, ATOL;
    # :42-48 _close; :257-258 the per-step parity test).  A difference of two such values carries both bounds; a sum of n_h
    # differences their sum.
    val, bound = np.empty((5, 3, len(hz), N)), np.empty((5, 3, len(hz), N))
    for i in range(3):
        s, g = 1 + i, i
        d = (F[s] - F[0], T[s] - T[0], C[s, :, g] - C[0, :, g])
        b = (2.0 * (1e-10 * np.maximum(np.abs(F[0]), np.abs(F[s])) + 1e-13),
             (1e-10 * np.abs(T[0]) + 1e-13) + (1e-10 * np.abs(T[s]) + 1e-13),
             (1e-10 * np.abs(C[0, :, g]) + 1e-13) + (1e-10 * np.abs(C[s, :, g]) + 1e-13))
        for h, n_h in enumerate(hz):
            for j in range(3):
                val[j, i, h], bound[j, i, h] = d[j][:n_h].sum(0), b[j][:n_h].sum(0)
            val[3, i, h], bound[3, i, h] = d[1][n_h - 1], b[1][n_h - 1]
            val[4, i, h], bound[4, i, h] = d[2][n_h - 1], b[2][n_h - 1]
    return p, N, exp, hz, val, bound


def test_values_against_the_oracle_fp64(capsys):
    """I_F, I_T, I_C, dT, dC of the engine's fp64 rows against the oracle's, each within the cumulated per-value bounds (see
    _oracle_case).  The signal at the 100-year horizon exceeds 1000 times its bound for every member, pulse and output —
    checked on the oracle's numbers first — so the bounds cannot hide a wrong response.  fp32 is held to no tolerance here (test
    1 covers it bit for bit); its worst deviation from the fp64 oracle is printed (measured: profiles/r21/NOTES.md)."""
    from fiveeqscm_amd.engine import EnsembleEngine
    p, N, exp, hz, val, bound = _oracle_case()
    ratio = np.abs(val[:, :, -1]) / bound[:, :, -1]
    assert ratio.min() > 1000.0, ("signal / bound at the 100-year horizon", float(ratio.min()))
    worst32 = 0.0
    for sfx in ("f64", "f32"):
        eng = EnsembleEngine(p, N, exp.emissions, dtype=DTYPES[sfx], device="cuda:0", scenario_names=exp.scenario_names,
                             output_steps=exp.output_steps)
        eng.run(mode="per_step")
        res = eng.pulse_response(exp, hz)
        got = torch.stack([getattr(res, n) for n in NAMES]).cpu().numpy()
        assert np.isfinite(got).all()
        err = np.abs(got - val)
        if sfx == "f64":
            with capsys.disabled():
                print(f"\n  fp64 pulse response vs the oracle: worst error / bound {float((err / bound).max()):.3e}; "
                      f"smallest signal / bound at 100 years {float(ratio.min()):.3e}")
            assert np.all(err <= bound), {n: float((err[i] / bound[i]).max()) for i, n in enumerate(NAMES)}
        else:
            rel = err / np.abs(val)
            worst32 = {n: float(rel[i].max()) for i, n in enumerate(NAMES)}
            with capsys.disabled():
                print(f"  fp32 pulse response vs the fp64 oracle, worst |got - ref| / |ref| over 24 members, 3 pulses, horizons {hz}: "
                      + ", ".join(f"{n} {v:.3e}" for n, v in worst32.items()))


# ---- 4. horizons --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_a_horizon_beyond_the_rows_stays_nan_and_one_equal_to_the_rows_is_written(sfx):
    eng, table, ref = _case(sfx, 3, 1, False)
    N, K = 65, 7
    res = _call(eng, table, N, K, (K, K + 1))
    for i, name in enumerate(NAMES):
        got = getattr(res, name).cpu()
        assert torch.equal(got[:, 0], ref[i, :, K - 1, :N]) and bool(got[:, 1].isnan().all()), name
    # the later rows, carried: the second horizon is written by the call that reaches it, the first is kept
    more = _call(eng, table, N, K, (K, K + 1), rows=slice(K, K + 3), state=res.state)
    for i, name in enumerate(NAMES):
        got = getattr(more, name).cpu()
        assert torch.equal(got[:, 0], ref[i, :, K - 1, :N]) and torch.equal(got[:, 1], ref[i, :, K, :N]), name
    assert more.state.rows == K + 3
    with pytest.raises(ValueError, match="strictly increasing"):
        _call(eng, table, N, K, (3, 3))
    with pytest.raises(ValueError, match="strictly increasing"):
        _call(eng, table, N, K, tuple(range(1, 10)))


# ---- 5. NaN containment -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_a_nan_in_one_stored_T_reaches_that_members_T_sums_from_its_row_on_and_nobody_else(sfx):
    eng, table, ref = _case(sfx, 3, 3, False)
    tile, M = _tile(sfx)
    N, K, k_nan, m_nan = 4 * M + 1, 6, 2, 2 * M + 1
    hz = tuple(range(1, K + 1))
    C, T = eng.C[:, :K, :, :N].contiguous(), eng.T[:, :K, :N].contiguous()
    T[2, k_nan, m_nan] = float("nan")                              # scenario 2 is pulse 1
    res = pulse.pulse_response(C, T, eng.out_steps[:K], eng.params, F_ext=eng.drive, dt=eng.dt, base=0, pulses=table, horizons=hz)
    want = _expect(ref, N, K, hz)
    for i, name in enumerate(NAMES):
        got = getattr(res, name).cpu()
        hit = torch.zeros_like(got, dtype=torch.bool)
        if name == "I_T":
            hit[1, k_nan:, m_nan] = True
        if name == "dT":
            hit[1, k_nan, m_nan] = True
        assert torch.equal(got.isnan(), hit), name
        assert torch.equal(got[~hit], want[i][~hit]), name         # the lane's other members, the other pulses: their bits


# ---- 6. the ratios ------------------------------------------------------------------------------------------------------------
def test_gwp_of_a_pulse_against_itself_is_one_and_mass_scales_as_stated():
    eng, table, ref = _case("f64", 3, 3, False)
    res = _call(eng, table, 129, 100, (20, 100))
    for g in range(3):
        assert torch.equal(res.gwp(g)[g], torch.ones_like(res.I_F[g])) and torch.equal(res.gtp(g)[g], torch.ones_like(res.dT[g]))
    per = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda:0").reshape(-1, 1, 1)          # noqa: E731
    sizes = per([s for _, _, s in table])
    assert torch.equal(res.agwp(), eng.dt * res.I_F / sizes) and torch.equal(res.iagtp(), eng.dt * res.I_T / sizes)
    assert torch.equal(res.agtp(), res.dT / sizes)
    c = np.asarray(eng.params["emis2conc"], dtype=np.float64)
    assert torch.equal(res.irf(), res.dC / per([s * c[g] for _, g, s in table]))
    irf = res.irf().cpu().numpy()
    assert np.all((irf[0] > 0.2) & (irf[0] < 1.0)), "the airborne fraction of a CO2 pulse after 20 and 100 years"
    mass = [3.664e12, 1.0e9, 44.013 / 28.014 * 1.0e9]             # kg of CO2 per GtC, of CH4 per Mt CH4, of N2O per Mt N2O-N
    a = res.agwp() / per(mass)
    assert torch.equal(res.gwp(0, mass_kg=mass), a / a[0:1])
    gwp100 = res.gwp(0, mass_kg=mass)[1, 1].median().item()
    assert 5.0 < gwp100 < 100.0, gwp100                            # CH4 against CO2 per kg over 100 years: tens
    with pytest.raises(ValueError, match="no pulse of gas"):
        res.gwp(7)


# ---- 7. the engine's refusals -------------------------------------------------------------------------------------------------
def test_engine_refusals():
    from fiveeqscm_amd.engine import EnsembleEngine
    N, n_steps = 64, 24
    p = params.sample_ensemble_shard(params.default_params("co2"), N)
    E = emissions.rcp_like_emissions(n_steps, 1)
    exp = pulse.pulse_experiment(E, 2, [(0, 100.0)], 20)
    eng = EnsembleEngine(p, N, E, device="cuda:0")
    with pytest.raises(ValueError, match="one scenario"):
        eng.pulse_response([(1, 0, 100.0)], (10,))
    eng = EnsembleEngine(p, N, exp.emissions, device="cuda:0", store_concentrations=False)
    with pytest.raises(ValueError, match="no stored concentrations"):
        eng.pulse_response(exp, (10,))
    eng = EnsembleEngine(p, N, exp.emissions, device="cuda:0", output_steps=[2, 3, 4, 9])
    eng.run(mode="per_step")
    with pytest.raises(ValueError, match=r"row 2 holds step 4, row 3 step 9"):
        eng.pulse_response(exp, (2,))
    assert tuple(eng.pulse_response(exp, (2,), rows=slice(0, 3)).I_F.shape) == (1, 1, N)
    with pytest.raises(ValueError, match="other than the base"):
        eng.pulse_response([(0, 0, 100.0)], (2,), rows=slice(0, 3))
    with pytest.raises(TypeError, match="no CPU fallback"):
        pulse.pulse_response(eng.C.cpu(), eng.T.cpu(), eng.out_steps, p, F_ext=eng.drive, dt=1.0, base=0, pulses=[(1, 0, 1.0)],
                             horizons=(1,))


# ---- 8. downstream ------------------------------------------------------------------------------------------------------------
def test_agwp_rows_feed_gather_summary():
    from fiveeqscm_amd.distributed import gather_summary
    eng, table, ref = _case("f64", 3, 3, False)
    res = _call(eng, table, 1025, 100, (20, 100))
    pct = (5.0, 50.0, 95.0)
    for h in range(2):
        row = res.agwp()[0, h:h + 1]
        summ = gather_summary(row.contiguous(), pct)
        assert np.array_equal(summ["percentiles"].cpu().numpy()[0], np.percentile(row.cpu().numpy()[0], pct))
