"""GPU parity tests: the HIP path, called through the C ABI, against the CPU oracle.

For the five-equation path the oracle is the build's own restatement of the published
equations — the reference (stujen/fiveEqSCM @ v0) has no implementation of it ("parity
unpinned").  The reference's one function, emissions[0]*exp(-time)
(U_FaIR/concentrations.py:4-5), is pinned by golden vectors generated from the reference.

Tolerance (BASELINE.json north_star): fp64, <= 1e-10 relative on C and T.  T starts at 0 and
C sits on a 278/720/270 pedestal, so the comparisons use |a-b| <= 1e-10 |b| + atol with
atol = 1e-13 (K or ppm/ppb), far below any physical scale.
"""
import ctypes
import os

import numpy as np
import pytest

from fiveeqscm_amd import emissions as emi
from fiveeqscm_amd import params as prm
from oracle import c_oracle, fiveeq_oracle as npo

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RTOL = 1e-10
ATOL = 1e-13


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from fiveeqscm_amd import _capi
    _capi.load()                      # the HIP library must be the thing that runs: no fallback
    return torch.device("cuda:0")


def _engine(params, N, E, **kw):
    from fiveeqscm_amd.engine import EnsembleEngine
    return EnsembleEngine(params, N, E, device="cuda:0", **kw)


def _close(got, want, rtol=RTOL, atol=ATOL, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    err = np.abs(got - want)
    bound = rtol * np.abs(want) + atol
    worst = np.max(err / bound)
    assert np.all(np.isfinite(got)), f"{what}: non-finite output"
    assert worst <= 1.0, f"{what}: max err/bound = {worst:.3g} (abs {err.max():.3g})"
    return float(np.max(err / (np.abs(want) + 1e-300)))


# ---- the kernels' own math primitives, to the ulp --------------------------------------------------
def _ulp_err(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def test_device_math_primitives_within_two_ulp(gpu):
    """Hand-written expm1 / exp / log / sqrt / reciprocal (fiveeq_math.hpp) against NumPy (glibc /
    SVML, <= 1 ulp themselves) over the argument ranges the model can produce."""
    from fiveeqscm_amd import _capi
    lib = _capi.load()
    rng = np.random.default_rng(7)

    def probe(op, x):
        xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        yd = torch.empty_like(xd)
        _capi.check(lib, lib.fiveeq_math_probe_f64(op, xd.numel(), ctypes.c_void_p(xd.data_ptr()),
                                                   ctypes.c_void_p(yd.data_ptr()), None))
        torch.cuda.synchronize()
        return yd.cpu().numpy()

    n = 400_000
    # expm1 on (-inf, 0]: log-uniform magnitudes from 1e-300 to 800 plus edge values
    x = -np.concatenate([10.0 ** rng.uniform(-300, 2.9, n), rng.uniform(0, 2, n), [0.0, 1e-320, 0.3465, 0.3466, 0.6931,
                                                                                      0.6932, 36.0, 37.5, 745.0, 800.0, 1e300, np.inf]])
    got, want = probe(0, x), np.expm1(x)
    assert np.all(got[x == 0] == 0) and got[-1] == -1.0 and got[-2] == -1.0
    assert _ulp_err(got, want).max() <= 2.0, _ulp_err(got, want).max()
    small = np.abs(x) < 1e-5                                           # the tau = 1e6 yr pool: full RELATIVE accuracy
    assert np.max(np.abs(got[small] - want[small]) / np.maximum(np.abs(want[small]), 1e-320)) < 3e-16
    # exp on [-700, 700] (clamped outside)
    x = np.concatenate([rng.uniform(-700, 700, n), rng.uniform(-12, 12, n), [0.0, -700.0, 700.0]])
    assert _ulp_err(probe(1, x), np.exp(x)).max() <= 2.0
    assert probe(1, np.array([1e4, -1e4])).tolist() == [float(np.exp(700.0)), float(np.exp(-700.0))]
    # log, sqrt, reciprocal on positive normals
    x = np.concatenate([10.0 ** rng.uniform(-280, 280, n), rng.uniform(0.5, 4.0, n), [1.0, 0.5, 2.0, 0.7071067811865475,
                                                                                       0.7071067811865476, 1.4142135623730951]])
    got, want = probe(2, x), np.log(x)
    assert probe(2, np.array([1.0]))[0] == 0.0
    nz = want != 0
    assert _ulp_err(got[nz], want[nz]).max() <= 2.0, _ulp_err(got[nz], want[nz]).max()
    near1 = np.concatenate([rng.uniform(0.999, 1.001, n), 1.0 + 10.0 ** rng.uniform(-15, -3, 1000)])
    got, want = probe(2, near1), np.log(near1)                         # ln near 1 keeps RELATIVE accuracy
    nz = want != 0
    assert _ulp_err(got[nz], want[nz]).max() <= 2.0
    assert _ulp_err(probe(3, x), np.sqrt(x)).max() <= 1.0
    assert _ulp_err(probe(4, x), 1.0 / x).max() <= 1.0


def test_device_math_primitives_fp32(gpu):
    """The fp32 twins against fp64 NumPy rounded to float: <= 2 ulp (float); the log (hardware log2 x ln2) <= 2.5."""
    from fiveeqscm_amd import _capi
    lib = _capi.load()
    rng = np.random.default_rng(8)

    def probe(op, x):
        xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
        yd = torch.empty_like(xd)
        _capi.check(lib, lib.fiveeq_math_probe_f32(op, xd.numel(), ctypes.c_void_p(xd.data_ptr()),
                                                   ctypes.c_void_p(yd.data_ptr()), None))
        torch.cuda.synchronize()
        return yd.cpu().numpy(), xd.cpu().numpy().astype(np.float64)

    def ulp32(got, want64):
        w = want64.astype(np.float32)
        return np.abs(got.astype(np.float64) - want64) / np.spacing(np.abs(w)).astype(np.float64)

    n = 200_000
    x = -np.concatenate([10.0 ** rng.uniform(-30, 1.9, n), rng.uniform(0, 2, n), [0.0, 0.3466, 0.6932, 17.0, 86.9, 87.0, 87.1,
                                                                                     100.0, 1e30, np.inf]])
    got, xx = probe(0, x)
    assert ulp32(got, np.expm1(xx)).max() <= 2.0 and got[-6:].tolist() == [-1.0] * 6 and got[x == 0].tolist() == [0.0]
    small = np.abs(xx) < 1e-4                                          # slow pools: full RELATIVE accuracy of the increment
    assert np.max(np.abs(got[small] - np.expm1(xx[small])) / np.abs(np.expm1(xx[small])).clip(1e-300)) < 2e-7
    # the packed twins (two members per lane) return the scalar routines' bits, primitive by primitive
    samples = {0: x[:2 * (x.size // 2)], 1: np.concatenate([rng.uniform(-90, 90, n), rng.uniform(-12, 12, n)]),
               2: np.concatenate([10.0 ** rng.uniform(-30, 30, n), rng.uniform(0.5, 4.0, n)])}
    samples[3] = samples[4] = samples[2]
    for op, xs in samples.items():
        a_, _ = probe(op, xs)
        b_, _ = probe(op + 8, xs)
        assert np.array_equal(a_.view(np.uint32), b_.view(np.uint32)), op
    x = np.concatenate([rng.uniform(-80, 80, n), rng.uniform(-12, 12, n)])
    got, xx = probe(1, x)
    assert ulp32(got, np.exp(xx)).max() <= 2.0
    x = np.concatenate([10.0 ** rng.uniform(-30, 30, n), rng.uniform(0.5, 4.0, n), 1.0 + 10.0 ** rng.uniform(-6, -2, 1000)])
    got, xx = probe(2, x)
    nz = np.log(xx) != 0
    u = ulp32(got[nz], np.log(xx)[nz])
    # ln2 x the hardware log2 (v_log_f32, <= 1 ulp also next to 1): <= 2.1 ulp measured, 0.55 on average
    assert u.max() <= 2.5 and u.mean() < 0.7, (u.max(), u.mean())
    near = xx[nz] < 1.01
    assert u[(xx[nz] > 1.0) & near].max() <= 2.5                       # ln next to 1 keeps RELATIVE accuracy
    assert probe(2, np.array([1.0, 1.0]))[0].tolist() == [0.0, 0.0]    # and ln(1) is exactly 0: C = C0 gives no forcing
    got, xx = probe(3, x)
    assert ulp32(got, np.sqrt(xx)).max() <= 1.0
    got, xx = probe(4, x)
    assert ulp32(got, 1.0 / xx).max() <= 1.0


# ---- the reference's function, ensemble form ---------------------------------------------------
def test_hfc_conc_kernel_matches_reference_golden(gpu, golden_hfc):
    from fiveeqscm_amd.concentrations import calculate_hfc_conc_ensemble
    for name in ("ref_unit_test", "config1_float_time", "fractional_time"):
        case = next(c for c in golden_hfc["cases"] if c["name"] == name)
        e0 = float(np.asarray(case["emissions"], dtype=np.float64).ravel()[0])
        time = np.asarray(case["time"], dtype=np.float64).ravel()
        want = np.array([float.fromhex(h) for h in case["out_hex"]])
        members = np.array([e0, 2.0 * e0, 0.0, -e0, 1.0])
        out = calculate_hfc_conc_ensemble(members, time).cpu().numpy()
        assert out.shape == (time.size, 5)
        # device exp and NumPy's exp are each within 1 ulp of the exact value (measured 0.72 and 0.62 at worst,
        # tests/test_first_kernels_gpu.py / _cpu.py), so they differ by at most one last place of exp(-t), 2.2e-16 relative; the
        # two products round once each, 1.1e-16: 4.5e-16.  Below the normal range: one unit of 2^-1074 in exp(-t), times e0 exactly.
        np.testing.assert_allclose(out[:, 0], want, rtol=4.5e-16, atol=abs(e0) * 5e-324, err_msg=name)
        np.testing.assert_allclose(out[:, 1], 2.0 * want, rtol=4.5e-16, atol=2.0 * abs(e0) * 5e-324)
        assert np.all(out[:, 2] == 0.0)
        np.testing.assert_array_equal(out[:, 3], -out[:, 0])
    with pytest.raises(IndexError):
        calculate_hfc_conc_ensemble(np.array([]), np.array([0.0, 1.0]))


def test_hfc_conc_kernel_ragged_sizes(gpu):
    from fiveeqscm_amd.concentrations import calculate_hfc_conc_ensemble
    rng = np.random.default_rng(5)
    for N, K in ((1, 1), (63, 5), (257, 300), (1000, 513), (256, 256), (257, 512)):
        e0 = rng.normal(size=N) * 10
        time = rng.uniform(-2, 30, size=K)
        out = calculate_hfc_conc_ensemble(e0, time).cpu().numpy()
        # as above, against glibc's exp; every result here is a normal number, so no absolute floor
        np.testing.assert_allclose(out, c_oracle.hfc_conc(e0, time), rtol=4.5e-16, atol=0.0)


def test_engine_bridge_to_reference_function(gpu, golden_hfc):
    """One pool, a=1, tau=1, alpha=1, R(0)=E0, no emissions: the engine reproduces
    calculate_hfc_conc at integer times: the only bridge to the reference."""
    tau = 1.0
    p = {"a": [[1.0, 0, 0, 0]], "tau": [[tau, 1, 1, 1]], "r0": [tau * (-np.expm1(-100.0 / tau))], "rC": [0.0],
         "rT": [0.0], "ra": [0.0], "PI_conc": [1.0], "emis2conc": [1.0], "f": [[0.0, 0.0, 0.0]], "iirf_max": 1e9,
         "d": [239.0, 4.1], "q": [0.33, 0.41]}
    n_steps, N = 40, 130
    e0 = np.linspace(0.5, 20.0, N)
    e0[0] = 10.0
    for mode in ("per_step", "fused"):
        eng = _engine(p, N, np.zeros((n_steps, 1)), R0=e0[None, :])
        eng.run(mode=mode)
        torch.cuda.synchronize()
        got = eng.C[:, 0, :].cpu().numpy() - 1.0
        gold = next(c for c in golden_hfc["cases"] if c["name"] == "config1_float_time")
        ref = np.array([float.fromhex(h) for h in gold["out_hex"]])[1:n_steps + 1]     # 10*exp(-t), t=1..40
        np.testing.assert_allclose(got[:, 0], ref, rtol=1e-13, atol=2e-16)              # C0 = 1 pedestal: abs floor
        np.testing.assert_allclose(got, ref[:, None] * (e0 / 10.0)[None, :], rtol=1e-13, atol=1e-15)


def _one_pool(tau):
    return {"a": [[1.0, 0, 0, 0]], "tau": [[tau, 1, 1, 1]], "r0": [tau * (-np.expm1(-100.0 / tau))], "rC": [0.0],
            "rT": [0.0], "ra": [0.0], "PI_conc": [1.0], "emis2conc": [1.0], "f": [[0.0, 0.0, 0.0]], "iirf_max": 1e9,
            "d": [239.0, 4.1], "q": [0.33, 0.41]}


def test_constant_emissions_on_the_engine(gpu):
    """The reference announces "test under constant emissions" (tests/unit/test_hfcs.py:15) but never
    wrote it, and its function could not pass it (it only reads emissions[0]).  On the general engine:
    one pool, alpha = 1, constant E  =>  R_k = E tau (1 - exp(-k/tau))."""
    for tau in (1.0, 7.5, 52.0):
        n, E = 80, 3.0
        eng = _engine(_one_pool(tau), 70, np.full((n, 1), E))
        eng.run()
        torch.cuda.synchronize()
        k = np.arange(1, n + 1)
        want = E * tau * (1.0 - np.exp(-k / tau))
        np.testing.assert_allclose(eng.C[:, 0, 5].cpu().numpy() - 1.0, want, rtol=1e-12)


def test_pulse_not_in_year_zero_on_the_engine(gpu):
    """The reference announces "test where pulse isn't in year zero" (tests/unit/test_hfcs.py:16).
    A one-year emission of E in year k0 leaves E tau (1 - e^{-1/tau}) at the end of that year, which
    then decays as exp(-(t - k0)/tau): the shape of calculate_hfc_conc shifted to the pulse year."""
    from fiveeqscm_amd.concentrations import calculate_hfc_conc
    tau, k0, n, E = 1.0, 7, 40, 10.0
    em = np.zeros((n, 1))
    em[k0, 0] = E
    eng = _engine(_one_pool(tau), 3, em)
    eng.run(mode="fused")
    torch.cuda.synchronize()
    got = eng.C[:, 0, 0].cpu().numpy() - 1.0
    assert np.all(got[:k0] == 0.0)
    landed = E * tau * (1.0 - np.exp(-1.0 / tau))
    want = calculate_hfc_conc(np.array([landed]), np.arange(n - k0), lifetime=tau)       # the reference's shape
    np.testing.assert_allclose(got[k0:], want, rtol=1e-12, atol=5e-16)      # C0 = 1 pedestal: ulp(1) floor


# ---- five-equation parity at the BASELINE config shapes ------------------------------------------
CASES = [
    pytest.param("co2", 1, 10_000, 750, id="config2-co2-10k"),          # BASELINE configs[1], full size
    pytest.param("multigas", 3, 4096 + 37, 750, id="multigas-ragged"),   # configs[2] shape, scaled, ragged tail
    pytest.param("multigas", 3, 1, 50, id="single-member"),
    pytest.param("co2", 1, 255, 3, id="sub-block"),
]


@pytest.mark.parametrize("kind,G,N,n_steps", CASES)
def test_per_step_kernel_matches_oracle(gpu, kind, G, N, n_steps):
    p = prm.sample_ensemble(prm.default_params(kind), N)
    E = emi.rcp_like_emissions(n_steps, G)
    want = npo.run(E, p, N)
    eng = _engine(p, N, E)
    eng.run(mode="per_step")
    torch.cuda.synchronize()
    _close(eng.C, want["C"], what="C")
    _close(eng.T, want["T"], what="T")
    _close(eng.R, np.concatenate(want["R"], axis=0), atol=1e-12, what="R")
    _close(eng.S, want["S"], what="S")


@pytest.mark.parametrize("kind,G,N,n_steps", CASES)
def test_fused_and_graph_paths_are_bit_identical_to_per_step(gpu, kind, G, N, n_steps):
    p = prm.sample_ensemble(prm.default_params(kind), N)
    E = emi.rcp_like_emissions(n_steps, G)
    ref = _engine(p, N, E)
    ref.run(mode="per_step")
    for mode, k in (("fused", None), ("graph", None), ("ksteps", 1), ("ksteps", 7), ("ksteps", 16), ("auto", None)):
        eng = _engine(p, N, E)
        eng.run(mode=mode, k_steps=k)
        torch.cuda.synchronize()
        for name in ("C", "T", "R", "S"):
            assert torch.equal(getattr(eng, name), getattr(ref, name)), (mode, k, name)
        eng.close()


def test_fp32_modes_are_bit_identical_too(gpu):
    """The fp32 twins: every launch shape gives the same bits (the arithmetic is one member_step<float>())."""
    N, n_steps = 4096 + 37, 70
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    E = emi.rcp_like_emissions(750, 3)[250:250 + n_steps]
    ref = _engine(p, N, E, dtype=torch.float32)
    ref.run(mode="per_step")
    for mode, k in (("fused", None), ("graph", None), ("ksteps", 9), ("auto", None)):
        eng = _engine(p, N, E, dtype=torch.float32)
        eng.run(mode=mode, k_steps=k)
        torch.cuda.synchronize()
        for name in ("C", "T", "R", "S"):
            assert torch.equal(getattr(eng, name), getattr(ref, name)), (mode, k, name)
        eng.close()


def test_small_ensemble_kernel_config2_full_size_matches_the_oracle_and_the_per_step_path(gpu):
    """BASELINE configs[1] at full size: 10,000 CO2-only fp64 members x 750 steps through fiveeq_run_small_* — one member per
    QUAD of lanes (pool per lane; the sums over pools folded with DPP moves in the per-step order) and the same kernel
    unspread — against the C oracle at <= 1e-10 relative on C and T, and torch.equal to the per-step path (C, T, R, S)."""
    N, n_steps = 10_000, 750
    p = prm.sample_ensemble(prm.default_params("co2"), N)
    E = emi.rcp_like_emissions(n_steps, 1)
    want = c_oracle.run(E, p, N, n_threads=8)
    ref = _engine(p, N, E)
    ref.run(mode="per_step")
    for lanes in (4, 1, "auto"):
        eng = _engine(p, N, E, small_lanes=lanes)
        assert eng.small_form() == (4 if lanes == "auto" else lanes)
        eng.run(mode="small")
        torch.cuda.synchronize()
        _close(eng.C, want["C"], what=f"C lanes={lanes}")
        _close(eng.T, want["T"], what=f"T lanes={lanes}")
        for name in ("C", "T", "R", "S"):
            assert torch.equal(getattr(eng, name), getattr(ref, name)), (lanes, name)
        eng.close()
    auto = _engine(p, N, E)
    auto.run(mode="auto")
    torch.cuda.synchronize()
    assert auto.last_mode == "small" and torch.equal(auto.T, ref.T) and torch.equal(auto.R, ref.R)
    auto.close(), ref.close()


def test_small_ensemble_kernel_ragged_sizes_layouts_and_resume(gpu):
    """The small-ensemble kernel at ragged sizes (the last quad / wave / workgroup partly idle), both precisions, every
    single-gas layout (1-3 pools: one lane per member only), selected output rows, no stored concentrations, a run resumed
    mid-way and a member sub-range of a larger allocation: bit-identical to the per-step path every time."""
    from fiveeqscm_amd import _capi
    lib = _capi.load()
    rng = np.random.default_rng(55)
    n_steps = 140                                                    # > one 125-step chunk of the drive table
    E = emi.rcp_like_emissions(750, 1)[200:200 + n_steps]
    for N in (1, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 16_385):
        for td in (torch.float64, torch.float32):
            p = prm.sample_ensemble(prm.default_params("co2"), N, seed=N)
            kw = dict(dtype=td, output_steps=sorted(set(int(v) for v in rng.integers(0, n_steps, size=5))),
                      store_concentrations=bool(rng.integers(0, 2)))
            ref = _engine(p, N, E, **kw)
            ref.run(mode="per_step")
            for lanes in (1, 4):
                eng = _engine(p, N, E, small_lanes=lanes, **kw)
                cut = int(rng.integers(1, n_steps))
                eng.run(0, cut, mode="small")
                eng.run(cut, n_steps, mode="small")
                torch.cuda.synchronize()
                for name in ("T", "R", "S") + (("C",) if kw["store_concentrations"] else ()):
                    assert torch.equal(getattr(eng, name), getattr(ref, name)), (N, td, lanes, cut, name)
                eng.close()
            ref.close()
    # 1-3 pools: lanes_per_member = 1 is the only form (4 is refused)
    for pools in (1, 2, 3):
        base = prm.default_params("co2")
        a0, tau0 = np.asarray(base["a"], dtype=np.float64)[0], np.asarray(base["tau"], dtype=np.float64)[0]
        base = dict(base, a=[list(a0[:pools] / a0[:pools].sum()) + [0.0] * (4 - pools)], tau=[list(tau0[:pools]) + [1.0] * (4 - pools)])
        p = prm.sample_ensemble(base, 777, seed=pools)
        ref = _engine(p, 777, E)
        ref.run(mode="per_step")
        eng = _engine(p, 777, E)
        assert eng.small_widest == 1 and eng.small_form() == 1
        eng.run(mode="small")
        torch.cuda.synchronize()
        assert torch.equal(eng.T, ref.T) and torch.equal(eng.C, ref.C) and torch.equal(eng.R, ref.R)
        with pytest.raises(ValueError, match="small"):
            _engine(p, 777, E, small_lanes=4).run(mode="small")
        eng.close(), ref.close()
    # a member sub-range of a larger allocation through the raw C ABI: members outside untouched
    N = 1000
    p = prm.sample_ensemble(prm.default_params("co2"), N, seed=9)
    ref = _engine(p, N, E)
    ref.run(mode="per_step")
    for m0, n in ((0, 999), (128, 129), (1, 998), (333, 64), (999, 1)):
        for lanes in (1, 4):
            eng = _engine(p, N, E)
            rc = lib.fiveeq_run_small_f64(*eng._run_args(0, n_steps, m0, n), lanes, eng._stream())
            assert rc == 0, lib.fiveeq_last_error()
            torch.cuda.synchronize()
            assert torch.equal(eng.T[:, m0:m0 + n], ref.T[:, m0:m0 + n]) and torch.equal(eng.R[:, m0:m0 + n], ref.R[:, m0:m0 + n])
            assert int((eng.T[:, :m0] != 0).sum()) == 0 and int((eng.T[:, m0 + n:] != 0).sum()) == 0, (m0, n, lanes)
            eng.close()
    ref.close()


def test_small_multi_gas_ensembles_one_member_per_octet_of_lanes(gpu):
    """Round 6 (DESIGN r05 section 8 item 2): the 4 + 1 + 1 layout on an OCTET of lanes — gas 0's four pools on lanes 0-3, the
    single pools of gases 1 and 2 on lanes 4 and 5, every lane running ONE gas's closure / expm1 chain / forcing, the sums and the
    three forcings carried across lanes by DPP moves in member_step()'s order.  10,000 three-gas members x 750 steps against the
    C oracle at 1e-10 and torch.equal to the per-step path; ragged sizes (the last octet / wave / workgroup partly idle), both
    precisions, selected rows, no stored concentrations, a resumed run, a member sub-range of a larger allocation, random
    forcing coefficients (log / linear / square-root terms on or exactly off per gas); and what the form refuses."""
    from fiveeqscm_amd import _capi
    lib = _capi.load()
    N, n_steps = 10_000, 750
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    E = emi.rcp_like_emissions(n_steps, 3)
    want = c_oracle.run(E, p, N, n_threads=8)
    ref = _engine(p, N, E)
    ref.run(mode="per_step")
    for lanes in (8, "auto"):
        eng = _engine(p, N, E, small_lanes=lanes)
        assert eng.small_widest == 8 and eng.small_form() == 8
        eng.run(mode="small" if lanes == 8 else "auto")
        torch.cuda.synchronize()
        assert eng.last_mode == "small"
        _close(eng.C, want["C"], what="C octet")
        _close(eng.T, want["T"], what="T octet")
        for name in ("C", "T", "R", "S"):
            assert torch.equal(getattr(eng, name), getattr(ref, name)), (lanes, name)
        eng.close()
    ref.close()
    rng = np.random.default_rng(77)
    n_steps = 140                                                    # > one 125-step chunk of the drive table
    E = emi.rcp_like_emissions(750, 3)[200:200 + n_steps]
    for N in (1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 1000, 8193):
        for td in (torch.float64, torch.float32):
            base = dict(prm.default_params("multigas"))
            f = np.array(base["f"], dtype=np.float64)
            f[rng.uniform(size=f.shape) < 0.3] = 0.0                 # a term switched off exactly: selected away, not branched around
            f[rng.uniform(size=f.shape) < 0.2] = 0.01
            base["f"] = f
            p = prm.sample_ensemble(base, N, seed=N)
            kw = dict(dtype=td, output_steps=sorted(set(int(v) for v in rng.integers(0, n_steps, size=5))),
                      store_concentrations=bool(rng.integers(0, 2)))
            ref = _engine(p, N, E, **kw)
            ref.run(mode="per_step")
            eng = _engine(p, N, E, small_lanes=8, **kw)
            cut = int(rng.integers(1, n_steps))
            eng.run(0, cut, mode="small")
            eng.run(cut, n_steps, mode="small")
            torch.cuda.synchronize()
            for name in ("T", "R", "S") + (("C",) if kw["store_concentrations"] else ()):
                assert torch.equal(getattr(eng, name), getattr(ref, name)), (N, td, cut, name)
            eng.close(), ref.close()
    N = 1000
    p = prm.sample_ensemble(prm.default_params("multigas"), N, seed=9)
    ref = _engine(p, N, E)
    ref.run(mode="per_step")
    for m0, n in ((0, 999), (128, 129), (1, 998), (333, 64), (999, 1)):
        eng = _engine(p, N, E)
        rc = lib.fiveeq_run_small_f64(*eng._run_args(0, n_steps, m0, n), 8, eng._stream())
        assert rc == 0, lib.fiveeq_last_error()
        torch.cuda.synchronize()
        assert torch.equal(eng.T[:, m0:m0 + n], ref.T[:, m0:m0 + n]) and torch.equal(eng.R[:, m0:m0 + n], ref.R[:, m0:m0 + n])
        assert torch.equal(eng.C[:, :, m0:m0 + n], ref.C[:, :, m0:m0 + n]) and torch.equal(eng.S[:, m0:m0 + n], ref.S[:, m0:m0 + n])
        assert int((eng.T[:, :m0] != 0).sum()) == 0 and int((eng.T[:, m0 + n:] != 0).sum()) == 0, (m0, n)
        assert int((eng.R[:, :m0] != 0).sum()) == 0 and int((eng.R[:, m0 + n:] != 0).sum()) == 0, (m0, n)
        eng.close()
    ref.close()
    # statistics records: the octet form writes none — refused when asked for by name, the one-lane form when left to choose
    st = _engine(p, N, E, collect_stats=True)
    assert st.small_form() == 1
    with pytest.raises(ValueError, match="small"):
        _engine(p, N, E, collect_stats=True, small_lanes=8).run(mode="small")
    with pytest.raises(ValueError, match="small"):
        _engine(prm.sample_ensemble(prm.default_params("co2"), 50), 50, emi.rcp_like_emissions(20, 1), small_lanes=8).run(mode="small")
    st.close()


def test_auto_takes_the_small_ensemble_kernel_where_the_measured_table_says(gpu):
    """profiles/r05/small_ensemble_ab.txt, auto_window_sweep.txt: a launch-bound ensemble takes the small-ensemble kernel — the
    quad form while its waves get a SIMD each (64 members per CU), else one member per lane — and an ensemble whose step hides
    the launch boundary the per-step kernel; with hist= the streamed pipeline; never the inverse form."""
    E = emi.rcp_like_emissions(30, 1)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for N, mode, lanes in ((10_000, "small", 4), (64 * cus, "small", 4), (64 * cus + 1, "small", 1), (100_000, "small", 1),
                           (250_000, "small", 1), (300_000, "per_step", 1), (4_000_000, "per_step", 1)):
        p = prm.sample_ensemble_shard(prm.default_params("co2"), N, device="cuda:0")
        eng = _engine(p, N, E, store_trajectory=N < 1_000_000)
        assert eng.resolve_mode("auto")[0] == mode and (mode != "small" or eng.small_form() == lanes), (N, mode, lanes)
        eng.close()
    p = prm.sample_ensemble(prm.default_params("co2"), 5000)
    assert _engine(p, 5000, E, collect_stats=True).resolve_mode("auto")[0] == "small"                # statistics ride along
    assert _engine(p, 5000, E, hist=(-1.0, 5.0, 64)).resolve_mode("auto")[0] == "fused"
    assert _engine(p, 5000, E).resolve_mode("auto", 7) == ("ksteps", 7)               # an explicit K is taken as given
    assert _engine(p, 5000, E).auto_k_steps() == 30                                    # K-step form, launch-bound: the whole span
    assert _engine(p, 5000, emi.rcp_like_emissions(750, 1)).auto_k_steps() == 128
    pm = prm.sample_ensemble(prm.default_params("multigas"), 5000)
    em = _engine(pm, 5000, emi.rcp_like_emissions(30, 3))
    assert em.small_widest == 8 and em.resolve_mode("auto")[0] == "small" and em.small_form() == 8     # 4 + 1 + 1: an octet per member
    assert _engine(pm, 5000, emi.rcp_like_emissions(30, 3), collect_stats=True).small_form() == 1       # ... one lane with statistics
    big_m = 64 * cus + 1
    assert _engine(prm.sample_ensemble_shard(prm.default_params("multigas"), big_m, device="cuda:0"), big_m,
                   emi.rcp_like_emissions(30, 3)).small_form() == 1                                     # ... and past 64 members per CU
    with pytest.raises(ValueError, match="small"):
        _engine(pm, 5000, emi.rcp_like_emissions(30, 3), small_lanes=4).run(mode="small")
    with pytest.raises(ValueError, match="small"):
        _engine(pm, 5000, emi.rcp_like_emissions(30, 3), hist=(-1.0, 5.0, 64)).run(mode="small")


def test_packed_fp32_lanes_equal_scalar_lanes_bit_for_bit(gpu):
    """The fp32 entry points compute two members per lane (v_pk_* arithmetic, 8-byte row accesses) whenever the rows allow
    it.  Packed arithmetic is IEEE per component and mirrors the scalar routines operation by operation, so every
    member's C, T and state must equal the one-member-per-lane kernels' bit for bit — at ragged sizes (the last lane
    holds one member), on member sub-ranges of a larger allocation, for every pool layout family and launch shape; the
    per-64-member statistics records keep their layout (count / min / max identical, sums to rounding)."""
    from fiveeqscm_amd import _capi
    lib = _capi.load()
    rng = np.random.default_rng(77)
    n_steps = 48
    try:
        for kind, G in (("multigas", 3), ("co2", 1)):
            E = emi.rcp_like_emissions(750, G)[255:255 + n_steps]
            for N in (2, 64, 126, 128, 130, 256, 1000, 4098, 20_000):
                p = prm.sample_ensemble(prm.default_params(kind), N, seed=N)
                for mode, k in (("per_step", None), ("fused", None), ("ksteps", int(rng.integers(2, 11))), ("graph", None)):
                    runs = []
                    for packing in (1, 0):
                        lib.fiveeq_set_f32_packing(packing)
                        eng = _engine(p, N, E, dtype=torch.float32, collect_stats=True)
                        eng.run(mode=mode, k_steps=k)
                        torch.cuda.synchronize()
                        runs.append(eng)
                    a, b = runs
                    for name in ("C", "T", "R", "S"):
                        assert torch.equal(getattr(a, name), getattr(b, name)), (kind, N, mode, k, name)
                    sa, sb = a.stats_sums(), b.stats_sums()
                    assert torch.equal(sa[:, [0, 3, 4]], sb[:, [0, 3, 4]]), (kind, N, mode)
                    assert torch.allclose(sa[:, 1:3], sb[:, 1:3], rtol=1e-13, atol=1e-11), (kind, N, mode)
                    # the records themselves: one per 64 members, the same members in the same record
                    ra, rb = a.T_stats, b.T_stats
                    assert ra.shape == rb.shape and torch.equal(ra[:, :, 2:], rb[:, :, 2:]), (kind, N, mode)
                    assert torch.allclose(ra[:, :, :2], rb[:, :, :2], rtol=1e-13, atol=1e-11), (kind, N, mode)
                    a.close()
                    b.close()
        # the bin-index ring: packed lanes write two 2-byte indices as one word; every member must be counted once
        E = emi.rcp_like_emissions(750, 3)[255:255 + n_steps]
        for N in (2, 130, 2050, 4098, 20_000):
            p = prm.sample_ensemble(prm.default_params("multigas"), N, seed=N)
            for mode in ("fused", "per_step"):
                runs = []
                for packing in (1, 0):
                    lib.fiveeq_set_f32_packing(packing)
                    eng = _engine(p, N, E, dtype=torch.float32, collect_stats=True, hist=(-1.0, 5.0, 1000),
                                  hist_ring_steps=int(rng.integers(1, 12)))
                    eng.run(mode=mode)
                    torch.cuda.synchronize()
                    runs.append(eng)
                a, b = runs
                for name in ("C", "T", "R", "S", "T_hist"):
                    assert torch.equal(getattr(a, name), getattr(b, name)), (mode, N, name)
                assert a.T_hist.sum(1).tolist() == [N] * n_steps
                assert torch.equal(a.T_hist, a.T_histogram(-1.0, 5.0, 1000))
                sa, sb = a.stats_sums(), b.stats_sums()
                assert torch.equal(sa[:, [0, 3, 4]], sb[:, [0, 3, 4]]) and torch.allclose(sa[:, 1:3], sb[:, 1:3], rtol=1e-13, atol=1e-11)
                a.close()
                b.close()
        # an odd member count inside an even-strided allocation (the last packed lane stores one member only), and a
        # sub-range that starts at an odd member (not 8-byte aligned: the scalar kernels must take over) — through the raw
        # C ABI, members outside the range untouched
        N, G = 1000, 3
        E = emi.rcp_like_emissions(750, G)[255:255 + n_steps]
        p = prm.sample_ensemble(prm.default_params("multigas"), N, seed=5)
        for m0, n in ((0, 999), (0, 1), (128, 129), (1, 998), (333, 64)):
            outs = []
            for packing in (1, 0):
                lib.fiveeq_set_f32_packing(packing)
                eng = _engine(p, N, E, dtype=torch.float32)
                for fn_name in ("fiveeq_run_f32", "fiveeq_run_fused_f32"):
                    eng.reset_state()
                    rc = getattr(lib, fn_name)(*eng._run_args(0, n_steps, m0, n), eng._stream())
                    assert rc == 0
                    torch.cuda.synchronize()
                    outs.append([getattr(eng, name).clone() for name in ("C", "T", "R", "S")])
                eng.close()
            for other in outs[1:]:
                for x, y in zip(outs[0], other):
                    assert torch.equal(x, y), (m0, n)
            T_rows = outs[0][1]
            assert int((T_rows[:, :m0] != 0).sum()) == 0 and int((T_rows[:, m0 + n:] != 0).sum()) == 0
            assert bool((T_rows[-1, m0:m0 + n] != 0).all())
    finally:
        lib.fiveeq_set_f32_packing(1)


def test_step_by_step_equals_run_and_resume(gpu):
    """Python-driven step(t) == C-driven run(); a run split at any step resumes bit-identically
    (checkpoint = the R,S tensors)."""
    N, n_steps = 777, 120
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    E = emi.rcp_like_emissions(n_steps, 3)
    a = _engine(p, N, E)
    a.run()
    b = _engine(p, N, E)
    for t in range(n_steps):
        b.step(t)
    c = _engine(p, N, E)
    c.run(0, 47, mode="fused")
    R_ck, S_ck = c.R.clone(), c.S.clone()
    d = _engine(p, N, E, R0=R_ck.cpu().numpy(), S0=S_ck.cpu().numpy())
    d.run(47, n_steps, mode="per_step")
    torch.cuda.synchronize()
    for name in ("R", "S"):
        assert torch.equal(getattr(a, name), getattr(b, name))
        assert torch.equal(getattr(a, name), getattr(d, name))
    assert torch.equal(a.C, b.C) and torch.equal(a.T, b.T)
    assert torch.equal(a.C[47:], d.C[47:]) and torch.equal(a.T[47:], d.T[47:])


def test_checkpoint_state_dict_roundtrip(gpu, tmp_path):
    N, n_steps = 500, 90
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    E = emi.rcp_like_emissions(n_steps, 3)
    kw = dict(collect_stats=True, hist=(-1.0, 4.0, 512))
    whole = _engine(p, N, E, **kw)
    whole.run(mode="fused")
    first = _engine(p, N, E, **kw)
    first.run(0, 33, mode="fused")
    ck = first.state_dict(include_outputs=True)
    assert ck["t_next"] == 33
    np.savez(tmp_path / "ck.npz", **ck)
    second = _engine(p, N, E, **kw)
    second.load_state_dict(dict(np.load(tmp_path / "ck.npz")))
    assert second.t_next == 33
    second.run(second.t_next, n_steps, mode="fused")
    torch.cuda.synchronize()
    assert torch.equal(second.R, whole.R) and torch.equal(second.S, whole.S)
    # the checkpoint carries what the run had accumulated: ALL rows, moments and histograms equal an uninterrupted run
    assert torch.equal(second.T, whole.T) and torch.equal(second.C, whole.C)
    assert torch.equal(second.T_stats, whole.T_stats) and torch.equal(second.T_hist, whole.T_hist)
    # the default checkpoint carries the REDUCED outputs only (histograms + folded per-step moments; no per-wave records,
    # no stored rows): small whatever the ensemble size, and the resumed run's summaries still equal the uninterrupted run's
    small = first.state_dict()
    assert set(small) == {"R", "S", "t_next", "T_hist", "_step_sums", "_step_sums_valid"}
    assert small["_step_sums"].shape == (n_steps, 5) and small["_step_sums_valid"].tolist() == [True] * 33 + [False] * 57
    third = _engine(p, N, E, **kw)
    third.load_state_dict(small)
    third.run(33, n_steps, mode="per_step")                              # another launch shape after the resume
    torch.cuda.synchronize()
    assert torch.equal(third.T_hist, whole.T_hist) and torch.equal(third.T[33:], whole.T[33:])
    assert int(third.T[:33].abs().sum()) == 0                            # rows of the first leg were not carried
    a, b = third.stats_sums(), whole.stats_sums()
    assert torch.equal(a[:, [0, 3, 4]], b[:, [0, 3, 4]]) and torch.allclose(a[:, 1:3], b[:, 1:3], rtol=1e-13, atol=0)
    bare = _engine(p, N, E)
    bare.load_state_dict(first.state_dict(include_outputs=False))      # state only: later rows still right
    bare.run(33, n_steps, mode="fused")
    torch.cuda.synchronize()
    assert torch.equal(bare.T[33:], whole.T[33:]) and torch.equal(bare.C[33:], whole.C[33:])
    with pytest.raises(ValueError):
        second.load_state_dict({"R": np.zeros((2, 2)), "S": np.zeros((2, N))})
    # a checkpoint that does not fit is refused BEFORE anything is copied (R, S and the masks used to be overwritten
    # before the accumulators' shapes were looked at): the engine keeps its state, its accumulators and its bookkeeping
    before = {k: getattr(second, k).clone() for k in ("R", "S", "T_hist", "T_stats", "_step_sums")}
    masks = (second._step_sums_valid.copy(), second._stats_have.copy(), second.t_next)
    good = first.state_dict(include_outputs=True)
    for bad in (dict(good, T_hist=good["T_hist"][:, :100]), dict(good, T=good["T"][:5]), dict(good, _step_sums=good["_step_sums"][:7]),
                dict(good, T_hist=good["T_hist"].astype(np.float64)), dict(good, t_next=n_steps + 1),
                dict(good, _step_sums_valid=good["_step_sums_valid"][:3]), {k: v for k, v in good.items() if k != "S"}):
        with pytest.raises((ValueError, KeyError)):
            second.load_state_dict(bad)
        assert all(torch.equal(getattr(second, k), v) for k, v in before.items())
        assert (second._step_sums_valid == masks[0]).all() and (second._stats_have == masks[1]).all() and second.t_next == masks[2]


def test_reset_and_reload_clear_the_run_accumulators(gpu):
    """T_hist accumulates and a checkpoint's summaries leave folded per-step moments behind: reset_state() and a state-only
    load_state_dict() must clear both, or a second run double-counts its histogram and reads another run's moments."""
    N, n_steps = 3000, 40
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    E = emi.rcp_like_emissions(750, 3)[240:240 + n_steps]
    eng = _engine(p, N, E, store_concentrations=False, collect_stats=True, hist=(-1.0, 4.0, 256), hist_ring_steps=8)
    eng.run(mode="fused")                                                # streamed bin ring; moments from the wave records
    torch.cuda.synchronize()
    hist1, sums1 = eng.T_hist.clone(), eng.stats_sums().clone()
    assert hist1.sum(1).tolist() == [N] * n_steps and not eng._step_sums_valid.any()
    eng.reset_state()
    assert int(eng.T_hist.sum()) == 0 and eng.t_next == 0
    eng.run(mode="fused")
    torch.cuda.synchronize()
    assert torch.equal(eng.T_hist, hist1) and torch.equal(eng.stats_sums(), sums1)       # not doubled
    # another state, another mode: wave records are written and must be what stats_sums() reads
    other = _engine(p, N, E * 1.7, store_concentrations=False, collect_stats=True)
    other.run(0, 11, mode="fused")
    eng.load_state_dict(other.state_dict(include_outputs=False))
    assert int(eng.T_hist.sum()) == 0 and not eng._step_sums_valid.any() and eng.t_next == 11
    eng.run(11, n_steps, mode="per_step")
    torch.cuda.synchronize()
    want = _engine(p, N, E, store_concentrations=False, collect_stats=True)
    want.load_state_dict(other.state_dict(include_outputs=False))
    want.run(11, n_steps, mode="fused")
    torch.cuda.synchronize()
    a, b = eng.stats_sums(11, n_steps), want.stats_sums(11, n_steps)
    assert torch.equal(a[:, [0, 3, 4]], b[:, [0, 3, 4]]) and torch.allclose(a[:, 1:3], b[:, 1:3], rtol=1e-13, atol=0)
    assert not torch.allclose(a[:, 1], sums1[11:, 1], rtol=1e-6)                        # and NOT the first run's moments
    # folded moments a checkpoint brought stay valid until a run writes wave records for exactly those steps
    eng.reset_state()
    eng.run(mode="fused")
    fresh = _engine(p, N, E, store_concentrations=False, collect_stats=True, hist=(-1.0, 4.0, 256), hist_ring_steps=8)
    fresh.load_state_dict(eng.state_dict())                              # "summaries": T_hist + folded sums, no wave records
    assert fresh._step_sums_valid.all() and torch.equal(fresh.stats_sums(), eng.stats_sums())
    fresh.run(16, 24, mode="per_step")
    assert fresh._step_sums_valid[:16].all() and not fresh._step_sums_valid[16:24].any() and fresh._step_sums_valid[24:].all()
    for e in (eng, other, want, fresh):
        e.close()


def test_all_compiled_layouts_match_oracle(gpu):
    rng = np.random.default_rng(11)
    base = prm.default_params("multigas")
    layouts = [(1,), (2,), (3,), (4,), (1, 1), (4, 1), (4, 4), (1, 1, 1), (4, 1, 1), (4, 4, 1), (4, 4, 4)]
    N, n_steps = 300, 200
    for pools in layouts:
        G = len(pools)
        a = np.zeros((G, 4))
        tau = np.ones((G, 4))
        for g, P in enumerate(pools):
            w = rng.uniform(0.2, 1.0, size=P)
            a[g, :P] = w / w.sum()
            tau[g, :P] = np.sort(rng.uniform(2.0, 400.0, size=P))[::-1]
        p = {"a": a, "tau": tau, "r0": [30.0, 9.0, 60.0][:G], "rC": [0.015, 0.0, 0.001][:G],
             "rT": [3.0, -0.3, 0.5][:G], "ra": [0.0, 3e-4, 1e-4][:G], "PI_conc": base["PI_conc"][:G],
             "emis2conc": base["emis2conc"][:G], "f": base["f"][:G], "iirf_max": 97.0, "d": base["d"],
             "q": base["q"]}
        p = prm.sample_ensemble(p, N, seed=3)
        E = emi.rcp_like_emissions(n_steps, G)
        want = npo.run(E, p, N)
        first = None
        for mode in ("per_step", "fused", "small"):                   # (small: every layout has the one-lane form)
            eng = _engine(p, N, E)
            eng.run(mode=mode)
            torch.cuda.synchronize()
            _close(eng.C, want["C"], what=f"C {pools} {mode}")
            _close(eng.T, want["T"], what=f"T {pools} {mode}")
            if first is None:
                first = (eng.C.clone(), eng.T.clone(), eng.R.clone(), eng.S.clone())
            for x, y in zip(first, (eng.C, eng.T, eng.R, eng.S)):
                assert torch.equal(x, y), (pools, mode)                   # and all three are one arithmetic, bit for bit
        e32 = [_engine(p, N, E, dtype=torch.float32) for _ in range(2)]
        e32[0].run(mode="per_step")
        e32[1].run(mode="small")
        torch.cuda.synchronize()
        assert torch.equal(e32[0].C, e32[1].C) and torch.equal(e32[0].T, e32[1].T) and torch.equal(e32[0].R, e32[1].R), pools


def test_random_models_and_scenarios_match_oracle(gpu):
    """30 randomly drawn models (pool fractions and time-scales, feedback strengths, forcing
    coefficients, box time-scales, dt) x random emission series with spikes and negative spells,
    every compiled gas count: per-step, fused and small-ensemble paths against the NumPy oracle at 1e-10, and bit-identical
    among themselves (random forcing coefficients: the log, linear and square-root terms all on, or some of them exactly 0)."""
    rng = np.random.default_rng(2026)
    worst, ran, loose, points, n_out, members = 0.0, 0, 0, 0, 0, 0
    for case in range(30):
        G = int(rng.integers(1, 4))
        pools = [int(rng.choice([1, 4])) for _ in range(G)]
        if tuple(pools) not in {(1,), (4,), (1, 1), (4, 1), (4, 4), (1, 1, 1), (4, 1, 1), (4, 4, 1), (4, 4, 4)}:
            pools = sorted(pools, reverse=True)
        a = np.zeros((G, 4))
        tau = np.ones((G, 4))
        for g, P in enumerate(pools):
            w = rng.uniform(0.1, 1.0, size=P)
            a[g, :P] = w / w.sum()
            tau[g, :P] = np.sort(10.0 ** rng.uniform(0.3, 5.5, size=P))[::-1] if P > 1 else 10.0 ** rng.uniform(0.5, 2.3)
        N = int(rng.integers(1, 700))
        n_steps = int(rng.integers(5, 260))
        dt = float(rng.choice([0.25, 0.5, 1.0, 2.0]))
        base = {"a": a, "tau": tau, "r0": rng.uniform(8, 60, G), "rC": rng.uniform(0, 0.03, G),
                "rT": rng.uniform(-1, 5, G), "ra": rng.uniform(0, 5e-4, G), "PI_conc": rng.uniform(100, 800, G),
                "emis2conc": rng.uniform(0.1, 0.6, G), "f": rng.uniform(0, 1, (G, 3)) * np.array([5.0, 0.01, 0.1]),
                "iirf_max": float(rng.uniform(60, 110)), "d": np.array([rng.uniform(100, 400), rng.uniform(1, 9)]),
                "q": rng.uniform(0.1, 0.6, 2)}
        base["f"][rng.uniform(size=(G, 3)) < 0.25] = 0.0              # terms switched off exactly: the kernels skip them
        p = prm.sample_ensemble(base, N, seed=case)
        E = rng.normal(0, 1, (n_steps, G)).cumsum(0) * rng.uniform(0.1, 3.0, G) + rng.uniform(0, 8, G)
        E[rng.integers(0, n_steps, 3)] *= 6.0                          # spikes
        F_ext = rng.normal(0, 0.3, n_steps)
        want = npo.run(E, p, N, F_ext=F_ext, dt=dt)
        if not (np.all(np.isfinite(want["C"])) and np.all(np.isfinite(want["T"]))):
            continue                                                   # a draw the model itself cannot digest
        first = None
        for mode, lanes in ((("per_step", "auto"), ("fused", "auto"), ("small", 1)) + ((("small", 4),) if pools == [4] else ())
                            + ((("small", 8),) if pools == [4, 1, 1] else ())):
            eng = _engine(p, N, E, F_ext=F_ext, dt=dt, small_lanes=lanes)
            eng.run(mode=mode)
            torch.cuda.synchronize()
            if first is None:
                first = (eng.C.clone(), eng.T.clone())
            assert torch.equal(eng.C, first[0]) and torch.equal(eng.T, first[1]), (case, mode, lanes, pools)    # one arithmetic
            # POINTWISE, the tolerance every other test uses: |got - want| <= 1e-10 |want| + 1e-13 at every stored value.  Two
            # stated exceptions, both COUNTED so that a test that bounds everything loosely fails:
            # (1) where the oracle's own trajectory passes through zero (|x| < 1e-3 of that member's largest |x|: random F_ext
            #     makes T change sign) a relative bound is meaningless; there the bound is 1e-10 of the member's own scale;
            # (2) members that leave the MODEL'S DOMAIN — a gas with a logarithmic or square-root forcing term driven to
            #     C <= 0.02 C0 by the random negative emissions (draws 4, 18, 20, 26: 603 of 9530 members).  ln(C / C0) is singular
            #     at 0 and the step guards it (log term := 0 for C <= 0, oracle/fiveeq_oracle.py step_forc): a discontinuity,
            #     across which any rounding difference grows exponentially — the NumPy and the C oracle, the same algebra on the
            #     same CPU, differ by 1.3x the bound on draw 18's member 58, and by <= 2e-4 of it on every in-domain member of
            #     every draw.  Out-of-domain members are held to the draw-wide scale (round 5's bound for everything).
            sing = (np.asarray(base["f"])[:, 0] != 0) | (np.asarray(base["f"])[:, 2] != 0)
            outside = ((want["C"].min(axis=0) <= 0.02 * np.asarray(base["PI_conc"])[:, None]) & sing[:, None]).any(axis=0)      # [N]
            for name in ("C", "T"):
                w_ = want[name]
                got = getattr(eng, name).cpu().numpy()
                own = np.abs(w_).max(axis=0, keepdims=True)                  # per (gas,) member: its largest magnitude over time
                near0 = np.abs(w_) < 1e-3 * own
                scale = np.where(near0, own, np.abs(w_))
                draw_wide = (np.abs(w_ - np.asarray(base["PI_conc"])[None, :, None]).max() if name == "C" else np.abs(w_).max())
                scale = np.where(outside, np.maximum(scale, draw_wide), scale)
                err = np.abs(got - w_) / (RTOL * scale + ATOL)
                worst = max(worst, float(err.max()))
                if mode == "per_step" and name == "T":
                    loose, points = loose + int((near0 & ~outside).sum()), points + near0.size
                    n_out, members = n_out + int(outside.sum()), members + outside.size
                assert err.max() <= 1.0, (case, mode, pools, name, float(err.max()), np.unravel_index(err.argmax(), err.shape))
        ran += 1
    # every draw but the one the model itself cannot digest (draw 13 today) was held to the bound, nearly all of it pointwise
    assert ran >= 27 and worst > 0.0 and loose <= 0.02 * points and n_out <= 0.08 * members, (ran, worst, loose, points, n_out, members)


def test_minor_gas_forcing_equals_an_explicit_single_pool_gas(gpu):
    """Host-side constant-lifetime species (minor_gases) fed in as F_ext == the same species carried on the
    GPU as an explicit one-pool gas with alpha pinned to 1 and a linear forcing term."""
    from fiveeqscm_amd.minor_gases import step_minor_gases
    N, n_steps, tau, c, eff = 300, 150, 13.4, 0.5, 0.2
    base = prm.default_params("co2")
    p = prm.sample_ensemble(base, N)
    E = emi.rcp_like_emissions(n_steps, 2)[:, :1]
    Eh = 20.0 * np.abs(np.sin(np.arange(n_steps) / 17.0))
    _, F_h = step_minor_gases(Eh, lifetime=tau, emis2conc=c, rad_eff=eff)
    a = _engine(p, N, E, F_ext=F_h)
    a.run()
    r0_h = tau * (-np.expm1(-100.0 / tau))                       # iIRF_100 at alpha = 1
    p2 = dict(p)
    p2.update(a=[base["a"][0], [1.0, 0, 0, 0]], tau=[base["tau"][0], [tau, 1, 1, 1]], ra=[0.0, 0.0],
              PI_conc=[278.0, 1.0], emis2conc=[base["emis2conc"][0], c], f=[base["f"][0], [0.0, eff, 0.0]],
              r0=np.vstack([p["r0"], np.full((1, N), r0_h)]), rC=np.vstack([p["rC"], np.zeros((1, N))]),
              rT=np.vstack([p["rT"], np.zeros((1, N))]))
    b = _engine(p2, N, np.column_stack([E[:, 0], Eh]))
    b.run()
    torch.cuda.synchronize()
    _close(b.T, a.T.cpu().numpy(), rtol=1e-11, what="T")
    _close(b.C[:, 0], a.C[:, 0].cpu().numpy(), rtol=1e-12, what="CO2")


def test_external_forcing_and_substeps(gpu):
    N, n_steps, dt = 500, 300, 0.25
    p = prm.sample_ensemble(prm.default_params("co2"), N)
    E = emi.rcp_like_emissions(n_steps, 1)
    F_ext = 0.5 * np.sin(np.arange(n_steps) / 11.0) - 0.2
    want = npo.run(E, p, N, F_ext=F_ext, dt=dt)
    eng = _engine(p, N, E, F_ext=F_ext, dt=dt)
    eng.run()
    torch.cuda.synchronize()
    _close(eng.C, want["C"], what="C")
    _close(eng.T, want["T"], what="T")


def test_extreme_corner_of_the_hypercube(gpu):
    """verify on the highest-emission, highest-rT corner, where alpha feeds back
    hardest and the iIRF clip engages, not only at the centre."""
    N = 64
    base = prm.default_params("co2")
    p = dict(base)
    p["r0"] = np.full((1, N), 1.2 * base["r0"][0])
    p["rC"] = np.full((1, N), 1.5 * base["rC"][0])
    p["rT"] = np.linspace(0.5, 1.5, N)[None, :] * base["rT"][0]
    p["q"] = prm.k_q(np.full(N, 2.5), np.full(N, 4.5), base["d"], prm.forcing_2x(base))
    E = 3.0 * np.abs(emi.rcp_like_emissions(750, 1))          # ~29 GtC/yr peak, never negative
    want = npo.run(E, p, N, keep=("C", "T", "alpha"))
    assert want["alpha"].max() == pytest.approx(float(npo.g_0(base["a"][0], base["tau"][0]))
                                                * np.exp(97.0 / float(npo.g_1(base["a"][0], base["tau"][0]))))
    eng = _engine(p, N, E)
    eng.run()
    torch.cuda.synchronize()
    _close(eng.C, want["C"], what="C")
    _close(eng.T, want["T"], what="T")


def test_no_trajectory_mode_and_negative_concentration_guard(gpu):
    N, n_steps = 200, 100
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    E = emi.rcp_like_emissions(n_steps, 3)
    E[:, 1] = -400.0                                   # drives CH4 below zero: log/sqrt guards engage
    want = npo.run(E, p, N)
    assert want["C"][:, 1].min() < 0
    a = _engine(p, N, E)
    a.run()
    b = _engine(p, N, E, store_trajectory=False)
    b.run()
    c = _engine(p, N, E, store_trajectory=False)
    c.run(mode="fused")
    torch.cuda.synchronize()
    _close(a.C, want["C"], what="C")
    _close(a.T, want["T"], what="T")
    assert b.C is None and b.T is None
    assert torch.equal(a.R, b.R) and torch.equal(a.S, b.S) and torch.equal(a.R, c.R) and torch.equal(a.S, c.S)


def test_selected_output_steps(gpu):
    """Only the listed steps are stored (rows in step order); everything else is bit-identical."""
    N, n_steps = 700, 120
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    E = emi.rcp_like_emissions(n_steps, 3)
    full = _engine(p, N, E)
    full.run()
    sel = [119, 3, 40, 41]
    for mode in ("per_step", "fused", "graph"):
        eng = _engine(p, N, E, output_steps=sel)
        eng.run(mode=mode)
        torch.cuda.synchronize()
        assert eng.out_steps.tolist() == [3, 40, 41, 119] and eng.C.shape == (4, 3, N) and eng.T.shape == (4, N)
        assert torch.equal(eng.C, full.C[[3, 40, 41, 119]]) and torch.equal(eng.T, full.T[[3, 40, 41, 119]])
        assert torch.equal(eng.R, full.R) and torch.equal(eng.S, full.S)
        eng.close()
    # a drive table that names a row beyond n_rows must not write: run with n_rows = 2 through the C ABI
    from fiveeqscm_amd import _capi
    eng = _engine(p, N, E, output_steps=sel)
    guard = torch.full_like(eng.T, -5.0)
    eng.T = guard
    eng.n_rows = 2
    eng.run()
    torch.cuda.synchronize()
    assert torch.equal(guard[:2], full.T[[3, 40]]) and torch.all(guard[2:] == -5.0)
    assert _capi.load() is eng.lib


@pytest.mark.parametrize("mode", ["per_step", "fused", "graph"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000, 4096 + 37])
def test_on_device_stats_match_trajectory(gpu, mode, N):
    """Per-wave (sum, sum^2, min, max) records folded on the host == moments of the stored T rows
    == moments of the oracle's T, for ragged wave/workgroup tails too."""
    n_steps = 90
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    E = emi.rcp_like_emissions(n_steps, 3)
    eng = _engine(p, N, E, collect_stats=True)
    eng.run(mode=mode)
    torch.cuda.synchronize()
    st = eng.stats()
    T = eng.T.cpu().numpy()
    assert st["count"].tolist() == [float(N)] * n_steps
    np.testing.assert_allclose(st["mean"].cpu().numpy(), T.mean(1), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(st["var"].cpu().numpy(), T.var(1), rtol=1e-8, atol=1e-16)
    np.testing.assert_array_equal(st["min"].cpu().numpy(), T.min(1))
    np.testing.assert_array_equal(st["max"].cpu().numpy(), T.max(1))
    want = npo.run(E, p, N)["T"]
    np.testing.assert_allclose(st["mean"].cpu().numpy(), want.mean(1), rtol=1e-10, atol=1e-13)
    # stats without any stored trajectory: same records
    eng2 = _engine(p, N, E, collect_stats=True, store_trajectory=False)
    eng2.run(mode=mode)
    torch.cuda.synchronize()
    assert torch.equal(eng2.T_stats, eng.T_stats)


def test_small_ensemble_kernels_write_the_fused_kernels_statistics_records(gpu):
    """The small-ensemble kernels batch T over 8 steps and fold it with the fused kernel's own routine — a tile per wave (one
    lane per member), or one tile per workgroup whose four waves hold 16 members each (a quad per member) — so the per-64-member
    records are the fused kernel's BIT FOR BIT: ragged ensembles (a last record with 1 ... 63 members, a workgroup with idle
    waves), step ranges that are not multiples of 8, a run resumed mid-way, both precisions, one and three gases."""
    from fiveeqscm_amd import _capi
    lib = _capi.load()
    rng = np.random.default_rng(21)
    n_steps = 131                                                    # one 125-step drive chunk + a ragged rest
    for kind, G in (("co2", 1), ("multigas", 3)):
        E = emi.rcp_like_emissions(750, G)[210:210 + n_steps]
        for N in (1, 15, 17, 63, 64, 65, 255, 256, 257, 1000, 4097):
            for td in (torch.float64, torch.float32):
                p = prm.sample_ensemble(prm.default_params(kind), N, seed=N)
                ref = _engine(p, N, E, dtype=td, collect_stats=True, store_trajectory=False)
                lib.fiveeq_set_f32_packing(0)                        # (packed fp32 lanes fold a record's sums in another order)
                try:
                    ref.run(mode="fused")
                finally:
                    lib.fiveeq_set_f32_packing(1)
                for lanes in ((4, 1) if G == 1 else (1,)):
                    eng = _engine(p, N, E, dtype=td, collect_stats=True, store_trajectory=False, small_lanes=lanes)
                    cut = int(rng.integers(1, n_steps))
                    eng.run(0, cut, mode="small")
                    eng.run(cut, n_steps, mode="small")
                    torch.cuda.synchronize()
                    assert torch.equal(eng.T_stats, ref.T_stats), (kind, N, td, lanes, cut)
                    assert torch.equal(eng.R, ref.R) and torch.equal(eng.S, ref.S), (kind, N, td, lanes)
                    eng.close()
                ref.close()


@pytest.mark.parametrize("dtype,N", [("f64", 1), ("f64", 1023), ("f64", 1024), ("f64", 1025), ("f64", 70_001),
                                     ("f32", 300_007)])
def test_in_loop_histograms_equal_histograms_of_stored_rows(gpu, dtype, N):
    """T_hist[step][bin] of EVERY step without a stored trajectory, through the ring of bin indices
    the stepping kernel writes.  (i) bit for bit the histogram fiveeq_hist_rows_* makes of the stored T rows, at ragged
    sizes, with outliers in the edge bins; (ii) C, T, R, S and the per-wave moments identical to the plain fused kernel's;
    (iii) a run that stores NOTHING gives the same histogram; (iv) percentiles read off it lie within one bin
    width of np.percentile of the ORACLE's T."""
    n_steps = 90
    td = torch.float64 if dtype == "f64" else torch.float32
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    E = emi.rcp_like_emissions(n_steps, 3) * 1.7              # warmer: T spreads over many bins
    E[:, 0] = emi.rcp_like_emissions(750, 1)[200:200 + n_steps, 0] * 1.7
    lo, hi, nb = 0.05, 1.2, 4096                              # tight on purpose: both edge bins collect outliers
    ref = _engine(p, N, E, dtype=td, collect_stats=True)
    ref.run(mode="fused")
    eng = _engine(p, N, E, dtype=td, collect_stats=True, hist=(lo, hi, nb))
    eng.run(mode="fused")
    bare = _engine(p, N, E, dtype=td, store_trajectory=False, hist=(lo, hi, nb), hist_ring_steps=3)
    bare.run(0, 40, mode="fused")                             # ragged chunks, resumed
    bare.run(40, n_steps, mode="per_step")
    strm = _engine(p, N, E, dtype=td, output_steps=[3, 50, n_steps - 1], store_concentrations=False, collect_stats=True,
                   hist=(lo, hi, nb), hist_ring_steps=7)      # streamed pipeline: fused kernel + ring + second stream
    strm.run(0, 33, mode="fused")
    strm.hist_ring_steps = 11                                  # changed between runs: the ring is rebuilt, not overrun
    strm.run(33, n_steps, mode="fused")                        # resumed mid-chunk
    pers = _engine(p, N, E, dtype=td, output_steps=[3, 50], store_concentrations=False, collect_stats=True,
                   hist=(lo, hi, nb), chunk_members=256 if N > 600 else 0)     # per-step kernel + the ring strip
    pers.run(mode="per_step")
    torch.cuda.synchronize()
    for name in ("C", "T", "R", "S", "T_stats"):
        assert torch.equal(getattr(eng, name), getattr(ref, name)), name
    want = ref.T_histogram(lo, hi, nb)
    assert torch.equal(pers.T_hist, want) and torch.equal(pers.T, ref.T[[3, 50]])
    # the per-step kernel folds a wave's moments with the DPP ladder, the fused kernel with the LDS transpose:
    # same numbers, different summation order (min/max exact, sums to rounding)
    assert torch.equal(pers.T_stats[..., 2:], ref.T_stats[..., 2:])
    assert torch.allclose(pers.T_stats[..., :2], ref.T_stats[..., :2], rtol=1e-12, atol=0)
    assert torch.equal(eng.T_hist, want)
    assert torch.equal(strm.T_hist, want) and torch.equal(strm.T, ref.T[[3, 50, n_steps - 1]])
    assert torch.equal(strm.R, ref.R) and torch.equal(strm.stats_sums(), ref.stats_sums())
    assert torch.equal(bare.T_hist, want) and torch.equal(bare.R, ref.R)
    assert eng.T_hist.sum(1).tolist() == [N] * n_steps
    assert int(want[-1, 0]) + int(want[-1, -1]) > 0 or N < 100           # the edge bins are exercised
    assert torch.equal(eng.hist_edge_counts(), torch.stack([want[:, 0], want[:, -1]], dim=1))
    if dtype == "f64" and N >= 1000:
        from fiveeqscm_amd.distributed import histogram_percentiles
        wide = _engine(p, N, E, store_trajectory=False, hist=(-2.0, 12.0, nb))
        wide.run(mode="fused")
        torch.cuda.synchronize()
        T_or = c_oracle.run(E, p, N, n_threads=4)["T"]
        hp, tot = histogram_percentiles(wide.T_hist, -2.0, 12.0, (5.0, 50.0, 95.0))
        assert tot.tolist() == [float(N)] * n_steps
        # within one bin width (14 K / 4096) of the exact percentile wherever the sample itself resolves a bin
        # (neighbouring order statistics closer than a bin: true for N >= 50k except in the outermost tail)
        tol = 14.0 / nb * (1.0 if N >= 50_000 else 4.0)
        assert np.abs(hp.cpu().numpy() - np.percentile(T_or, (5.0, 50.0, 95.0), axis=1).T).max() < tol


def test_randomized_launch_shapes_and_histogram_specs(gpu):
    """60 random combinations of ensemble size (around the 64 / 256 / 1024 block edges), step sub-ranges, steps per
    launch, dtype, layout and histogram specification: K-step / small / streamed results must equal the fused kernel's
    bit for bit, and every in-loop histogram the histogram of the stored rows."""
    rng = np.random.default_rng(2026)
    edges = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 3000, 5000]
    for case in range(60):
        N = int(rng.choice(edges)) if rng.random() < 0.7 else int(rng.integers(1, 6000))
        n_steps = int(rng.integers(1, 70))
        t0 = int(rng.integers(0, n_steps))
        t1 = int(rng.integers(t0 + 1, n_steps + 1))
        kind, G = (("multigas", 3), ("co2", 1))[int(rng.integers(0, 2))]
        td = (torch.float64, torch.float32)[int(rng.integers(0, 2))]
        nb = int(rng.choice([1, 2, 3, 17, 512, 1000, 4095, 4096]))
        lo = float(rng.uniform(-3.0, 0.3))
        hi = lo + float(rng.uniform(0.05, 9.0))
        p = prm.sample_ensemble(prm.default_params(kind), N, seed=case)
        E = emi.rcp_like_emissions(750, G)[200:200 + n_steps] * float(rng.uniform(0.5, 2.5))
        ref = _engine(p, N, E, dtype=td, store_concentrations=False, collect_stats=True)
        ref.run(0, t0, mode="fused")                                  # a common, non-trivial starting state
        state = ref.state_dict(include_outputs=False)
        ref.run(t0, t1, mode="fused")
        want_hist = ref.T_histogram(lo, hi, nb, rows=list(range(t0, t1)))
        forms = [("fused", None), ("per_step", None), ("ksteps", int(rng.integers(1, 20))), ("small", 1)]
        if G == 1:                                                    # one member per quad of lanes: a lone 4-pool gas
            forms += [("small", 4)]
        for mode, k_use in forms:
            plain = mode in ("ksteps", "small")                       # forms that do not fill T_hist
            eng = _engine(p, N, E, dtype=td, store_concentrations=False, collect_stats=True,
                          hist=None if plain else (lo, hi, nb), hist_ring_steps=int(rng.integers(1, 12)),
                          small_lanes=k_use if mode == "small" else "auto")
            eng.load_state_dict(state)
            eng.run(t0, t1, mode=mode, k_steps=None if mode == "small" else k_use)
            torch.cuda.synchronize()
            what = (case, N, n_steps, t0, t1, kind, td, nb, mode, k_use)
            assert torch.equal(eng.R, ref.R) and torch.equal(eng.S, ref.S), what
            assert torch.equal(eng.T[t0:t1], ref.T[t0:t1]), what
            if not plain:
                assert torch.equal(eng.T_hist[t0:t1], want_hist), what
                assert int(eng.T_hist[:t0].sum()) == 0 and int(eng.T_hist[t1:].sum()) == 0, what
            a, b = eng.stats_sums(t0, t1), ref.stats_sums(t0, t1)
            assert torch.equal(a[:, [0, 3, 4]], b[:, [0, 3, 4]]), what
            assert torch.allclose(a[:, 1:3], b[:, 1:3], rtol=1e-11, atol=1e-9), what
            if mode == "small" and td == torch.float64:               # the fused kernel's records, bit for bit
                assert torch.equal(eng.T_stats[:, t0:t1], ref.T_stats[:, t0:t1]), what
            eng.close()
        ref.close()


def test_runs_are_reproducible_bit_for_bit(gpu):
    """No run-to-run nondeterminism: the integer histogram atomics commute, every floating-point reduction has a fixed
    order (per wave, then a fixed fold), and the two-stream pipeline is ordered by events."""
    N, n_steps = 300_011, 60
    p = prm.sample_ensemble_shard(prm.default_params("multigas"), N, device="cuda:0")
    E = emi.rcp_like_emissions(750, 3)[260:260 + n_steps]
    outs = []
    for rep in range(3):
        for mode in ("fused", "per_step"):
            eng = _engine(p, N, E, store_concentrations=False, output_steps=[10, 59], collect_stats=True,
                          hist=(-1.0, 5.0, 4096), hist_ring_steps=16)
            eng.run(mode=mode)
            torch.cuda.synchronize()
            outs.append((mode, eng.T_hist.clone(), eng.T.clone(), eng.R.clone(), eng.stats_sums().clone()))
            eng.close()
    for mode in ("fused", "per_step"):
        same = [o for o in outs if o[0] == mode]
        for other in same[1:]:
            for a, b in zip(same[0][1:], other[1:]):
                assert torch.equal(a, b), mode
    assert torch.equal(outs[0][1], outs[1][1])                                               # and the same histogram in both modes


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_histogram_kernel_and_percentiles(gpu, dtype):
    """fiveeq_hist_rows: EXACTLY the counts of the bin rule's reference (edge clamping, ragged chunk, NaN skipped,
    accumulation into an existing histogram), and the percentiles read from it against the exact ones."""
    from fiveeqscm_amd.distributed import histogram_percentiles
    N, n_steps = 40_000 + 123, 60
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    E = emi.rcp_like_emissions(n_steps, 3)
    eng = _engine(p, N, E, dtype=torch.float64 if dtype == "f64" else torch.float32)
    eng.run(mode="fused")
    torch.cuda.synchronize()
    T = eng.T.double().cpu().numpy()
    lo, hi, nb = -0.05, float(T.max()) * 0.9, 1024                    # hi below the maximum: exercises the edge bin
    h = eng.T_histogram(lo, hi, nb)
    torch.cuda.synchronize()
    # THE BIN RULE of include/fiveeq.h by its exact reference (oracle/summary_passes.bin_rule: the fp64 formula for fp64 rows,
    # one correctly rounded fp32 FMA for fp32 rows; proved in tests/test_hist_reference_cpu.py), on the rows in their own type
    from oracle.summary_passes import bin_rule
    rows = eng.T.cpu().numpy()
    pos = bin_rule(rows, lo, hi, nb, rows.dtype.type)
    want = np.stack([np.bincount(r, minlength=nb) for r in pos])
    got = h.cpu().numpy()
    assert np.array_equal(got, want) and np.array_equal(got.sum(1), np.full(n_steps, N))
    eng.T_histogram(lo, hi, nb, out=h)                                # accumulate: counts double
    torch.cuda.synchronize()
    assert np.array_equal(h.cpu().numpy(), 2 * got)
    eng.T[5, 17] = float("nan")                                       # NaN is skipped, not binned
    h5 = eng.T_histogram(lo, hi, nb, rows=[5])
    assert int(h5.sum()) == N - 1
    lo2, hi2 = float(T.min()) - 0.01, float(T.max()) + 0.01
    hp, tot = histogram_percentiles(eng.T_histogram(lo2, hi2, 4096, rows=list(range(10, 60))), lo2, hi2, (5.0, 50.0, 95.0))
    exact = np.percentile(T[10:60], (5.0, 50.0, 95.0), axis=1).T
    assert np.abs(hp.cpu().numpy() - exact).max() < (hi2 - lo2) / 4096
    # argument validation happens on the host
    from fiveeqscm_amd import _capi
    with pytest.raises(_capi.FiveEqError):
        eng.T_histogram(1.0, 1.0, 16)
    with pytest.raises(_capi.FiveEqError):
        eng.T_histogram(0.0, 1.0, 5000)


def test_stats_fp32_accumulate_in_fp64(gpu):
    N, n_steps = 5000, 60
    p = prm.sample_ensemble(prm.default_params("co2"), N)
    E = emi.rcp_like_emissions(n_steps, 1)
    eng = _engine(p, N, E, dtype=torch.float32, collect_stats=True)
    eng.run()
    torch.cuda.synchronize()
    T = eng.T.double().cpu().numpy()
    np.testing.assert_allclose(eng.stats()["mean"].cpu().numpy(), T.mean(1), rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("kind,G,N", [("multigas", 3, 1000), ("co2", 1, 257)])
def test_inverse_mode_matches_oracle_and_round_trips(gpu, kind, G, N):
    """Concentration-driven mode: diagnosed emissions, reached concentrations' forcing -> T, per-member
    cumulative emissions: all against the NumPy oracle; and the forward -> inverse round trip."""
    n_steps, j = 250, 5
    p = prm.sample_ensemble(prm.default_params(kind), N)
    E = emi.rcp_like_emissions(n_steps, G)
    fwd = _engine(p, N, E)
    fwd.run()
    torch.cuda.synchronize()
    target = fwd.C[:, :, j].cpu().numpy()
    want = npo.run_inverse(target, p, N)
    inv = _engine(p, N, target, concentration_driven=True, collect_stats=True)
    inv.run()
    torch.cuda.synchronize()
    _close(inv.E, want["E"], rtol=1e-8, atol=1e-9, what="E")          # E is a small difference of large terms
    _close(inv.T, want["T"], what="T")
    _close(inv.cumE, want["cumE"], rtol=1e-9, atol=1e-9, what="cumE")
    _close(inv.R, np.concatenate(want["R"], axis=0), atol=1e-11, what="R")
    np.testing.assert_allclose(inv.E[:, :, j].cpu().numpy(), E, rtol=1e-8, atol=1e-9)     # round trip
    _close(inv.T[:, j], fwd.T[:, j].cpu().numpy(), what="T round trip")
    np.testing.assert_allclose(inv.stats()["mean"].cpu().numpy(), inv.T.cpu().numpy().mean(1), rtol=1e-13)
    # split run (resume from R, S, cumE left on the device) == single run, bit for bit
    two = _engine(p, N, target, concentration_driven=True)
    two.run(0, 100)
    two.run(100, n_steps)
    torch.cuda.synchronize()
    assert torch.equal(two.E, inv.E) and torch.equal(two.T, inv.T) and torch.equal(two.cumE, inv.cumE)


def test_device_side_latin_hypercube(gpu):
    """fiveeq_lhs_rows_f64 (the kernel) against params.lhs_rows (the NumPy twin) BIT FOR BIT, on a shard of a
    larger design; params.sample_ensemble_shard on the device == on the host bit for bit; an engine built from the
    device tensors equals one built from their host copies."""
    for N, lo, hi in ((1, 0, 1), (1000, 0, 1000), (10_000_000, 3_750_000, 3_750_000 + 70_001),
                      (100_000_000, 99_900_000, 100_000_000)):
        got = prm.lhs_rows_device(N, range(11), lo, hi, "cuda:0").cpu().numpy()
        assert np.array_equal(got, prm.lhs_rows(N, range(11), lo, hi)), N
    N = 50_000
    base = prm.default_params("multigas")
    pd = prm.sample_ensemble_shard(base, 4 * N, N, 2 * N, device="cuda:0")
    ph = prm.sample_ensemble_shard(base, 4 * N, N, 2 * N)
    for name in ("r0", "rC", "rT", "q", "TCR", "ECS"):
        assert np.array_equal(pd[name].cpu().numpy(), ph[name]), name
    full = prm.sample_ensemble_shard(base, N, device="cuda:0")
    u = ((full["r0"][0] / base["r0"][0] - 0.8) / 0.4).cpu().numpy()
    assert np.array_equal(np.sort(np.floor(u * N + 1e-9).astype(np.int64).clip(0, N - 1)), np.arange(N))   # one per stratum
    E = emi.rcp_like_emissions(60, 3)
    a = _engine(pd, N, E)
    b = _engine(ph, N, E)
    a.run(mode="fused")
    b.run(mode="fused")
    torch.cuda.synchronize()
    assert torch.equal(a.T, b.T) and torch.equal(a.C, b.C)


def test_temperature_only_storage(gpu):
    N, n_steps = 900, 80
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    E = emi.rcp_like_emissions(n_steps, 3)
    full = _engine(p, N, E)
    full.run()
    for mode in ("per_step", "fused"):
        t_only = _engine(p, N, E, store_concentrations=False)
        t_only.run(mode=mode)
        torch.cuda.synchronize()
        assert t_only.C is None and torch.equal(t_only.T, full.T) and torch.equal(t_only.R, full.R)
        assert t_only.bytes_per_member_step("per_step") == 8 * (2 * 6 + 3 * 3 + 6 + 1)


# fp32 budget against the fp64 oracle over 750 steps, at the level the kernels actually reach (measured worst over these
# ensembles: 1.1e-5 relative on T, 1.2e-6 on C; profiles/r03/fp32_vs_fp64_sweep_1M.txt): 3e-5 on T, 5e-6 on C, with an
# absolute floor of a few fp32 roundings of the quantity's scale (T of order 1 K, concentrations of order 300-2000).
FP32_T = dict(rtol=3e-5, atol=2e-6)
FP32_C = dict(rtol=5e-6, atol=2e-4)


def test_fp32_kernel_tracks_fp64_oracle(gpu):
    """BASELINE configs[4] runs fp32: stay within 3e-5 (T) / 5e-6 (C) relative of the fp64 oracle over 750 steps
    (increment-form updates keep the tau = 1e6 yr pool alive in fp32) — packed lanes (even N) and scalar lanes (odd N)."""
    for N in (2048, 2047):
        p = prm.sample_ensemble(prm.default_params("multigas"), N)
        E = emi.rcp_like_emissions(750, 3)
        want = npo.run(E, p, N)
        for mode in ("per_step", "fused"):
            eng = _engine(p, N, E, dtype=torch.float32)
            eng.run(mode=mode)
            torch.cuda.synchronize()
            _close(eng.C.double(), want["C"], what="C32", **FP32_C)
            _close(eng.T.double(), want["T"], what="T32", **FP32_T)


def test_sharding_invariance(gpu):
    """Members never interact: running [0,N) as one shard or as two gives bit-identical members
    (the property the 8-GPU partition relies on)."""
    N, n_steps, cut = 3000, 150, 1234
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    E = emi.rcp_like_emissions(n_steps, 3)
    whole = _engine(p, N, E)
    whole.run()

    def shard(lo, hi):
        ps = dict(p)
        for k in ("r0", "rC", "rT", "q"):
            ps[k] = p[k][:, lo:hi]
        e = _engine(ps, hi - lo, E)
        e.run(mode="fused")
        return e

    s0, s1 = shard(0, cut), shard(cut, N)
    torch.cuda.synchronize()
    assert torch.equal(whole.C[:, :, :cut], s0.C) and torch.equal(whole.C[:, :, cut:], s1.C)
    assert torch.equal(whole.T[:, :cut], s0.T) and torch.equal(whole.T[:, cut:], s1.T)


@pytest.mark.parametrize("mode", ["per_step", "graph"])
def test_chunk_major_schedule_is_bit_identical(gpu, mode):
    """Large ensembles run chunk-major (all steps for members [0,c), then [c,2c), ...) to stay inside the
    Infinity Cache; members never interact, so every output — trajectories, state, per-wave statistics —
    must equal the plain schedule bit for bit, ragged last chunk included."""
    N, n_steps = 3000 + 77, 70
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    E = emi.rcp_like_emissions(n_steps, 3)
    plain = _engine(p, N, E, collect_stats=True, chunk_members=None)
    plain.run(mode=mode)
    chunked = _engine(p, N, E, collect_stats=True, chunk_members=1024)
    assert chunked._chunks() == [(0, 1024), (1024, 1024), (2048, 1024), (3072, 5)]
    chunked.run(0, 31, mode=mode)
    chunked.run(31, n_steps, mode=mode)
    torch.cuda.synchronize()
    for name in ("C", "T", "R", "S", "T_stats"):
        assert torch.equal(getattr(plain, name), getattr(chunked, name)), name
    auto = _engine(p, N, E)
    assert auto.chunk_members == 0                      # small ensembles are not chunked
    big = prm.default_params("multigas")
    from fiveeqscm_amd.engine import EnsembleEngine
    # the fewest EVEN chunks whose state + parameter rows take at most 0.7 of the 256 MiB cache each (profiles/r05/
    # chunk_share_sweep.txt); ensembles whose rows fit the cache (the 1M bench workload, the 1.25M config-4 shard) are not chunked
    auto = EnsembleEngine.auto_chunk
    assert auto(8_000_000, 6, 3, torch.float64) == 1_143_040 and auto(12_500_000, 6, 3, torch.float32) == 2_083_584
    assert auto(1_000_000, 6, 3, torch.float64) == 0 == auto(1_250_000, 6, 3, torch.float64) == auto(1_700_000, 6, 3, torch.float64)
    assert auto(1_800_000, 6, 3, torch.float64) == 900_096 and auto(2_400_000, 6, 3, torch.float64) == 1_200_128
    for n, td, w in ((1_800_000, torch.float64, 8), (8_000_000, torch.float64, 8), (100_000_000, torch.float32, 4), (4_000_001, torch.float32, 4)):
        c = auto(n, 6, 3, td)
        k = -(-n // c)
        assert c % 256 == 0 and c * w * 19 <= 0.7 * (256 << 20) + 256 * w * 19 and n - (k - 1) * c > c // 2      # even: no small ragged last chunk
    chunked.close()
    plain.close()


def test_leading_dimension_subrange(gpu):
    """ld > n_members: run the middle of a larger allocation through the raw C ABI and check the
    neighbours are untouched."""
    from fiveeqscm_amd import _capi
    lib = _capi.load()
    N, ld, lo, n_steps = 300, 1000, 350, 60
    p = prm.sample_ensemble(prm.default_params("co2"), N)
    E = emi.rcp_like_emissions(n_steps, 1)
    ref = _engine(p, N, E)
    ref.run()
    dev = torch.device("cuda:0")
    big = lambda rows: torch.full((rows, ld), -7.0, dtype=torch.float64, device=dev)   # noqa: E731
    r, q, R, S = big(3), big(2), big(4), big(2)
    C, T = big(n_steps), big(n_steps)
    r[:, lo:lo + N], q[:, lo:lo + N] = ref.r, ref.q
    R[:, lo:lo + N], S[:, lo:lo + N] = 0.0, 0.0
    off = lambda t: ctypes.c_void_p(t.data_ptr() + lo * 8)                              # noqa: E731
    rc = lib.fiveeq_run_f64(ctypes.byref(ref.model), N, ld, ctypes.c_void_p(ref.drive.data_ptr()), n_steps, 0,
                            n_steps, off(r), off(q), off(R), off(S), off(C), off(T), n_steps, None,
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _capi.check(lib, rc)
    torch.cuda.synchronize()
    assert torch.equal(C[:, lo:lo + N], ref.C[:, 0, :]) and torch.equal(T[:, lo:lo + N], ref.T)
    assert torch.equal(R[:, lo:lo + N], ref.R)
    for buf in (R, S, C, T):
        assert torch.all(buf[:, :lo] == -7.0) and torch.all(buf[:, lo + N:] == -7.0)


def test_full_size_config3_properties(gpu):
    """BASELINE configs[2] at full size (1M members, CO2+CH4+N2O, fp64, 750 steps): the oracle cannot
    run this in seconds, so use size-independent properties: the ensemble is a 4096-member block tiled
    244x (+ ragged tail); every tile must equal tile 0 bit-for-bit, and tile 0 must match the oracle."""
    N, B = 1_000_000, 4096
    blk = prm.sample_ensemble(prm.default_params("multigas"), B)
    p = dict(blk)
    reps = -(-N // B)
    for k in ("r0", "rC", "rT", "q"):
        p[k] = np.tile(blk[k], (1, reps))[:, :N]
    E = emi.rcp_like_emissions(750, 3)
    eng = _engine(p, N, E)
    eng.run()
    torch.cuda.synchronize()
    want = c_oracle.run(E, blk, B, n_threads=8)
    _close(eng.C[:, :, :B], want["C"], what="C tile0")
    _close(eng.T[:, :B], want["T"], what="T tile0")
    full = (N // B) * B
    Tt = eng.T[:, :full].view(750, N // B, B)
    assert torch.equal(Tt, Tt[:, :1, :].expand_as(Tt))
    Ct = eng.C[:, :, :full].view(750, 3, N // B, B)
    assert torch.equal(Ct, Ct[:, :, :1, :].expand_as(Ct))
    assert torch.equal(eng.T[:, full:], eng.T[:, :N - full])
    # and the fused path agrees bit-for-bit at full size
    Tp, Cp = eng.T.clone(), eng.C[-1].clone()
    eng.reset_state()
    eng.run(mode="fused")
    torch.cuda.synchronize()
    assert torch.equal(eng.T, Tp) and torch.equal(eng.C[-1], Cp)


def test_full_size_config5_shard_fp32_sparse_outputs(gpu):
    """BASELINE configs[4]: one GPU's shard of the 100M-member fp32 ensemble (12.5M members), run the way
    such a job must be run: time-fused, three stored years instead of a 150 GB trajectory, per-step
    moments on the device.  Size-independent checks: the ensemble is a 4096-member block tiled 3052x,
    so every stored row is periodic with period 4096 bit for bit; tile 0 tracks the fp64 oracle within
    the fp32 budget; the on-device moments equal the moments of the stored rows."""
    N, B, n_steps = 12_500_000, 4096, 750
    blk = prm.sample_ensemble(prm.default_params("multigas"), B)
    p = dict(blk)
    reps = -(-N // B)
    for k in ("r0", "rC", "rT", "q"):
        p[k] = np.tile(blk[k].astype(np.float32), (1, reps))[:, :N]
    E = emi.rcp_like_emissions(n_steps, 3)
    years = [249, 499, 749]
    eng = _engine(p, N, E, dtype=torch.float32, output_steps=years, collect_stats=True)
    eng.run(mode="fused")
    torch.cuda.synchronize()
    assert eng.T.shape == (3, N) and eng.C.shape == (3, 3, N)
    # the same shard with NO concentrations stored and the in-loop histograms of all 750 steps (streamed pipeline):
    # at the stored years they must equal the histograms of the stored rows, bit for bit, and every step counts N members
    hst = _engine(p, N, E, dtype=torch.float32, output_steps=years, store_concentrations=False, collect_stats=True,
                  hist=(-2.0, 12.0, 4096))
    hst.run(mode="fused")
    torch.cuda.synchronize()
    assert torch.equal(hst.T, eng.T)
    assert torch.equal(hst.T_hist[years], eng.T_histogram(-2.0, 12.0, 4096))
    assert hst.T_hist.sum(1).tolist() == [N] * n_steps
    a, b = hst.stats_sums(), eng.stats_sums()
    assert torch.equal(a[:, 3:], b[:, 3:]) and torch.allclose(a[:, 1:3], b[:, 1:3], rtol=1e-11, atol=1e-6)
    del hst
    want = c_oracle.run(E, blk, B, n_threads=8)
    _close(eng.T[:, :B].double(), want["T"][years], what="T tile0 fp32", **FP32_T)
    _close(eng.C[:, :, :B].double(), want["C"][years], what="C tile0 fp32", **FP32_C)
    full = (N // B) * B
    Tt = eng.T[:, :full].view(3, N // B, B)
    assert torch.equal(Tt, Tt[:, :1, :].expand_as(Tt))
    assert torch.equal(eng.T[:, full:], eng.T[:, :N - full])
    st = eng.stats()
    for row, t in enumerate(years):
        x = eng.T[row].double()
        assert abs(st["mean"][t].item() - x.mean().item()) <= 1e-12 * abs(x.mean().item())
        assert st["min"][t].item() == x.min().item() and st["max"][t].item() == x.max().item()
    assert st["count"][0].item() == float(N)


def test_whole_config5_ensemble_on_one_gpu(gpu):
    """BASELINE configs[4] WHOLE — 100,000,000 distinct fp32 Latin-hypercube members — on ONE MI355X (7.6 GB of state and
    parameters of 288 GB; three stored years; the per-wave statistics records alone are 37.5 GB, their offsets pass 2^32):
    the maximum size the configs name, with every index past 32 bits somewhere.  Size-independent checks: a strided sample
    of 4096 members against the fp64 oracle run on the same (fp32-rounded) parameters; the per-step path for the first
    steps bit for bit against the time-fused launch; the on-device moments against the stored rows, every member counted."""
    N, n_steps, years = 100_000_000, 750, [9, 249, 749]
    if torch.cuda.mem_get_info()[0] < 120 << 30:
        pytest.skip("needs ~100 GB of free HBM")
    pd = prm.sample_ensemble_shard(prm.default_params("multigas"), N, device=gpu, dtype=torch.float32)
    E = emi.rcp_like_emissions(n_steps, 3)
    eng = _engine(pd, N, E, dtype=torch.float32, output_steps=years, collect_stats=True)
    eng.run(mode="fused")
    torch.cuda.synchronize()
    idx = torch.arange(4096, device=gpu) * (N // 4096) + 17
    sample = dict(pd)
    for k in ("r0", "rC", "rT", "q"):
        sample[k] = pd[k][:, idx].double().cpu().numpy()
    want = c_oracle.run(E, sample, 4096, n_threads=8)
    _close(eng.T[:, idx].double(), want["T"][years], what="T sample fp32", **FP32_T)
    _close(eng.C[:, :, idx].double(), want["C"][years], what="C sample fp32", **FP32_C)
    st = eng.stats()
    assert st["count"].tolist() == [float(N)] * n_steps
    for row, t in enumerate(years):
        x = eng.T[row].double()
        assert abs(st["mean"][t].item() - x.mean().item()) <= 1e-11 * abs(x.mean().item())
        assert st["min"][t].item() == x.min().item() and st["max"][t].item() == x.max().item()
    T9, C9 = eng.T[0].clone(), eng.C[0].clone()
    eng.reset_state()
    eng.run(0, 10, mode="per_step")
    torch.cuda.synchronize()
    assert torch.equal(eng.T[0], T9) and torch.equal(eng.C[0], C9)
    eng.close()
    del eng, pd, T9, C9, x
    torch.cuda.empty_cache()                                     # ~60 GB back to the device for the tests that follow


def test_full_size_config3_direct_parity_of_final_state(gpu):
    """BASELINE configs[2] at full size with 1,000,000 DISTINCT Latin-hypercube members (no tiling): the
    final pools and thermal boxes after 750 steps against the plain-C oracle run on all usable host threads
    (~5 s on 16 threads).  The end state integrates every step's error, so this is the whole-run parity at the
    stated tolerance over the entire hypercube, corners included."""
    import os
    N, n_steps = 1_000_000, 750
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    E = emi.rcp_like_emissions(n_steps, 3)
    threads = len(os.sched_getaffinity(0))
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:
            quota, period = fh.read().split()[:2]
        if quota != "max":
            threads = max(1, min(threads, int(int(quota) / int(period))))
    except OSError:
        pass
    want = c_oracle.run(E, p, N, n_threads=min(threads, 64), keep=())
    eng = _engine(p, N, E, output_steps=[749], collect_stats=True)
    eng.run()
    torch.cuda.synchronize()
    _close(eng.R, want["R"], atol=1e-12, what="R final")
    _close(eng.S, want["S"], what="S final")
    T_end = want["S"][0] + want["S"][1]
    _close(eng.T[0], T_end, what="T final")
    st = eng.stats()
    assert abs(st["mean"][749].item() - T_end.mean()) < 1e-12 and st["max"][749].item() == eng.T[0].max().item()


def _host_threads():
    import os
    threads = len(os.sched_getaffinity(0))
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:
            quota, period = fh.read().split()[:2]
        if quota != "max":
            threads = max(1, min(threads, int(int(quota) / int(period))))
    except OSError:
        pass
    return min(threads, 64)


@pytest.mark.parametrize("chunk", [0, 262144])
def test_full_size_config4_shard_rank3_of_8(gpu, chunk):
    """BASELINE configs[3]: the 10M-member multi-gas ensemble over 8 GPUs.  This is rank 3's actual shard — members
    [3.75M, 5M) of the shard-computable 10M-member Latin hypercube, drawn on the device — at full size, fp64, 750 steps,
    with the chunk-major schedule off and on: final pools, thermal boxes and T of all 1.25M DISTINCT members against
    the C oracle run on the host twin of the same design."""
    from fiveeqscm_amd.distributed import shard_bounds
    N_total, n_steps = 10_000_000, 750
    lo, hi = shard_bounds(N_total, 3, 8)
    N = hi - lo
    assert N == 1_250_000
    base = prm.default_params("multigas")
    pd = prm.sample_ensemble_shard(base, N_total, lo, hi, device="cuda:0")
    ph = dict(pd)
    for k in ("r0", "rC", "rT", "q"):
        ph[k] = pd[k].cpu().numpy()
    E = emi.rcp_like_emissions(n_steps, 3)
    want = c_oracle.run(E, ph, N, n_threads=_host_threads(), keep=())
    eng = _engine(pd, N, E, output_steps=[249, 499, 749], collect_stats=True, chunk_members=chunk)
    assert len(eng._chunks()) == (1 if not chunk else 5)
    eng.run()
    torch.cuda.synchronize()
    _close(eng.R, want["R"], atol=1e-12, what="R final")
    _close(eng.S, want["S"], what="S final")
    T_end = want["S"][0] + want["S"][1]
    _close(eng.T[2], T_end, what="T final")
    st = eng.stats()
    assert abs(st["mean"][749].item() - T_end.mean()) < 1e-12 and st["count"][0].item() == float(N)
    # the percentile exchange of this shard alone (world size 1): exact against NumPy on the oracle's T
    from fiveeqscm_amd.distributed import gather_summary
    s = gather_summary(eng.T[2:3], percentiles=(5.0, 50.0, 95.0))
    np.testing.assert_allclose(s["percentiles"].cpu().numpy()[0], np.percentile(T_end, (5.0, 50.0, 95.0)), rtol=1e-10)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_percentile_selection_on_device_rows(gpu, dtype):
    """distributed.exact_percentiles on CUDA rows (the path RCCL runs take): histograms by the engine's HIP kernel,
    candidates by value with a one-bin margin — exact against NumPy, including ties, a constant row and heavy tails."""
    from fiveeqscm_amd.distributed import exact_percentiles, gather_summary
    rng = np.random.default_rng(9)
    n = 1_000_003
    x = np.stack([rng.normal(2.0, 0.7, n), rng.uniform(size=n) ** 6, np.full(n, -1.25), np.round(rng.normal(size=n), 2),
                  rng.standard_cauchy(n)])
    xt = torch.from_numpy(x).to("cuda:0", dtype)
    xs = xt.double().cpu().numpy()
    pct = (0.0, 0.1, 5.0, 50.0, 95.0, 99.9, 100.0)
    st = {}
    got = exact_percentiles(xt, pct, xt.min(1).values.double(), xt.max(1).values.double(), n, stats=st)
    np.testing.assert_allclose(got.cpu().numpy(), np.percentile(xs, pct, axis=1).T, rtol=1e-13, atol=0)
    one = gather_summary(xt, percentiles=pct)                   # one rank: the sort path
    np.testing.assert_allclose(one["percentiles"].cpu().numpy(), np.percentile(xs, pct, axis=1).T, rtol=1e-13, atol=0)


def test_bin_index_ring_equals_the_histogram_of_stored_rows_and_leaves_the_stored_concentrations(gpu):
    """The streamed form writes 2-byte bin indices from inside the fused kernel: its T_hist must equal the histogram of stored
    rows bit for bit (same bin rule), the model results must not notice it, the moments come from the kernel's wave
    records, and it coexists with stored C rows.  Ragged sizes (the last packed
    lane holds one member; rows that are not 8-byte aligned take the pass's narrow path), NaN-free edge bins in use."""
    rng = np.random.default_rng(3)
    for N, td in ((1, torch.float64), (2, torch.float32), (1001, torch.float64), (1001, torch.float32), (4098, torch.float32),
                  (70_000, torch.float32), (70_001, torch.float64)):
        n_steps = 41
        p = prm.sample_ensemble(prm.default_params("multigas"), N, seed=N)
        E = emi.rcp_like_emissions(750, 3)[270:270 + n_steps]
        lo, hi, nb = 0.2, 1.4, int(rng.choice([7, 512, 4096]))          # tight range: both edge bins collect outliers
        a = _engine(p, N, E, dtype=td, collect_stats=True, hist=(lo, hi, nb), hist_ring_steps=int(rng.integers(1, 9)))
        a.run(mode="fused")
        ref = _engine(p, N, E, dtype=td, collect_stats=True)
        ref.run(mode="fused")
        torch.cuda.synchronize()
        assert a.C is not None and torch.equal(a.T_hist, ref.T_histogram(lo, hi, nb)), (N, td, nb)
        assert a.T_hist.sum(1).tolist() == [N] * n_steps
        assert N < 1000 or (int(a.T_hist[:, 0].sum()) > 0 and int(a.T_hist[:, -1].sum()) > 0)      # both edge bins in use
        for name in ("C", "T", "R", "S", "T_stats"):
            assert torch.equal(getattr(a, name), getattr(ref, name)), (N, td, name)
        assert torch.equal(a.stats_sums(), ref.stats_sums()) and not a._step_sums_valid.any()
        # the per-step form of the same ring: the step kernel writes the bin indices; stored C rows allowed here too
        c = _engine(p, N, E, dtype=td, collect_stats=True, hist=(lo, hi, nb), hist_ring_steps=int(rng.integers(1, 9)),
                    per_step_streams=int(rng.integers(1, 3)))
        c.run(0, 17, mode="per_step")
        c.run(17, n_steps, mode="per_step")
        torch.cuda.synchronize()
        assert torch.equal(c.T_hist, a.T_hist), (N, td, nb, "per_step")
        for name in ("C", "T", "R", "S"):
            assert torch.equal(getattr(c, name), getattr(ref, name)), (N, td, name, "per_step")
        sc, sr = c.stats_sums(), ref.stats_sums()
        assert torch.equal(sc[:, [0, 3, 4]], sr[:, [0, 3, 4]]) and torch.allclose(sc[:, 1:3], sr[:, 1:3], rtol=1e-13, atol=1e-11)
        for e in (a, c, ref):
            e.close()


def test_per_step_parts_on_two_streams_are_bit_identical(gpu):
    """mode='per_step' may launch a timestep as several kernels over contiguous member parts on their own streams (one part's
    launch tail overlaps the other's kernel).  Members never interact: results, statistics records and stored rows must
    equal the single-launch form bit for bit, for both precisions, with chunk-major on top, resumed mid-run, and on the
    caller's non-default stream; the automatic choice splits only launches long enough to gain from it."""
    N, n_steps = 40_000 + 257, 60
    E = emi.rcp_like_emissions(750, 3)[250:250 + n_steps]
    for td in (torch.float64, torch.float32):
        p = prm.sample_ensemble(prm.default_params("multigas"), N, seed=9)
        ref = _engine(p, N, E, dtype=td, collect_stats=True, per_step_streams=1, chunk_members=0)
        ref.run(mode="per_step")
        for streams, chunk in ((2, 0), (3, 0), (2, 16384)):
            eng = _engine(p, N, E, dtype=td, collect_stats=True, per_step_streams=streams, chunk_members=chunk)
            lay = eng.per_step_launches()
            assert sum(n for _, n, _ in lay) == N and max(si for _, _, si in lay) == streams - 1
            assert all(m0 % 256 == 0 for m0, _, _ in lay) and [m0 for m0, _, _ in lay] == sorted(m0 for m0, _, _ in lay)
            user = torch.cuda.Stream()
            with torch.cuda.stream(user):
                eng.run(0, 23, mode="per_step", stream=user)
                eng.run(23, n_steps, mode="per_step", stream=user)
            user.synchronize()
            for name in ("C", "T", "R", "S", "T_stats"):
                assert torch.equal(getattr(eng, name), getattr(ref, name)), (td, streams, chunk, name)
            # back-to-back calls without joins in between (bench.py's repeated blocks), joined once at the end
            eng.reset_state()
            for t in range(0, n_steps, 7):
                eng.run(t, min(n_steps, t + 7), mode="per_step", join=False)
            assert eng._ps_unjoined
            eng.join()
            torch.cuda.current_stream().synchronize()
            for name in ("C", "T", "R", "S", "T_stats"):
                assert torch.equal(getattr(eng, name), getattr(ref, name)), (td, streams, chunk, name, "unjoined")
            # graph replay: one captured plan per part, replayed side by side on the same streams
            eng.reset_state()
            eng.run(mode="graph")
            torch.cuda.synchronize()
            assert len(eng.prepare_graph()) == len(lay)
            for name in ("C", "T", "R", "S", "T_stats"):
                assert torch.equal(getattr(eng, name), getattr(ref, name)), (td, streams, chunk, name, "graph")
            eng.run(0, 5, mode="per_step", join=False)
            eng.reset_state()                                    # joins by itself before it touches the state
            assert not eng._ps_unjoined and int(eng.R.abs().sum()) == 0
            eng.close()
        ref.close()
    small = _engine(prm.sample_ensemble(prm.default_params("multigas"), 4096), 4096, E)
    assert small.per_step_streams == 1 and small.per_step_launches() == [(0, 4096, 0)]
    from fiveeqscm_amd import engine as eng_mod
    t_1m = 1_000_000 * 248 / eng_mod.HBM_STREAM_BYTES_PER_S
    assert t_1m >= eng_mod.PER_STEP_SPLIT_MIN_S > 250_000 * 248 / eng_mod.HBM_STREAM_BYTES_PER_S
    small.close()


def test_streamed_rows_are_bit_identical_and_picked_for_the_launches_that_cannot_stay_cached(gpu):
    """include/fiveeq.h, "CACHE POLICY OF THE PER-STEP KERNEL'S ROWS": the STREAMED form of the per-step kernel (non-temporal
    loads and stores of the state and parameter rows) is the same arithmetic — per-step, step-by-step and graph replay, both
    precisions (packed and scalar fp32 lanes), several layouts, ragged sizes, sub-ranges: bit for bit — and the library's own
    rule takes it exactly for the launches whose rows cannot survive until the next step."""
    from fiveeqscm_amd import _capi
    lib = _capi.load()
    CACHED, STREAMED, AUTO = 0, 1, 2
    n_steps = 40
    try:
        for kind, G, N, td in (("multigas", 3, 70_001, torch.float64), ("multigas", 3, 70_001, torch.float32),
                               ("multigas", 3, 70_002, torch.float32), ("co2", 1, 4097, torch.float64), ("co2", 1, 1, torch.float32)):
            E = emi.rcp_like_emissions(750, G)[240:240 + n_steps]
            p = prm.sample_ensemble(prm.default_params(kind), N, seed=5)
            out = {}
            for policy in (CACHED, STREAMED):
                lib.fiveeq_set_row_policy(policy)
                eng = _engine(p, N, E, dtype=td, collect_stats=True, per_step_streams=2 if N > 1024 else 1)
                eng.run(0, 11, mode="per_step")
                for t in range(11, 15):
                    eng.step(t)
                eng.run(15, n_steps, mode="graph")
                torch.cuda.synchronize()
                out[policy] = [getattr(eng, name).clone() for name in ("C", "T", "R", "S", "T_stats")]
                eng.close()
            for a, b, name in zip(out[CACHED], out[STREAMED], ("C", "T", "R", "S", "T_stats")):
                assert torch.equal(a, b), (kind, N, td, name)
        # the rule, end to end: an 8M-member fp64 ensemble run unchunked streams, its chunk-major schedule does not
        lib.fiveeq_set_row_policy(AUTO)
        pools = (ctypes.c_int32 * 3)(4, 1, 1)
        N = 8_000_000
        big = _engine(prm.sample_ensemble_shard(prm.default_params("multigas"), N, device=gpu), N,
                      emi.rcp_like_emissions(750, 3)[240:252], output_steps=[11])
        assert big.chunk_members and all(lib.fiveeq_rows_streamed(3, pools, n, N, 8) == 0 for _, n, _ in big.per_step_launches())
        big.run(mode="per_step")
        torch.cuda.synchronize()
        T_chunked, R_chunked = big.T.clone(), big.R.clone()
        big.chunk_members = 0
        assert all(lib.fiveeq_rows_streamed(3, pools, n, N, 8) == 1 for _, n, _ in big.per_step_launches())
        big.reset_state()
        big.run(mode="per_step")
        torch.cuda.synchronize()
        assert torch.equal(big.T, T_chunked) and torch.equal(big.R, R_chunked)
        big.close()
    finally:
        lib.fiveeq_set_row_policy(AUTO)


def test_side_streams_are_probed_for_real_concurrency(gpu):
    """fiveeqscm_amd/tuning.py: the side streams of the two-stream schedules are probed with a pair of one-wave launches of known
    duration (fiveeq_busy): what the picker returns runs beside the caller's stream and beside each other; the choice is made
    once per caller's stream; a stream is never concurrent with itself; the probe kernel validates its bound."""
    from fiveeqscm_amd import _capi, tuning
    lib = _capi.load()
    main = torch.cuda.current_stream(gpu)
    picked = tuning.concurrent_side_streams(lib, main, 2, probe=True)
    rep = tuning.side_stream_report(main)
    assert rep["probed"] and rep["passed"][:2] == [True, True] and rep["candidates_tried"] >= 2 and rep["probe_enabled"]
    assert len(picked) == 2 and len({main.cuda_stream, picked[0].cuda_stream, picked[1].cuda_stream}) == 3
    assert tuning.streams_concurrent(lib, main, picked[0]) and tuning.streams_concurrent(lib, main, picked[1])
    assert tuning.streams_concurrent(lib, picked[0], picked[1])
    assert not tuning.streams_concurrent(lib, main, main)
    again = tuning.concurrent_side_streams(lib, main, 1)                     # run()'s form: the cache, no probe, no synchronise
    assert again[0].cuda_stream == picked[0].cuda_stream
    other = torch.cuda.Stream()
    # a stream nobody probed: run() gets plain side streams for it and never clocks anything (the probe used to
    # synchronise the caller's stream inside an asynchronous API) ...
    calls, real = [], tuning.streams_concurrent
    tuning.streams_concurrent = lambda *a, **k: calls.append(a) or real(*a, **k)
    try:
        plain = tuning.concurrent_side_streams(lib, other, 1)
        assert not calls and tuning.side_stream_report(other) == {"probed": False, "passed": [None], "candidates_tried": 0,
                                                                  "probe_enabled": True}
        assert plain[0].cuda_stream != other.cuda_stream
        # ... nor does a capturing stream or FIVEEQ_SIDE_STREAM_PROBE=0, even when asked to probe
        cap = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=cap):
            tuning.concurrent_side_streams(lib, cap, 1, probe=True)
        os.environ["FIVEEQ_SIDE_STREAM_PROBE"] = "0"
        try:
            off = torch.cuda.Stream()
            tuning.concurrent_side_streams(lib, off, 1, probe=True)
            assert tuning.side_stream_report(off)["probe_enabled"] is False and not tuning.side_stream_report(off)["probed"]
        finally:
            del os.environ["FIVEEQ_SIDE_STREAM_PROBE"]
        assert not calls
    finally:
        tuning.streams_concurrent = real
    # ... until somebody asks for the probe where a synchronise is harmless (EnsembleEngine.probe_streams)
    mine = tuning.concurrent_side_streams(lib, other, 1, probe=True)
    assert tuning.side_stream_report(other)["probed"] and tuning.side_stream_report(other)["passed"] == [True]
    assert mine[0].cuda_stream != other.cuda_stream and tuning.streams_concurrent(lib, other, mine[0])
    out = torch.zeros(1, dtype=torch.float64, device=gpu)
    assert lib.fiveeq_busy(10, ctypes.c_void_p(out.data_ptr()), None) == _capi.OK
    torch.cuda.synchronize()
    assert 0.0 < out.item() < 1.0
    assert lib.fiveeq_busy(10**9, ctypes.c_void_p(out.data_ptr()), None) == _capi.E_INVALID
    assert lib.fiveeq_busy(-1, ctypes.c_void_p(out.data_ptr()), None) == _capi.E_INVALID
    # no candidate passes (a profiler that serialises kernels, a busy card): the last one is taken as it is — only overlap is lost
    probe, tuning.streams_concurrent = tuning.streams_concurrent, lambda *a, **k: False
    try:
        lonely = torch.cuda.Stream()
        got = tuning.concurrent_side_streams(lib, lonely, 1, probe=True)
        assert len(got) == 1 and got[0].cuda_stream != lonely.cuda_stream
        failed = tuning.side_stream_report(lonely)                # ... and the failed probe is on record, not silent
        assert failed["probed"] and failed["passed"] == [False] and failed["candidates_tried"] == tuning._PROBE_CANDIDATES
    finally:
        tuning.streams_concurrent = probe
    # and the engine uses them
    eng = _engine(prm.sample_ensemble(prm.default_params("multigas"), 4096), 4096, emi.rcp_like_emissions(20, 3), per_step_streams=2)
    assert [s.cuda_stream for s in eng.per_step_stream_list()] == [main.cuda_stream, picked[0].cuda_stream]
    assert eng.side_stream_report() == {"wanted": 1, "probed": True, "passed": [True], "probe_enabled": True,
                                        "candidates_tried": tuning.side_stream_report(main)["candidates_tried"]}
    eng.close()
    # the cache is shared by host threads (the C ABI advertises multi-threaded use): eight threads asking at once get one answer
    import threading
    shared, seen = torch.cuda.Stream(), []
    ths = [threading.Thread(target=lambda: seen.append(tuple(s.cuda_stream for s in tuning.concurrent_side_streams(lib, shared, 2))))
           for _ in range(8)]
    [t.start() for t in ths], [t.join() for t in ths]
    assert len(set(seen)) == 1 and len(seen) == 8


def test_calibrate_measures_the_box_dependent_constants(gpu):
    """engine.calibrate(): the launch boundary and the streaming ceiling the schedules are derived from, measured with the
    per-step kernel on this box instead of taken from the baked-in MI355X figures (review: constants baked into auto_k_steps)."""
    from fiveeqscm_amd import engine as eng_mod
    before = (eng_mod.HBM_STREAM_BYTES_PER_S, eng_mod.LAUNCH_BOUNDARY_S)
    got = eng_mod.calibrate(apply=False)
    assert (eng_mod.HBM_STREAM_BYTES_PER_S, eng_mod.LAUNCH_BOUNDARY_S) == before
    assert 0.5e-6 < got["launch_boundary_s"] < 2e-5, got
    assert 2e12 < got["hbm_stream_bytes_per_s"] < 9e12, got
    try:
        eng_mod.calibrate(members=500_000)
        assert eng_mod.LAUNCH_BOUNDARY_S != before[1] or eng_mod.HBM_STREAM_BYTES_PER_S != before[0]
        p = prm.sample_ensemble(prm.default_params("co2"), 1000)
        eng = _engine(p, 1000, emi.rcp_like_emissions(10, 1))
        assert 2 <= eng.auto_k_steps() <= 128                      # a 1000-member ensemble stays launch-bound on any box
        eng.close()
    finally:
        eng_mod.HBM_STREAM_BYTES_PER_S, eng_mod.LAUNCH_BOUNDARY_S = before


def test_fused_span_relaunch_is_bit_identical(gpu, monkeypatch):
    """mode='fused' as launches of fused_span steps (the engine's choice for ensembles of few rounds of waves: a long launch
    ends in a long tail behind the SIMD's oldest-first arbitration) gives the bits of ONE launch: state, stored rows, wave records."""
    from fiveeqscm_amd import engine as eng_mod
    N, n_steps = 5000, 300
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    E = emi.rcp_like_emissions(n_steps, 3)
    monkeypatch.setattr(eng_mod, "FUSED_SPAN_MIN_ROUNDS", 0.0)            # 5000 members are 2 % of a round: let "auto" relaunch them
    for dtype in (torch.float64, torch.float32):
        ref = _engine(p, N, E, dtype=dtype, collect_stats=True, fused_span=None)
        assert ref.fused_span_steps(n_steps) == n_steps
        ref.run(mode="fused")
        for span in ("auto", 7, 128, 1000):
            eng = _engine(p, N, E, dtype=dtype, collect_stats=True, fused_span=span)
            want = {"auto": eng_mod.FUSED_SPAN_STEPS, 7: 7, 128: 128, 1000: n_steps}[span]
            assert eng.fused_span_steps(n_steps) == want and eng.fused_span_steps(5) == min(want, 5)
            eng.run(0, 100, mode="fused")
            eng.run(100, n_steps, mode="fused")
            torch.cuda.synchronize()
            for name in ("R", "S", "C", "T", "T_stats"):
                assert torch.equal(getattr(eng, name), getattr(ref, name)), (dtype, span, name)
            assert eng.bytes_per_member_step("fused") >= ref.bytes_per_member_step("fused")
            eng.close()
        ref.close()
    big = _engine(p, N, E, fused_span="auto")
    monkeypatch.setattr(eng_mod, "FUSED_SPAN_MAX_ROUNDS", 0.0)            # an ensemble of "many rounds": one launch
    assert big.fused_span_steps(n_steps) == n_steps
    monkeypatch.setattr(eng_mod, "FUSED_SPAN_MAX_ROUNDS", 8.0)
    monkeypatch.setattr(eng_mod, "FUSED_SPAN_MIN_ROUNDS", 1.0)            # ... and one too small to be worth relaunching
    assert big.fused_span_steps(n_steps) == n_steps
    big.close()
    with pytest.raises(ValueError):
        _engine(p, N, E, fused_span=0)


def test_auto_with_histograms_picks_what_the_measured_table_says(gpu):
    """profiles/r04/auto_hist_table.json: on a launch-bound ensemble the streamed pipeline (mode 'fused') fills T_hist 2-4x
    faster than per-step + bins (and than round 4's tiled kernel at the auto K), so that is what mode='auto' resolves to on an
    engine with hist=; a bandwidth-bound ensemble keeps the per-step kernel (the north-star form).  Whatever it picks, the
    results are those of the explicit per-step run, bit for bit."""
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "r04", "auto_hist_table.json")) as fh:
        table = json.load(fh)
    for dt in ("f64", "f32"):
        for nb in ("4096", "1024"):
            for n in ("10000", "100000"):
                row = table[dt][nb][n]
                assert row["auto_k_steps"] > 1
                others = [v for k, v in row.items() if k != "auto_k_steps" and k != "fused+bin ring"]
                assert row["fused+bin ring"] < min(others), (dt, nb, n, row)
    n_steps = 90
    E = emi.rcp_like_emissions(n_steps, 3)
    for N, want_mode in ((20_000, "fused"), (1_000_000, "per_step")):
        p = prm.sample_ensemble_shard(prm.default_params("multigas"), N, device="cuda:0")
        a = _engine(p, N, E, hist=(-1.0, 6.0, 1024), hist_ring_steps=32)
        assert (a.auto_k_steps() > 1) == (want_mode == "fused")
        a.run(mode="auto")
        assert a.last_mode == want_mode
        b = _engine(p, N, E, hist=(-1.0, 6.0, 1024), hist_ring_steps=32)
        b.run(mode="per_step")
        torch.cuda.synchronize()
        assert torch.equal(a.T_hist, b.T_hist) and torch.equal(a.T, b.T) and torch.equal(a.C, b.C) and torch.equal(a.R, b.R)
        assert int(a.T_hist.sum()) == N * n_steps
        a.close(), b.close()
        del a, b


def test_summaries_in_a_checkpoint_cover_only_the_steps_the_engine_has_moments_for(gpu):
    """state_dict('summaries') marks a step's moments valid only if this engine ran the step (or a checkpoint brought its
    moments): a run that starts late, or follows a state-only checkpoint, must not save the zero-filled records of the steps
    before it as real moments (advisor, round 3)."""
    N, n_steps = 3000, 60
    p = prm.sample_ensemble(prm.default_params("multigas"), N)
    E = emi.rcp_like_emissions(n_steps, 3)
    whole = _engine(p, N, E, collect_stats=True, store_trajectory=False)
    whole.run(0, 40)
    want = whole.stats_sums(0, 40).cpu().numpy()
    late = _engine(p, N, E, collect_stats=True, store_trajectory=False)
    late.load_state_dict(whole.state_dict(include_outputs=False))          # state only: no moments of steps [0, 40)
    late.run(40, n_steps)
    ck = late.state_dict()
    assert ck["_step_sums_valid"].tolist() == [False] * 40 + [True] * 20 and not ck["_step_sums"][:40].any()
    whole.run(40, n_steps)
    np.testing.assert_array_equal(ck["_step_sums"][40:], whole.stats_sums(40, n_steps).cpu().numpy())
    full = whole.state_dict()
    assert full["_step_sums_valid"].all()
    np.testing.assert_array_equal(full["_step_sums"][:40], want)
    third = _engine(p, N, E, collect_stats=True, store_trajectory=False)
    third.load_state_dict(whole.state_dict())                               # summaries travel: the loader has all 60 steps
    assert third.state_dict()["_step_sums_valid"].all()
    fresh = _engine(p, N, E, collect_stats=True, store_trajectory=False)
    fresh.run(10, 20)
    assert fresh.state_dict()["_step_sums_valid"].tolist() == [False] * 10 + [True] * 10 + [False] * 40
    for e in (whole, late, third, fresh):
        e.close()


def test_step_and_the_readers_join_an_unjoined_run(gpu):
    """run(..., join=False) leaves work on the side streams; step() and the readers (stats_sums, T_histogram,
    hist_edge_counts) must wait for it themselves, and step() must drop folded moments of the step it overwrites."""
    N, n_steps = 600_000, 40
    p = prm.sample_ensemble_shard(prm.default_params("multigas"), N, device="cuda:0")
    E = emi.rcp_like_emissions(n_steps, 3)
    a = _engine(p, N, E, collect_stats=True, per_step_streams=2)
    assert len(a.per_step_stream_list()) == 2
    a.run(0, 30, join=False)
    assert a._ps_unjoined
    for t in range(30, n_steps):
        a.step(t)                                        # joins first: the side stream's part of R, S is complete
    assert not a._ps_unjoined
    b = _engine(p, N, E, collect_stats=True, per_step_streams=1)
    b.run()
    torch.cuda.synchronize()
    for name in ("C", "T", "R", "S"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.stats_sums(), b.stats_sums())
    a.reset_state()
    a.run(0, n_steps, join=False)
    sums = a.stats_sums()                                # a reader right behind an unjoined run
    h = a.T_histogram(-1.0, 6.0, 256)
    assert not a._ps_unjoined and torch.equal(sums, b.stats_sums()) and torch.equal(h, b.T_histogram(-1.0, 6.0, 256))
    a._step_sums_valid[5] = True                         # pretend a streamed pass left folded moments for step 5
    a._step_sums[5] = -1.0
    a.reset_state()
    for t in range(6):
        a.step(t)
    assert not a._step_sums_valid[5] and torch.equal(a.stats_sums(0, 6), b.stats_sums(0, 6))
    a.close(), b.close()


def test_a_reader_on_another_stream_joins_the_streams_of_the_unjoined_run(gpu):
    """run(..., stream=s1, join=False) leaves work on s1 AND on s1's side streams; a reader that runs on
    the default stream (stats_sums, reset_state, load_state_dict, a later run on another main) must wait for exactly THOSE
    streams — round 5 re-derived the side streams from the reader's stream and waited for the wrong ones, a silent race.  The
    engine now remembers the stream list of the unjoined run.  A long busy kernel in front of the run on s1 makes the race wide
    enough to see: without the join the reader would see zero state."""
    from fiveeqscm_amd import _capi
    lib = _capi.load()
    N, n_steps = 600_000, 30
    p = prm.sample_ensemble_shard(prm.default_params("multigas"), N, device="cuda:0")
    E = emi.rcp_like_emissions(n_steps, 3)
    b = _engine(p, N, E, collect_stats=True, per_step_streams=1)
    b.run()
    torch.cuda.synchronize()
    want = b.stats_sums()
    a = _engine(p, N, E, collect_stats=True, per_step_streams=2)
    s1 = torch.cuda.Stream()
    a.probe_streams(s1)
    assert a.side_stream_report(s1)["probed"]
    scratch = torch.zeros(1, dtype=torch.float64, device=gpu)
    default = torch.cuda.current_stream(gpu)
    for reader in ("stats_sums", "run_on_default", "state_dict_roundtrip", "reset_state"):
        a.reset_state()
        torch.cuda.synchronize()
        s1.wait_stream(default)
        assert lib.fiveeq_busy(3_000_000, ctypes.c_void_p(scratch.data_ptr()), ctypes.c_void_p(s1.cuda_stream)) == _capi.OK   # ~10 ms
        a.run(0, n_steps if reader != "run_on_default" else 20, stream=s1, join=False)
        assert a._ps_unjoined and [s.cuda_stream for s in a._ps_unjoined] == [s.cuda_stream for s in a.per_step_stream_list(s1)]
        if reader == "stats_sums":
            got = a.stats_sums()                                  # on the DEFAULT stream
            assert a._ps_unjoined is None and torch.equal(got, want)
        elif reader == "run_on_default":
            a.run(20, n_steps)                                    # another main: ordered behind s1 and s1's side stream
            torch.cuda.synchronize()
            for name in ("C", "T", "R", "S"):
                assert torch.equal(getattr(a, name), getattr(b, name)), name
        elif reader == "state_dict_roundtrip":
            sd = b.state_dict()
            a.load_state_dict(sd)                                 # must not be overwritten by the late kernels of the unjoined run
            torch.cuda.synchronize()
            assert torch.equal(a.R, b.R) and torch.equal(a.S, b.S) and a._ps_unjoined is None
        else:
            a.reset_state()
            torch.cuda.synchronize()
            assert int(a.R.abs().sum()) == 0 and int(a.S.abs().sum()) == 0
    a.close(), b.close()


def test_per_step_histograms_use_a_one_slot_bin_ring(gpu):
    N, n_steps = 50_000, 40
    p = prm.sample_ensemble_shard(prm.default_params("multigas"), N, device="cuda:0")
    E = emi.rcp_like_emissions(n_steps, 3)
    a = _engine(p, N, E, hist=(-1.0, 6.0, 512), hist_ring_steps=16, store_trajectory=False)
    a.run(mode="per_step")
    assert tuple(a._bins["buf"].shape) == (1, 16, N)     # half the ring of the double-buffered fused pipeline
    per_step = a.T_hist.clone()
    a.reset_state()
    a.run(mode="fused")
    assert tuple(a._bins["buf"].shape) == (2, 16, N) and torch.equal(a.T_hist, per_step)
    a.close()


def test_random_sequences_of_segments_modes_and_checkpoints(gpu):
    """30 random runs cut into 2-5 consecutive segments, every segment in another launch shape (per-step, fused, K-step,
    graph replay, auto — with hist= the forms that fill T_hist), one checkpoint somewhere on the way restored into a
    FRESH engine (reduced outputs or raw buffers), fp64 / fp32, stored concentrations or not: state, stored
    rows, histograms and per-step moments at the end must be those of ONE per-step run of the whole range."""
    rng = np.random.default_rng(404)
    for case in range(30):
        N = int(rng.choice([1, 63, 64, 65, 257, 1024, 2049, 5000, 20_011]))
        n_steps = int(rng.integers(20, 90))
        kind, G = (("multigas", 3), ("co2", 1))[int(rng.integers(0, 2))]
        td = (torch.float64, torch.float32)[int(rng.integers(0, 2))]
        with_hist = bool(rng.integers(0, 2))
        ring = int(rng.integers(0, 2))                                                   # (kept: the stream of random numbers)
        store_c = bool(rng.integers(0, 2))
        kw = dict(dtype=td, store_concentrations=store_c, collect_stats=True,
                  hist=(-0.5, float(rng.uniform(2.0, 6.0)), int(rng.choice([64, 1000, 4096]))) if with_hist else None,
                  hist_ring_steps=int(rng.integers(2, 20)))
        p = prm.sample_ensemble(prm.default_params(kind), N, seed=1000 + case)
        E = emi.rcp_like_emissions(750, G)[220:220 + n_steps] * float(rng.uniform(0.5, 2.0))
        ref = _engine(p, N, E, **kw)
        ref.run(mode="per_step")
        cuts = sorted(set([0, n_steps] + [int(v) for v in rng.integers(1, n_steps, size=int(rng.integers(1, 5)))]))
        modes = ["per_step", "fused", "auto"] if with_hist else ["per_step", "fused", "ksteps", "graph", "auto"]
        ck_at = int(rng.integers(1, len(cuts) - 1)) if len(cuts) > 2 else None            # checkpoint BEFORE this segment
        raw = bool(rng.integers(0, 2))
        eng, first_row, log = _engine(p, N, E, **kw), 0, []
        for i in range(len(cuts) - 1):
            if ck_at is not None and i == ck_at:
                state = eng.state_dict(include_outputs=True if raw else "summaries")
                eng.close()
                eng = _engine(p, N, E, **kw)
                eng.load_state_dict(state)
                first_row = 0 if raw else cuts[i]                                     # "summaries" do not carry stored rows
                log.append(("checkpoint", "raw" if raw else "summaries", cuts[i]))
            mode = modes[int(rng.integers(0, len(modes)))]
            k = int(rng.integers(1, 12)) if mode == "ksteps" else None
            eng.run(cuts[i], cuts[i + 1], mode=mode, k_steps=k)
            log.append((mode, k, cuts[i], cuts[i + 1]))
        torch.cuda.synchronize()
        what = (case, N, n_steps, kind, td, kw["hist"], ring, store_c, log)
        assert torch.equal(eng.R, ref.R) and torch.equal(eng.S, ref.S), what
        assert torch.equal(eng.T[first_row:], ref.T[first_row:]), what
        if store_c:
            assert torch.equal(eng.C[first_row:], ref.C[first_row:]), what
        if with_hist:
            assert torch.equal(eng.T_hist, ref.T_hist), what
        a, b = eng.stats_sums(), ref.stats_sums()
        assert torch.equal(a[:, [0, 3, 4]], b[:, [0, 3, 4]]), what
        assert torch.allclose(a[:, 1:3], b[:, 1:3], rtol=1e-11, atol=1e-9), what
        assert eng.state_dict()["_step_sums_valid"].all(), what
        eng.close(), ref.close()
