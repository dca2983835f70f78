"""Per-member minor-gas forcing rows on the MI355X (include/fiveeq.h "MINOR-GAS FORCING ROWS"): the C entry points into guarded
buffers against the NumPy twin fed the device primitive's own expm1 bits — exact, fp64 and fp32 — at every lane edge and member
class; invariance under row and member splits and species groups; into= on top of AR(1) noise; fp64 accuracy against a
50-digit evaluation; and the rows through EnsembleEngine(member_forcing=)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from fiveeqscm_amd import _capi, emissions
from fiveeqscm_amd import params as prm
from fiveeqscm_amd.engine import EnsembleEngine
from fiveeqscm_amd.forcing import ar1_noise_rows
from fiveeqscm_amd.minor_gases import minor_gas_rows, minor_gas_rows_host, step_minor_gases
import minor_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float64, torch.float32]
NP_OF = {torch.float64: np.float64, torch.float32: np.float32}
SENTINEL = -777.25
N_ROWS = 12
GUARD_ROWS = 2
LN2 = float(np.log(2.0))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _probe_em1(x):
    """fe_expm1_neg of fp64 x (any shape) as the device computes it: fiveeq_math_probe_f64(op = 0)."""
    lib = _capi.load()
    x_d = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).reshape(-1)).to(DEV)
    y_d = torch.empty_like(x_d)
    with torch.cuda.device(DEV):
        _capi.check(lib, lib.fiveeq_math_probe_f64(0, x_d.numel(), _ptr(x_d), _ptr(y_d), _stream()))
    torch.cuda.synchronize()
    return y_d.cpu().numpy().reshape(np.shape(x))


def _em1_of(tau, npd, dt=1.0):
    """The device primitive at x = -dt / tau, x formed in NumPy from tau widened from the kernel precision first."""
    return _probe_em1(-dt / np.asarray(tau).astype(npd).astype(np.float64))


def _call(dtype, E, c, tau, eff, R, ld, start=None, dt=1.0):
    """One fiveeq_minor_rows_* call into guarded buffers of row length ld with GUARD_ROWS rows beyond n_rows: (rows
    [n_rows + GUARD_ROWS, ld], R [K, ld]) on the host.  start [n_rows, n]: what the rows hold before (accumulate = 1)."""
    lib = _capi.load()
    n_rows, K = E.shape
    n = tau.shape[1]

    def pad(a, dt_):
        out = torch.full((a.shape[0], ld), SENTINEL, dtype=torch.float64)
        out[:, :n] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
        return out.to(DEV, dt_)
    tau_d, eff_d, R_d = pad(tau, dtype), pad(eff, dtype), pad(R, torch.float64)
    rows = torch.full((n_rows + GUARD_ROWS, ld), SENTINEL, dtype=dtype, device=DEV)
    if start is not None:
        rows[:n_rows, :n] = torch.from_numpy(start).to(DEV, dtype)
    E_d = torch.from_numpy(np.ascontiguousarray(E, dtype=np.float64)).to(DEV)
    c_h = (ctypes.c_double * K)(*[float(v) for v in c])
    fn = getattr(lib, "fiveeq_minor_rows_" + ("f64" if dtype == torch.float64 else "f32"))
    with torch.cuda.device(DEV):
        _capi.check(lib, fn(K, n, ld, n_rows, dt, ctypes.cast(c_h, ctypes.c_void_p), _ptr(E_d), _ptr(tau_d), _ptr(eff_d), _ptr(R_d),
                            _ptr(rows), int(start is not None), _stream()))
    torch.cuda.synchronize()
    return rows.cpu().numpy(), R_d.cpu().numpy()


def _case(K, n, seed=0):
    """Emissions with negative years and a zero year, per-member tau and eff, R0 != 0."""
    rng = np.random.default_rng(1000 * K + n + seed)
    t = np.arange(N_ROWS)[:, None]
    E = rng.uniform(0.5, 3.0, (1, K)) * (1.0 + 0.1 * t) * np.where(rng.random((N_ROWS, K)) < 0.15, -0.3, 1.0)
    E[N_ROWS // 2] = 0.0
    tau = rng.uniform(1.5, 250.0, (K, 1)) * rng.uniform(0.7, 1.3, (K, n))
    eff = rng.uniform(0.01, 0.5, (K, 1)) * rng.uniform(0.8, 1.2, (K, n))
    c = rng.uniform(0.05, 0.4, K)
    R0 = rng.uniform(0.0, 5.0, (K, n))
    return E, tau, c, eff, R0


def _edge_lanes(n):
    return sorted({m for m in (0, 63, 64, n - 1) if 0 <= m < n})


def _with_member_classes(tau, eff, npd):
    """The member classes of the issue written over lanes 0, 63, 64 and the last one, a class per species row in turn: the
    clamp (tau = 1e-3: x = -1000 < -800, em1 = -1), the k = 0 branch (tau = 1e9), tau on both sides of x = -ln2/2 and of
    x = -3 ln2/2 (neighbours in the kernel precision), and eff = 0."""
    tau, eff = tau.copy(), eff.copy()
    K, n = tau.shape
    below = lambda v: float(np.nextafter(npd(v), npd(0)))                                # noqa: E731
    above = lambda v: float(np.nextafter(npd(v), npd(np.inf)))                           # noqa: E731
    classes = [1e-3, 1e9, below(2.0 / LN2), above(2.0 / LN2), below(2.0 / (3.0 * LN2)), above(2.0 / (3.0 * LN2))]
    for i, m in enumerate(_edge_lanes(n)):
        for k in range(K):
            tau[k, m] = classes[(i + k) % len(classes)]
        if K > 1 or m == 63:                         # (one species: a single lane without forcing, not every edge lane)
            eff[(i + 1) % K, m] = 0.0
    if n > 8:                                        # every class in some lane even for K = 1
        for j, v in enumerate(classes):
            tau[j % K, 1 + j] = v
    return tau, eff


# ---- exact bits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_rows_equal_the_twin_on_the_device_expm1_and_leave_the_guards(n, K, dtype):
    npd = NP_OF[dtype]
    E, tau, c, eff, R0 = _case(K, n)
    tau, eff = _with_member_classes(tau, eff, npd)
    em1 = _em1_of(tau, npd)
    if n > 8:
        assert (em1 == -1.0).any() and (np.abs(em1) < 2e-9).any()                        # the clamp and the k = 0 branch are there
    want = minor_gas_rows_host(E, tau, c, eff, n, R0=R0, em1=em1, dtype=npd)
    for ld in (n, n + 7):
        rows, R = _call(dtype, E, c, tau, eff, R0, ld)
        assert rows.dtype == npd and np.array_equal(rows[:N_ROWS, :n], want.rows), ld
        assert np.array_equal(R[:, :n], want.R), ld
        assert (rows[N_ROWS:] == SENTINEL).all() and (rows[:, n:] == SENTINEL).all() and (R[:, n:] == SENTINEL).all(), ld
    assert np.isfinite(want.rows).all() and np.abs(want.rows).sum() > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_accumulate_starts_from_the_stored_rows(dtype):
    npd, K, n = NP_OF[dtype], 3, 65
    E, tau, c, eff, R0 = _case(K, n)
    start = np.random.default_rng(5).normal(0.0, 0.4, (N_ROWS, n)).astype(npd)
    em1 = _em1_of(tau, npd)
    into = start.copy()
    want = minor_gas_rows_host(E, tau, c, eff, n, R0=R0, em1=em1, into=into, dtype=npd)
    rows, R = _call(dtype, E, c, tau, eff, R0, n + 7, start=start)
    assert np.array_equal(rows[:N_ROWS, :n], want.rows) and np.array_equal(R[:, :n], want.R)
    assert (rows[N_ROWS:] == SENTINEL).all() and (rows[:, n:] == SENTINEL).all()


# ---- invariance -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_and_member_splits_give_the_same_bits(dtype):
    K, n = 3, 257
    E, tau, c, eff, R0 = _case(K, n)
    tau, eff = _with_member_classes(tau, eff, NP_OF[dtype])
    kw = dict(device=DEV, dtype=dtype)
    whole = minor_gas_rows(E, tau, c, eff, n, R0=R0, **kw)
    assert whole.rows.dtype == dtype and whole.rows.shape == (N_ROWS, n) and whole.R.shape == (K, n) and whole.species == K
    for cuts in ((5,), tuple(range(1, N_ROWS))):                                         # {5, 7} and 12 x {1}
        parts, R = [], R0
        for a, b in zip((0,) + cuts, cuts + (N_ROWS,)):
            out = minor_gas_rows(E[a:b], tau, c, eff, n, R0=R, **kw)
            parts.append(out.rows)
            R = out.R.cpu().numpy()
        assert torch.equal(torch.cat(parts), whole.rows) and torch.equal(out.R, whole.R), cuts
    for lo, hi in ((0, 100), (100, 257)):
        part = minor_gas_rows(E, tau, c, eff, n, lo, hi, R0=R0, **kw)
        assert torch.equal(part.rows, whole.rows[:, lo:hi]) and torch.equal(part.R, whole.R[:, lo:hi]), (lo, hi)
    assert minor_gas_rows(E, tau, c, eff, n, 7, 7, **kw).rows.shape == (N_ROWS, 0)
    assert minor_gas_rows(E[:0], tau, c, eff, n, **kw).rows.shape == (0, n)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [9, 17])
def test_more_than_eight_species_go_in_groups_like_the_twin(K, dtype):
    npd, n = NP_OF[dtype], 130
    E, tau, c, eff, R0 = _case(K, n)
    got = minor_gas_rows(E, tau, c, eff, n, R0=R0, device=DEV, dtype=dtype)
    want = minor_gas_rows_host(E, tau, c, eff, n, R0=R0, em1=_em1_of(tau, npd), dtype=npd)
    assert got.species == K and np.array_equal(got.rows.cpu().numpy(), want.rows) and np.array_equal(got.R.cpu().numpy(), want.R)
    if dtype == torch.float64:                       # fp64: the groups chain into ONE ordered sum (the scalar statement, ungrouped)
        one_sum, _ = ref.rows_scalar(E, c, tau, eff, R0, em1=_em1_of(tau, npd))
        assert np.array_equal(want.rows, np.array(one_sum))


def test_into_noise_rows_fp64():
    """into=ar1_noise_rows(...): the first product is added onto the stored fp64 noise value.  With ONE species that is
    noise + eff R, the very add of `noise + fresh rows` (a fresh run's 0.0 + p is p exactly): torch.equal.  With several species
    the sum runs ((noise + p0) + p1) + ..., which is not noise + ((p0 + p1) + ...) in floating point: those rows are held to
    the twin started from the same noise instead."""
    n = 257
    noise = ar1_noise_rows(n, N_ROWS, 0.4, 0.6, seed=11, device=DEV, dtype=torch.float64)
    E, tau, c, eff, R0 = _case(1, n)
    fresh = minor_gas_rows(E, tau, c, eff, n, R0=R0, device=DEV)
    into = noise.clone()
    out = minor_gas_rows(E, tau, c, eff, n, R0=R0, into=into)
    assert out.rows is into and torch.equal(into, noise + fresh.rows) and torch.equal(out.R, fresh.R)
    assert not torch.equal(into, noise)
    E, tau, c, eff, R0 = _case(9, n)
    into = noise.clone()
    minor_gas_rows(E, tau, c, eff, n, R0=R0, into=into)
    start = noise.cpu().numpy()
    want = minor_gas_rows_host(E, tau, c, eff, n, R0=R0, em1=_em1_of(tau, np.float64), into=start)
    assert np.array_equal(into.cpu().numpy(), want.rows)
    with pytest.raises(ValueError, match="into"):
        minor_gas_rows(E, tau, c, eff, n, into=noise[:, :100])
    with pytest.raises(ValueError, match="into"):
        minor_gas_rows(E, tau, c, eff, n, into=noise.float())


# ---- accuracy ---------------------------------------------------------------------------------------------------------------
def test_fp64_rows_against_fifty_digits(capsys):
    """|F - F_mp| <= 1e-10 max_t |F_mp| per member (the project's standing fp64 criterion), every member class included.
    The test prints the measured worst value; profiles/r29/NOTES.md records it."""
    K, n = 8, 65
    E, tau, c, eff, R0 = _case(K, n)
    tau, eff = _with_member_classes(tau, eff, np.float64)
    got = minor_gas_rows(E, tau, c, eff, n, R0=R0, device=DEV).rows.cpu().numpy()
    F = ref.rows_mp(E, c, tau, eff, R0)
    worst = 0.0
    for m in range(n):
        scale = max(abs(F[t][m]) for t in range(N_ROWS))
        assert scale > 0
        worst = max(worst, max(float(abs(float(got[t, m]) - F[t][m]) / scale) for t in range(N_ROWS)))
    with capsys.disabled():
        print(f"\nminor rows fp64: worst |F - F_mp| / max_t |F_mp| = {worst:.3e} over {n} members, K = {K}")
    assert worst <= 1e-10


# ---- through the engine -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _engine_case():
    N = 257
    p = prm.sample_ensemble_shard(prm.default_params("co2"), N)
    return N, p, emissions.rcp_like_emissions(N_ROWS, 1)


def _members(p, pick):
    """The parameter dict with the per-member rows r0, rC, rT, q replaced by pick(row) (the sampled TCR / ECS left out)."""
    return {k: (pick(np.asarray(v)) if k in ("r0", "rC", "rT", "q") else v) for k, v in p.items() if k not in ("TCR", "ECS")}


def _T(p, N, E, **kw):
    eng = EnsembleEngine(p, N, E, device=DEV, **kw)
    eng.run(mode="per_step")
    torch.cuda.synchronize()
    T = eng.T.cpu()
    eng.close()
    return T


def test_shared_parameters_through_the_engine_are_the_external_forcing_run():
    N, p, E = _engine_case()
    Em, tau, c, eff, _ = _case(3, 1)
    _, F = step_minor_gases(Em, tau[:, 0], c, eff[:, 0])
    rows = minor_gas_rows(Em, tau[:, 0], c, eff[:, 0], N, device=DEV).rows
    want = _T(p, N, E, F_ext=F).numpy()
    got = _T(p, N, E, member_forcing=rows).numpy()
    err = np.abs(got - want) / (1e-10 * np.abs(want) + 1e-13)
    assert np.isfinite(got).all() and err.max() <= 1.0, float(err.max())
    assert np.abs(want - _T(p, N, E).numpy()).max() > 1e-6                               # the minor gases do something


def test_distinct_members_through_the_engine_column_by_column():
    N, p, E = _engine_case()
    Em, tau, c, eff, _ = _case(3, N)
    rows = minor_gas_rows(Em, tau, c, eff, N, device=DEV).rows
    T = _T(p, N, E, member_forcing=rows)
    same = _T(_members(p, lambda v: np.repeat(v[:, :1], N, 1)), N, E, member_forcing=rows)
    assert (same[-1].max() - same[-1].min()).item() > 1e-6                               # identical members differ by their rows alone
    for m in (0, 63, 64, 256):
        assert torch.equal(_T(_members(p, lambda v: v[:, m:m + 1]), 1, E, member_forcing=rows[:, m:m + 1].contiguous())[:, 0], T[:, m]), m
