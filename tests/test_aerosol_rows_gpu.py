"""Per-member aerosol forcing rows on the MI355X (include/fiveeq.h "AEROSOL FORCING ROWS"): the C entry points into guarded
buffers against the NumPy twin fed the device primitive's own logarithm bits — exact, fp64 and fp32 — at every lane edge, mask
and member class; accumulate and into= on top of AR(1) noise and of minor-gas rows; invariance under row and member splits;
fp64 accuracy against a 50-digit evaluation within the derived bound; the calibration helper against its twin; and the rows
through EnsembleEngine(member_forcing=)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from fiveeqscm_amd import _capi, emissions
from fiveeqscm_amd import params as prm
from fiveeqscm_amd.aerosols import aci_scale_for_target, aci_scale_for_target_host, aerosol_rows, aerosol_rows_host
from fiveeqscm_amd.engine import EnsembleEngine
from fiveeqscm_amd.forcing import ar1_noise_rows
from fiveeqscm_amd.minor_gases import minor_gas_rows
from oracle import fiveeq_oracle as npo
import aerosol_reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float64, torch.float32]
NP_OF = {torch.float64: np.float64, torch.float32: np.float32}
SENTINEL = -777.25
N_ROWS = ref.N_ROWS
GUARD_ROWS = 2
SQRT2 = float(np.sqrt(2.0))


def _ptr(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def probe_log(Y):
    """fe_log of fp64 Y (any shape) as the device computes it: fiveeq_math_probe_f64(op = 2)."""
    lib = _capi.load()
    x_d = torch.from_numpy(np.ascontiguousarray(Y, dtype=np.float64).reshape(-1)).to(DEV)
    y_d = torch.empty_like(x_d)
    with torch.cuda.device(DEV):
        _capi.check(lib, lib.fiveeq_math_probe_f64(2, x_d.numel(), _ptr(x_d), _ptr(y_d), _stream()))
    torch.cuda.synchronize()
    return y_d.cpu().numpy().reshape(np.shape(Y))


def _call(dtype, E, base, ari, shape, beta, in_aci, ld, start=None, null_cloud=False):
    """One fiveeq_aerosol_rows_* call into guarded buffers of row length ld with GUARD_ROWS rows beyond n_rows: rows
    [n_rows + GUARD_ROWS, ld] on the host.  start [n_rows, n]: what the rows hold before (accumulate = 1).  null_cloud: shape and
    beta are passed as NULL (a call without a cloud term)."""
    lib = _capi.load()
    n_rows, K = E.shape
    n = ari.shape[1]

    def pad(a):
        out = torch.full((a.shape[0], ld), SENTINEL, dtype=torch.float64)
        out[:, :n] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
        return out.to(DEV, dtype)
    ari_d, shape_d, beta_d = pad(ari), pad(shape), pad(beta[None])
    rows = torch.full((n_rows + GUARD_ROWS, ld), SENTINEL, dtype=dtype, device=DEV)
    if start is not None:
        rows[:n_rows, :n] = torch.from_numpy(start).to(DEV, dtype)
    E_d = torch.from_numpy(np.ascontiguousarray(E, dtype=np.float64)).to(DEV)
    b_h = (ctypes.c_double * K)(*[float(v) for v in base])
    mask = sum(1 << k for k in range(K) if in_aci[k])
    assert not (null_cloud and mask)
    fn = getattr(lib, "fiveeq_aerosol_rows_" + ("f64" if dtype == torch.float64 else "f32"))
    with torch.cuda.device(DEV):
        _capi.check(lib, fn(K, mask, n, ld, n_rows, ctypes.cast(b_h, ctypes.c_void_p), _ptr(E_d), _ptr(ari_d),
                            _ptr(None if null_cloud else shape_d), _ptr(None if null_cloud else beta_d), _ptr(rows),
                            int(start is not None), _stream()))
    torch.cuda.synchronize()
    return rows.cpu().numpy()


def _seen(out, ari, beta, classes, npd):
    """What the twin's y (and the parameters as the kernel reads them) show in each class lane: the set of properties."""
    seen = {}
    for m, (s_class, _) in classes.items():
        y, got = out.y[:, m], set()
        if (y == 1.0).any():
            got.add("y == 1")
        if ((y > 1.0) & (y - 1.0 < 1e-9)).any():
            got.add("y - 1 < 1e-9")
        if ((y > 1.0) & (y < SQRT2)).any() and ((y > SQRT2) & (y < 2.0)).any() and ((y > 2.0) & (y < 4.0)).any():
            got.add("y around sqrt(2) and 2")
        if (y > 1e6).any():
            got.add("y > 1e6")
        if npd(beta[m]) == 0:
            got.add("beta = 0")
        if npd(beta[m]) < 0:
            got.add("beta < 0")
        if (ari[:, m].astype(npd) == 0).all():
            got.add("ari of zeros")
        seen[m] = got
    return seen


EVERYTHING = {"y == 1", "y - 1 < 1e-9", "y around sqrt(2) and 2", "y > 1e6", "beta = 0", "beta < 0", "ari of zeros"}


# ---- exact bits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_rows_equal_the_twin_on_the_device_log_and_leave_the_guards(n, K, dtype):
    """Every mask of the issue, base == 0 and base != 0, ld = n and n + 7; the member classes rotate over the edge lanes (rot =
    0, 1, 2), and the twin's y shows that lanes 0, 63, 64 and the last each met every one of them."""
    npd = NP_OF[dtype]
    for in_aci in ref.masks(K):
        met = {m: set() for m in ref.edge_lanes(n)}
        for base_zero in (True, False):
            for rot in range(3):
                E, base, ari, shape, beta, classes = ref.case(K, n, in_aci, base_zero, rot)
                want = aerosol_rows_host(E, base, ari, shape, beta, n, aci=in_aci, log=probe_log, dtype=npd)
                for ld in (n, n + 7):
                    rows = _call(dtype, E, base, ari, shape, beta, in_aci, ld, null_cloud=not any(in_aci) and ld == n)
                    assert rows.dtype == npd and np.array_equal(rows[:N_ROWS, :n], want.rows), (in_aci, base_zero, rot, ld)
                    assert (rows[N_ROWS:] == SENTINEL).all() and (rows[:, n:] == SENTINEL).all(), (in_aci, base_zero, rot, ld)
                assert np.isfinite(want.rows).all() and (n < 9 or np.abs(want.rows).sum() > 0)   # (n < 9: class lanes only)
                if any(in_aci):
                    assert (want.y0 == 1.0).all() == base_zero and (base != 0).all() != base_zero
                    for m, got in _seen(want, ari, beta, classes, npd).items():
                        if m in met:
                            met[m] |= got
        if any(in_aci):
            assert all(got == EVERYTHING for got in met.values()), (in_aci, met)


@pytest.mark.parametrize("dtype", DTYPES)
def test_accumulate_starts_from_the_stored_rows(dtype):
    npd, K, n = NP_OF[dtype], 3, 65
    in_aci = [True, False, True]
    E, base, ari, shape, beta, _ = ref.case(K, n, in_aci, False)
    start = np.random.default_rng(5).normal(0.0, 0.4, (N_ROWS, n)).astype(npd)
    want = aerosol_rows_host(E, base, ari, shape, beta, n, aci=in_aci, into=start.copy(), log=probe_log, dtype=npd)
    rows = _call(dtype, E, base, ari, shape, beta, in_aci, n + 7, start=start)
    assert np.array_equal(rows[:N_ROWS, :n], want.rows) and not np.array_equal(want.rows, start)
    assert (rows[N_ROWS:] == SENTINEL).all() and (rows[:, n:] == SENTINEL).all()
    one = _call(dtype, E[:1], base, ari, shape, beta, in_aci, n + 7, start=start[:1])   # a single row: nothing to read ahead
    assert np.array_equal(one[:1, :n], want.rows[:1]) and (one[1:] == SENTINEL).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_into_noise_rows_and_minor_gas_rows_equals_the_twin(dtype):
    npd, K, n = NP_OF[dtype], 3, 257
    in_aci = [True, False, True]
    E, base, ari, shape, beta, _ = ref.case(K, n, in_aci, False)
    noise = ar1_noise_rows(n, N_ROWS, 0.4, 0.6, seed=11, device=DEV, dtype=dtype)
    rng = np.random.default_rng(8)
    minor = minor_gas_rows(rng.uniform(0.5, 3.0, (N_ROWS, 2)), rng.uniform(2.0, 200.0, (2, n)), [0.1, 0.3],
                           rng.uniform(0.01, 0.5, (2, n)), n, device=DEV, dtype=dtype).rows
    for under in (noise, minor):
        into = under.clone()
        out = aerosol_rows(E, base, ari, shape, beta, n, aci=in_aci, into=into, dtype=dtype)
        want = aerosol_rows_host(E, base, ari, shape, beta, n, aci=in_aci, into=under.cpu().numpy(), log=probe_log, dtype=npd)
        assert out.rows is into and out.species == K and np.array_equal(into.cpu().numpy(), want.rows)
        assert not torch.equal(into, under)
    with pytest.raises(ValueError, match="into"):
        aerosol_rows(E, base, ari, shape, beta, n, aci=in_aci, into=noise[:, :100], dtype=dtype)
    with pytest.raises(ValueError, match="into"):
        aerosol_rows(E, base, ari, shape, beta, n, aci=in_aci, into=noise.to(torch.float16), dtype=dtype)


# ---- invariance -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_and_member_splits_give_the_same_bits(dtype):
    K, n = 3, 257
    in_aci = [True, False, True]
    E, base, ari, shape, beta, _ = ref.case(K, n, in_aci, False)
    kw = dict(aci=in_aci, device=DEV, dtype=dtype)
    whole = aerosol_rows(E, base, ari, shape, beta, n, **kw)
    assert whole.rows.dtype == dtype and whole.rows.shape == (N_ROWS, n) and whole.species == K
    assert np.array_equal(whole.rows.cpu().numpy(),
                          aerosol_rows_host(E, base, ari, shape, beta, n, aci=in_aci, log=probe_log, dtype=NP_OF[dtype]).rows)
    for cuts in ((5,), tuple(range(1, N_ROWS))):                                         # {5, 7} and 12 x {1}
        parts = [aerosol_rows(E[a:b], base, ari, shape, beta, n, **kw).rows for a, b in zip((0,) + cuts, cuts + (N_ROWS,))]
        assert torch.equal(torch.cat(parts), whole.rows), cuts
    for lo, hi in ((0, 64), (64, 257), (0, 100), (100, 257)):
        part = aerosol_rows(E, base, ari, shape, beta, n, lo, hi, **kw)
        assert torch.equal(part.rows, whole.rows[:, lo:hi]), (lo, hi)
        shard = aerosol_rows(E, base, ari[:, lo:hi], shape[:, lo:hi], beta[lo:hi], n, lo, hi, **kw)
        assert torch.equal(shard.rows, part.rows), (lo, hi)
    assert aerosol_rows(E, base, ari, shape, beta, n, 7, 7, **kw).rows.shape == (N_ROWS, 0)
    assert aerosol_rows(E[:0], base, ari, shape, beta, n, **kw).rows.shape == (0, n)


# ---- accuracy ---------------------------------------------------------------------------------------------------------------
def test_fp64_rows_against_fifty_digits_within_the_derived_bound(capsys):
    """|F - F_mp| <= error_bound per member and step: the bound tests/aerosol_reference.py derives from the operation list (the
    CPU test's, test_fp64_twin_against_fifty_digits_within_the_derived_bound) with the logarithm's term widened from np.log's
    1 ulp to fe_log's pinned 2 ulp (test_device_math_primitives_within_two_ulp): c = 2 in 2 c u (|ln y| + |ln y0| + ...).  Every
    member class included.  The test prints the worst error / bound; profiles/r30/NOTES.md records it."""
    K, n = 8, 65
    worst = 0.0
    for in_aci in ref.masks(K)[1::2]:                                                    # every species, and alternating bits
        for rot in range(3):
            E, base, ari, shape, beta, _ = ref.case(K, n, in_aci, rot == 1, rot)
            got = aerosol_rows(E, base, ari, shape, beta, n, aci=in_aci, device=DEV).rows.cpu().numpy()
            F = ref.rows_mp(E, base, ari, shape, beta, in_aci)
            for m in range(n):
                for t in range(N_ROWS):
                    bound = ref.error_bound(E[t], base, ari[:, m], shape[:, m], beta[m], in_aci, log_ulps=2)
                    err = float(abs(got[t, m] - F[t][m]))
                    assert err <= bound, (in_aci, rot, t, m, err, bound)
                    worst = max(worst, err / bound if bound else 0.0)
    with capsys.disabled():
        print(f"\naerosol rows fp64: worst |F - F_mp| / bound = {worst:.3f} over {n} members, K = {K}")
    assert worst > 0


# ---- the calibration --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_calibration_equals_its_twin_and_is_the_same_for_one_shard_and_two(dtype):
    K, n = 3, 257
    in_aci = [True, False, True]
    E, base, ari, shape, _, _ = ref.case(K, n, in_aci, False)
    target = -np.random.default_rng(5).uniform(0.2, 1.6, n)
    kw = dict(aci=in_aci, device=DEV, dtype=dtype)
    beta = aci_scale_for_target(E, base, shape, target, (8, 12), n, **kw)
    want = aci_scale_for_target_host(E, base, shape, target, (8, 12), n, aci=in_aci, log=probe_log, dtype=NP_OF[dtype])
    assert beta.dtype == torch.float64 and beta.is_cuda and np.array_equal(beta.cpu().numpy(), want) and (want > 0).all()
    parts = [aci_scale_for_target(E, base, shape, target, (8, 12), n, lo, hi, **kw) for lo, hi in ((0, 100), (100, 257))]
    assert torch.equal(torch.cat(parts), beta)
    # the beta goes back in as it is, and the window mean of the cloud term is the target
    rows = aerosol_rows(E, base, np.zeros(K), shape, beta, n, **kw).rows
    mean = rows[8:12].double().mean(0).cpu().numpy()
    assert np.abs(mean - target).max() <= (1e-14 if dtype == torch.float64 else 1e-6) * np.abs(target).max()
    flat = E.copy()
    flat[8:12] = base
    with pytest.raises(ValueError, match="member 100: its cloud term averages to 0"):
        aci_scale_for_target(flat, base, shape, target, (8, 12), n, 100, 257, **kw)


# ---- through the engine -----------------------------------------------------------------------------------------------------
GASES = {"co2": 1, "multigas": 3}                 # pool layouts {4} and 4 + 1 + 1


@functools.lru_cache(maxsize=None)
def _engine_case(kind, N):
    p = prm.sample_ensemble_shard(prm.default_params(kind), N)
    return p, emissions.rcp_like_emissions(N_ROWS, GASES[kind])


def _run(p, N, E, mode, **kw):
    eng = EnsembleEngine(p, N, E, device=DEV, **kw)
    eng.run(mode=mode)
    torch.cuda.synchronize()
    out = {name: getattr(eng, name).cpu() for name in ("C", "T", "R", "S")}
    eng.close()
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", list(GASES))
def test_emissions_equal_to_base_are_the_run_without_rows_bit_for_bit(kind, dtype):
    N, K = 130, 3
    p, E = _engine_case(kind, N)
    in_aci = [True, False, True]
    _, base, ari, shape, beta, _ = ref.case(K, N, in_aci, False)
    rows = aerosol_rows(np.repeat(base[None], N_ROWS, 0), base, ari, shape, beta, N, aci=in_aci, device=DEV, dtype=dtype).rows
    assert bool((rows == 0).all()) and not bool(torch.signbit(rows).any())
    for mode in ("per_step", "fused"):
        want = _run(p, N, E, mode, dtype=dtype)
        got = _run(p, N, E, mode, dtype=dtype, member_forcing=rows)
        assert want["T"].abs().sum() > 0 and all(torch.equal(got[k], want[k]) for k in want), mode


@pytest.mark.parametrize("kind", list(GASES))
def test_real_rows_through_the_engine_against_the_oracle_member_by_member(kind):
    """Every stored T (and C) against the oracle's step run member by member on F_ext = the TWIN's rows of that member, at the
    tolerance test_member_forcing_gpu.py holds that comparison to: 1e-10 |ref| + 1e-13."""
    N, K = 65, 3
    p, E = _engine_case(kind, N)
    in_aci = [True, False, True]
    Em, base, ari, shape, beta, _ = ref.case(K, N, in_aci, False, with_classes=False)
    twin = aerosol_rows_host(Em, base, ari, shape, beta, N, aci=in_aci, log=probe_log).rows
    rows = aerosol_rows(Em, base, ari, shape, beta, N, aci=in_aci, device=DEV).rows
    assert np.array_equal(rows.cpu().numpy(), twin) and np.abs(twin).max() > 0.05
    G = GASES[kind]
    C_ref, T_ref = np.empty((N_ROWS, G, N)), np.empty((N_ROWS, N))
    for m in range(N):
        pm = dict(p)
        for k in ("r0", "rC", "rT", "q"):
            pm[k] = np.asarray(p[k])[:, m:m + 1]
        o = npo.run(E, pm, 1, F_ext=twin[:, m])
        C_ref[:, :, m], T_ref[:, m] = o["C"][:, :, 0], o["T"][:, 0]
    plain = _run(p, N, E, "per_step")
    for mode in ("per_step", "fused"):
        got = _run(p, N, E, mode, member_forcing=rows)
        for name, a, b in (("C", got["C"].numpy(), C_ref), ("T", got["T"].numpy(), T_ref)):
            err = np.abs(a - b) / (1e-10 * np.abs(b) + 1e-13)
            assert np.isfinite(a).all() and err.max() <= 1.0, (mode, name, float(err.max()))
        assert np.abs(got["T"].numpy() - plain["T"].numpy()).max() > 1e-3                 # the rows do something
