"""The single-valued parameter rows on the GPU (include/fiveeq.h "SINGLE-VALUED PARAMETER ROWS"):
  1. the scan, against the NumPy rule on the integer view of every row, exactly;
  2. fiveeq_run_uniform_* against fiveeq_run_* on the same inputs, bit for bit, for every mask that matters;
  3. the masked rows are really not read (they hold NaN on the device during the uniform call);
  4. the engine: what it finds, and modes per_step / graph / fused against an engine built with uniform_rows=False.
Sizes: below, at and past one wave (64 members; 128 per packed wave), several workgroups, odd counts."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from fiveeqscm_amd import _capi  # noqa: E402
from fiveeqscm_amd import params as prm  # noqa: E402
from fiveeqscm_amd.emissions import make_drive, rcp_like_emissions  # noqa: E402

DEV = "cuda:0"
N_STEPS = 30
BENCH_MASK = (1 << 4) | (1 << 7) | (1 << 8)          # rC[1], rC[2], rT[2]: the rows bench.py's workload leaves single-valued
ROWS_CACHED, ROWS_STREAMED, ROWS_AUTO = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return _capi.load()


def _ptr(t, off=0):
    return ctypes.c_void_p(0 if t is None else t.data_ptr() + off)


def _bits(t):
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def _same(a, b):
    return torch.equal(a, b) and torch.equal(_bits(a), _bits(b))


# ---- 1. the scan --------------------------------------------------------------------------------------------------------------
KINDS = ("distinct", "one", "zero", "nan", "but_first", "but_last", "but_middle", "neg_zero")


def _scan_rows(np_dtype, n, ld, shift, rng):
    """[11, ld]: row i is of kind KINDS[(i + shift) % 8]; columns [n, ld) hold garbage."""
    word = np.int64 if np_dtype == np.float64 else np.int32
    rows = np.empty((11, ld), dtype=np_dtype)
    nan_bits = word(0x7FF8000000000123) if word is np.int64 else word(0x7FC00123)
    for i in range(11):
        kind = KINDS[(i + shift) % len(KINDS)]
        v = np_dtype(rng.uniform(0.5, 2.0))
        if kind == "distinct":
            rows[i, :n] = v + np.arange(n)
        elif kind == "zero" or kind == "neg_zero":
            rows[i, :n] = 0.0
            if kind == "neg_zero":
                rows[i, n // 2] = -0.0
        elif kind == "nan":
            rows[i, :n].view(word)[:] = nan_bits
        else:
            rows[i, :n] = v
            if kind != "one":
                rows[i, {"but_first": 0, "but_last": n - 1, "but_middle": n // 2}[kind]] = v * np_dtype(1.5)
        rows[i, n:].view(word)[:] = rng.integers(1, 2 ** 31 - 1, size=ld - n)
    return rows


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_scan_matches_the_numpy_rule(lib, sfx):
    np_dtype, word = (np.float64, np.int64) if sfx == "f64" else (np.float32, np.int32)
    rng = np.random.default_rng(16)
    fn = getattr(lib, f"fiveeq_uniform_rows_{sfx}")
    for n in (1, 63, 64, 65, 257, 1000):
        for shift in (0, 3):
            ld = n + 5
            rows = _scan_rows(np_dtype, n, ld, shift, rng)
            view = rows.view(word)
            want = (view[:, :n] == view[:, :1]).all(axis=1)
            dev = torch.from_numpy(rows).to(DEV)
            mask = ctypes.c_uint32(0xFFFFFFFF)
            vals = np.zeros(11, dtype=np_dtype)
            rc = fn(n, ld, 9, _ptr(dev), _ptr(dev[9]), ctypes.byref(mask), vals.ctypes.data_as(ctypes.c_void_p), None)
            _capi.check(lib, rc)
            assert mask.value == sum(1 << i for i in range(11) if want[i]), (n, shift, bin(mask.value), want)
            assert np.array_equal(vals.view(word), view[:, 0]), (n, shift)
            if n > 1:                                   # the sizes above 1 really tell the kinds apart
                kinds = [KINDS[(i + shift) % len(KINDS)] for i in range(11)]
                assert [k in ("one", "zero", "nan") for k in kinds] == list(want)


# ---- 2. and 3. the kernel -----------------------------------------------------------------------------------------------------
FORMS = {                                               # dtype, ld(n): fp32 packs with an even ld, cannot with an odd one
    "f64": (torch.float64, lambda n: n + 3),
    "f32_packed": (torch.float32, lambda n: (n + 3) // 2 * 2),
    "f32_scalar": (torch.float32, lambda n: (n + 2) | 1),
}


def _inputs(kind, dtype, n, ld, mask, rng):
    """Random parameter rows r [3G, ld], q [2, ld] around the set's own values, each row of `mask` holding one random value."""
    base = prm.default_params(kind)
    G = prm.n_gas_of(base)
    centre = np.array([np.asarray(base[k], dtype=np.float64).reshape(G)[g] for g in range(G) for k in ("r0", "rC", "rT")]
                      + list(base["q"]))
    rows = centre[:, None] * rng.uniform(0.8, 1.2, size=(3 * G + 2, ld)) + rng.uniform(0.0, 0.01, size=(3 * G + 2, ld))
    for k in range(3 * G + 2):
        if mask >> k & 1:
            rows[k, :] = rows[k, 0]
    rows = torch.from_numpy(rows).to(DEV, dtype)
    return G, rows[:3 * G].contiguous(), rows[3 * G:].contiguous()


def _run(lib, kind, dtype, n, ld, r, q, drive, mask=None, values=None):
    """30 steps from a zero state with stored rows and statistics; fiveeq_run_* (mask None) or fiveeq_run_uniform_*."""
    model = prm.make_model(prm.default_params(kind))
    G, SP = model.n_gas, sum(prm.pools_of(prm.default_params(kind)))
    sfx = "f64" if dtype == torch.float64 else "f32"
    R = torch.zeros((SP, ld), dtype=dtype, device=DEV)
    S = torch.zeros((2, ld), dtype=dtype, device=DEV)
    C = torch.zeros((N_STEPS, G, ld), dtype=dtype, device=DEV)
    T = torch.zeros((N_STEPS, ld), dtype=dtype, device=DEV)
    stats = torch.zeros(((n + 63) // 64, N_STEPS, 4), dtype=torch.float64, device=DEV)
    args = [ctypes.byref(model), n, ld, _ptr(drive), N_STEPS, 0, N_STEPS, _ptr(r), _ptr(q), _ptr(R), _ptr(S), _ptr(C), _ptr(T),
            N_STEPS, _ptr(stats)]
    if mask is None:
        rc = getattr(lib, f"fiveeq_run_{sfx}")(*args, None)
    else:
        rc = getattr(lib, f"fiveeq_run_uniform_{sfx}")(*args, mask, values, None)
    _capi.check(lib, rc)
    torch.cuda.synchronize()
    return {"R": R, "S": S, "C": C, "T": T, "T_stats": stats}


def _values(r, q, dtype):
    first = torch.cat([r[:, 0], q[:, 0]]).cpu().numpy()
    return first.ctypes.data_as(ctypes.c_void_p), first       # (keep `first` alive for the call)


def _masks(G):
    rows = 3 * G + 2
    out = [0] + [1 << k for k in range(rows)] + [(1 << rows) - 1]
    return out + [BENCH_MASK] if G == 3 else out              # the benchmark's rows exist in the three-gas layout only


@pytest.mark.parametrize("policy", [ROWS_CACHED, ROWS_STREAMED])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("kind", ["multigas", "co2"])
def test_uniform_run_is_the_plain_run_bit_for_bit(lib, kind, form, policy):
    dtype, ld_of = FORMS[form]
    rng = np.random.default_rng(1600 + policy)
    G = prm.n_gas_of(prm.default_params(kind))
    drive = torch.from_numpy(make_drive(rcp_like_emissions(N_STEPS, G))).to(DEV, dtype).contiguous()
    lib.fiveeq_set_row_policy(policy)
    try:
        for n in (1, 64, 65, 300, 1025):
            ld = ld_of(n)
            for mask in _masks(G):
                _, r, q = _inputs(kind, dtype, n, ld, mask, rng)
                vals, keep = _values(r, q, dtype)
                want = _run(lib, kind, dtype, n, ld, r, q, drive)
                got = _run(lib, kind, dtype, n, ld, r, q, drive, mask, vals)
                for name in want:
                    assert _same(got[name], want[name]), (kind, form, policy, n, hex(mask), name)
                assert bool(torch.isfinite(want["T"][:, :n]).all())      # a run worth comparing
                # 3. the rows are really not read: NaN in the masked device rows, the same outputs
                if mask in (BENCH_MASK, (1 << (3 * G + 2)) - 1):
                    r2, q2 = r.clone(), q.clone()
                    for k in range(3 * G + 2):
                        if mask >> k & 1:
                            (r2[k] if k < 3 * G else q2[k - 3 * G]).fill_(float("nan"))
                    got = _run(lib, kind, dtype, n, ld, r2, q2, drive, mask, vals)
                    for name in want:
                        assert _same(got[name], want[name]), ("masked rows were read", kind, form, policy, n, hex(mask), name)
                del keep
    finally:
        lib.fiveeq_set_row_policy(ROWS_AUTO)


# ---- 4. the engine ------------------------------------------------------------------------------------------------------------
def _engine_outputs(params, N, dtype, mode, uniform_rows, n_steps=40):
    from fiveeqscm_amd.engine import EnsembleEngine
    G = prm.n_gas_of(params)
    eng = EnsembleEngine(params, N, rcp_like_emissions(n_steps, G), dtype=dtype, device=DEV, collect_stats=True,
                         per_step_streams=2, uniform_rows=uniform_rows)
    found = eng.uniform_rows
    eng.run(0, n_steps, mode=mode)
    torch.cuda.synchronize()
    out = {"R": eng.R.clone(), "S": eng.S.clone(), "C": eng.C.clone(), "T": eng.T.clone(), "T_stats": eng.T_stats.clone()}
    split = len(eng.per_step_launches())
    eng.close()
    return found, out, split


def _two_gas(params):
    out = dict(params)
    for k in ("a", "tau", "r0", "rC", "rT", "ra", "PI_conc", "emis2conc", "f"):
        out[k] = params[k][:2]
    return out


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_engine_finds_the_rows_and_every_mode_matches(lib, dtype):
    for N in (2000, 600):                               # the two-stream split (halves of >= 512 members) and below it
        params = prm.sample_ensemble_shard(prm.default_params("multigas"), N, device=torch.device(DEV), dtype=dtype)
        for mode in ("per_step", "graph", "fused"):
            found, got, split = _engine_outputs(params, N, dtype, mode, "auto")
            none, want, _ = _engine_outputs(params, N, dtype, mode, False)
            assert found == ("rC[1]", "rC[2]", "rT[2]") and none == ()
            assert split == (2 if N >= 1024 else 1)
            for name in want:
                assert _same(got[name], want[name]), (N, mode, name)


def test_engine_without_single_valued_rows_and_the_fallback_layout(lib):
    dtype, N = torch.float64, 1100
    co2 = prm.sample_ensemble_shard(prm.default_params("co2"), N, device=torch.device(DEV), dtype=dtype)
    found, got, _ = _engine_outputs(co2, N, dtype, "per_step", "auto")
    _, want, _ = _engine_outputs(co2, N, dtype, "per_step", False)
    assert found == ()
    for name in want:
        assert _same(got[name], want[name]), name
    # pools 4 + 1: a compiled layout without the form — the rows are reported, the launches are the plain ones
    two = prm.sample_ensemble_shard(_two_gas(prm.default_params("multigas")), N, device=torch.device(DEV), dtype=dtype)
    for mode in ("per_step", "graph"):
        found, got, _ = _engine_outputs(two, N, dtype, mode, "auto")
        _, want, _ = _engine_outputs(two, N, dtype, mode, False)
        assert found == ("rC[1]",)
        for name in want:
            assert _same(got[name], want[name]), (mode, name)


def test_refresh_follows_an_overwritten_row(lib):
    from fiveeqscm_amd.engine import EnsembleEngine
    N = 300
    params = prm.sample_ensemble_shard(prm.default_params("multigas"), N, device=torch.device(DEV), dtype=torch.float64)
    eng = EnsembleEngine(params, N, rcp_like_emissions(8, 3), device=DEV)
    assert eng.uniform_rows == ("rC[1]", "rC[2]", "rT[2]")
    eng.r[4, 7] = 0.001                                 # rC[1]: no longer one value
    assert eng.refresh_uniform_rows() == ("rC[2]", "rT[2]")
    eng.run(0, 8)
    ref = EnsembleEngine(params, N, rcp_like_emissions(8, 3), device=DEV, uniform_rows=False)
    ref.r[4, 7] = 0.001
    ref.run(0, 8)
    torch.cuda.synchronize()
    assert _same(eng.T, ref.T) and _same(eng.C, ref.C)
    eng.close()
    ref.close()
