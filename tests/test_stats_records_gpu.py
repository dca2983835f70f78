"""Every per-wave statistics record the stepping kernels write, held to the exact per-record reference of
tests/stats_reference.py (bound gamma(20), derived there from the code; extrema and counts bit for bit).

INPUTS: stats_reference.pattern() in the slow thermal box of S0 (and a small per-member R0), so that T differs from member to
member from the first step: signs alternate, a record's magnitudes lie within a factor of 10, its extrema sit at known inner
lanes.  Every test asserts these properties on the T rows it got back (stats_reference.check_inputs) before it looks at a record.

ROUTES (the label a form's worst error-to-bound ratio is printed under):
    ladder          per_step / graph, one member per lane          packed ladder   fp32 per_step / graph, packed lanes
    flush           fused / ksteps, one member per lane            packed flush    fp32 fused / ksteps, packed lanes
    small tile      mode 'small' (4 lanes per member: one tile per workgroup of four waves; 1 lane: one tile per wave)
    inverse flush   the concentration-driven and mixed-drive kernels (one member per lane, the flush)

WHAT IS CHECKED: every record of every step of N in SIZES x layouts {4} and 4 + 1 + 1, n_steps = 19 (two full flush batches
and a ragged one), in every form of the table of FORMS below; the same records bit for bit without a stored trajectory;
resumed runs ([0, 5), [5, 13), [13, 19): batches that start mid-way) against the single run, with a sentinel in every slot a
segment must not touch; member sub-ranges of an ld = 330 allocation through the C ABI with the record pointer offset;
chunked schedules and a two-stream per-step run; the host folds stats() / stats_sums() against exact moments, in fp64 and fp32.

ALREADY PINNED ELSEWHERE, and left there: a NaN member's record (NaN sums, the extrema of the finite members) and the all-NaN
record's neutral extrema by every route — tests/test_step_edges_gpu.py (test_a_nan_member_touches_neither_its_neighbours_nor_
their_records, test_a_record_of_nan_members_only_has_the_neutral_extrema_by_every_route); packed == scalar and small == fused
bit for bit — tests/test_engine_gpu.py.

NOTES ON THE ISSUE'S CASES.  The engine rounds chunk_members down to a multiple of 256 (128 would switch chunking off) and
splits a launch over two streams from 1024 members on, so chunks of 128 members are driven through the C ABI here (a
chunk-major schedule by hand), the engine's own chunking runs with chunk_members=256, and the second stream comes into play
in a run of 1089 members with per_step_streams=2.  A sub-range's LAST record holds fewer members than the same record of the
whole run ([64, 194): members 192, 193), so it is held to the reference of its own members; the full records are the whole
run's bit for bit.  small_lanes=8 (the octet form) writes no records: with collect_stats the request is refused and 'auto' falls
back to one lane per member, which is what is checked.

MEASURED (MI355X): see the docstring of test_every_record_of_every_form.
"""
import functools

import numpy as np
import pytest

import stats_reference as sr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N_STEPS = 19
SIZES = [1, 63, 64, 65, 127, 128, 129, 191, 193, 255, 256, 257, 321]
KINDS = ("co2", "multigas")                       # pools {4} and 4 + 1 + 1
SENTINEL = -1.2345678e300
WORST = {}                                        # route -> [worst s1 ratio, worst s2 ratio] over the session, printed per test


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from fiveeqscm_amd import _capi
    return _capi.load()                           # the HIP library must be the thing that runs: no fallback


class _Packing:
    """fiveeq_set_f32_packing for the block, restored on exit."""

    def __init__(self, lib, on):
        self.lib, self.on = lib, int(on)

    def __enter__(self):
        self.lib.fiveeq_set_f32_packing(self.on)

    def __exit__(self, *exc):
        self.lib.fiveeq_set_f32_packing(1)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(kind, N):
    """Parameters [.., N], emissions, target concentrations, R0 [SP, N] and S0 [2, N] of the N-member ensemble."""
    from fiveeqscm_amd import params as prm
    base = prm.default_params(kind)
    G = len(np.atleast_1d(base["PI_conc"]))
    p = prm.sample_ensemble(base, N, seed=1000 + N)
    t = np.arange(N_STEPS, dtype=np.float64)[:, None]
    E = (np.array([0.5, 20.0, 1.0])[None, :G] * (1.0 + 0.05 * t))            # small: T stays the relaxing S0 pattern
    target = np.asarray(base["PI_conc"], dtype=np.float64).reshape(1, G) * (1.0 + 0.002 * (t + 1.0))
    SP = 4 + (G - 1)
    R0 = np.zeros((SP, N))
    first_pool = [0, 4, 5][:G]
    R0[first_pool] = (1.0 + 0.25 * (np.arange(N) % 7))[None, :] * np.array([1.0, 2.0, 0.5])[:G, None]
    S0 = np.stack([sr.pattern(N), np.zeros(N)])
    return dict(p=p, E=E, target=target, R0=R0, S0=S0, G=G)


def _sliced(kind, N, a, b):
    """Members [a, b) of the N-member ensemble as an ensemble of its own."""
    x = _inputs(kind, N)
    p = dict(x["p"])
    for k in ("r0", "rC", "rT", "q", "TCR", "ECS"):
        p[k] = np.ascontiguousarray(x["p"][k][..., a:b])
    return dict(x, p=p, R0=np.ascontiguousarray(x["R0"][:, a:b]), S0=np.ascontiguousarray(x["S0"][:, a:b]))


def _engine(x, N, drive="emissions", **kw):
    from fiveeqscm_amd.engine import EnsembleEngine, MixedDriveEngine
    kw = dict(dict(R0=x["R0"], S0=x["S0"], collect_stats=True, device="cuda:0"), **kw)
    if drive == "emissions":
        return EnsembleEngine(x["p"], N, x["E"], **kw)
    if drive == "scenarios":
        return EnsembleEngine(x["p"], N, np.stack([x["E"], 1.5 * x["E"], 0.25 * x["E"]]), **kw)
    if drive == "concentrations":
        return EnsembleEngine(x["p"], N, x["target"], concentration_driven=True, **kw)
    assert drive == "mixed"
    return MixedDriveEngine(x["p"], N, x["E"], x["target"], (1, 2), **kw)


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    word = {8: np.int64, 4: np.int32}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(word), b.view(word))


_REFS = {}


def _reference(T, first=0):
    """records() of rows T, with the inputs' properties asserted; cached by the rows' bits (the forms share their T)."""
    key = (T.dtype.str, T.shape, first, T.tobytes())
    if key not in _REFS:
        sr.check_inputs(T, first)
        _REFS[key] = sr.records(T)
    return _REFS[key]


def _check(stats, T, route, what, first=0):
    """stats [R, n, 4] against the reference of the rows T [n, members] (members first ..)."""
    ref = _reference(T, first)
    try:
        e1, e2 = sr.compare(stats, ref)
    except AssertionError as exc:
        raise AssertionError(f"{what}: {exc}") from exc
    w = WORST.setdefault(route, [0.0, 0.0])
    w[0], w[1] = max(w[0], e1), max(w[1], e2)
    assert e1 <= 1.0 and e2 <= 1.0, (what, route, e1, e2)


def _report():
    for route, (e1, e2) in sorted(WORST.items()):
        print(f"  {route:14s} worst |s1 - ref| / (gamma(20) abs1) = {e1:.4f}   |s2 - ref| / (gamma(20) s2_ref) = {e2:.4f}")


def _run_and_check(x, N, route, what, eng_kw, run_kw, drive="emissions"):
    """One run with stored T and one without: every record against the reference, the two T_stats equal bit for bit.
    Returns (T_stats, T) of the first."""
    eng = _engine(x, N, drive, **eng_kw)
    eng.run(**run_kw)
    stats, T = _host(eng.T_stats), _host(eng.T)
    eng.close()
    if drive == "scenarios":
        assert stats.shape[0] == T.shape[0] == 3
        assert not _same_bits(T[0], T[1]) and not _same_bits(T[0], T[2])
        for s in range(3):                        # every scenario against its OWN rows
            _check(stats[s], T[s], route, (*what, "scenario", s))
    else:
        _check(stats, T, route, what)
    bare = _engine(x, N, drive, store_trajectory=False, **eng_kw)
    bare.run(**run_kw)
    assert bare.T is None
    assert _same_bits(_host(bare.T_stats), stats), (*what, "without a stored trajectory")
    bare.close()
    return stats, T


MODES = [("per_step", {}), ("graph", {}), ("fused", {})] + [("ksteps", dict(k_steps=k)) for k in (1, 3, 8, 11)]


def _route(mode, packed):
    return ("packed " if packed else "") + ("ladder" if mode in ("per_step", "graph") else "flush")


# ---- every record of every form ---------------------------------------------------------------------------------------------------
FORMS = ("f64", "f32 packed", "f32 scalar", "small", "f32 compensated", "other drives")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_record_of_every_form(lib, kind, N, form):
    """f64 / f32 packed / f32 scalar: per_step, graph, fused, ksteps with k_steps 1, 3, 8, 11.  small: 4 and 1 lanes on {4},
    1 lane and the 'auto' fall-back from the octet on 4 + 1 + 1, both precisions.  f32 compensated: fused and small.  Other
    drives: concentration-driven (fp64, fp32), mixed drive and the scenario axis (3 scenarios, per_step and fused, packed fp32
    too).  Odd N runs fp32 scalar whatever the packing switch says (odd row strides), which the packed case then repeats.

    Worst error-to-bound ratios measured on the MI355X, 2026-10-21, over every test of this file (bound: 1; each test prints
    the running table):

        route            |s1 - ref| / (gamma(20) abs1)    |s2 - ref| / (gamma(20) s2_ref)
        ladder                    0.0168                           0.0866
        packed ladder             0.0000                           0.0852
        flush                     0.0174                           0.0866
        packed flush              0.0000                           0.0852
        small tile                0.0170                           0.0866
        inverse flush             0.0174                           0.1345

    (fp32 rows: a record's sum of 64 24-bit values is exact in fp64, hence the zeros.)  stats(): mean at most 0.0134 of its
    bound, var at most 0.1018 (test_host_folds_against_exact_moments prints both per case).  No case failed on a record; the
    one thing the tests brought up is the compensated form's resumed run, which is a trajectory of its own by design (see
    test_resumed_runs_write_the_same_records_and_no_other_slot)."""
    x = _inputs(kind, N)
    f64, f32 = torch.float64, torch.float32
    what = (kind, N, form)
    if form in ("f64", "f32 packed", "f32 scalar"):
        dtype, packing = (f64, 1) if form == "f64" else (f32, int(form == "f32 packed"))
        packed = dtype == f32 and packing == 1 and N % 2 == 0
        with _Packing(lib, packing):
            first = None
            for mode, kw in MODES:
                stats, T = _run_and_check(x, N, _route(mode, packed), (*what, mode, kw), dict(dtype=dtype), dict(mode=mode, **kw))
                first = T if first is None else first
                assert _same_bits(T, first), (*what, mode, kw, "T differs from the per-step run's")
    elif form == "small":
        for dtype in (f64, f32):
            lanes = (4, 1) if kind == "co2" else (1, "auto")
            for ln in lanes:
                eng_kw = dict(dtype=dtype, small_lanes=ln)
                probe = _engine(x, N, **eng_kw)
                assert probe.small_form() == (1 if ln == "auto" else ln)      # 'auto' with records: never the octet
                probe.close()
                _run_and_check(x, N, "small tile", (*what, dtype, ln), eng_kw, dict(mode="small"))
            if kind == "multigas":                # the octet form writes no records: the request is refused, nothing is written
                eng = _engine(x, N, dtype=dtype, small_lanes=8)
                assert eng.small_form() == 0
                with pytest.raises(ValueError):
                    eng.run(mode="small")
                eng.close()
    elif form == "f32 compensated":
        for mode, route in (("fused", "packed flush" if N % 2 == 0 else "flush"), ("small", "small tile")):
            _run_and_check(x, N, route, (*what, mode), dict(dtype=f32, compensated=True, small_lanes=1), dict(mode=mode))
    else:
        for dtype in (f64, f32):
            _run_and_check(x, N, "inverse flush", (*what, "concentrations", dtype), dict(dtype=dtype), {}, drive="concentrations")
            if kind == "multigas":
                _run_and_check(x, N, "inverse flush", (*what, "mixed", dtype), dict(dtype=dtype), {}, drive="mixed")
            for mode in ("per_step", "fused"):
                _run_and_check(x, N, _route(mode, dtype == f32 and N % 2 == 0), (*what, "scenarios", dtype, mode),
                               dict(dtype=dtype), dict(mode=mode), drive="scenarios")
    _report()


# ---- resumed runs ------------------------------------------------------------------------------------------------------------------
SEGMENTS = ((0, 5), (5, 13), (13, 19))            # 5 and 13: in the middle of a flush batch of the single run


def _resume_forms(kind):
    f64, f32 = torch.float64, torch.float32
    out = []
    for dtype in (f64, f32):
        out += [(f"{dtype} {mode} {kw}", "emissions", dict(dtype=dtype), dict(mode=mode, **kw))
                for mode, kw in MODES if mode != "graph"]
        out += [(f"{dtype} small {ln}", "emissions", dict(dtype=dtype, small_lanes=ln), dict(mode="small"))
                for ln in ((4, 1) if kind == "co2" else (1,))]
        out += [(f"{dtype} concentrations", "concentrations", dict(dtype=dtype), {}),
                (f"{dtype} scenarios fused", "scenarios", dict(dtype=dtype), dict(mode="fused"))]
        if kind == "multigas":
            out.append((f"{dtype} mixed", "mixed", dict(dtype=dtype), {}))
    out += [(f"compensated {mode}", "emissions", dict(dtype=f32, compensated=True, small_lanes=1), dict(mode=mode))
            for mode in ("fused", "small")]
    return out


@pytest.mark.parametrize("N", [129, 256, 321])
@pytest.mark.parametrize("kind", KINDS)
def test_resumed_runs_write_the_same_records_and_no_other_slot(lib, kind, N):
    """[0, 5), [5, 13), [13, 19) against the single run [0, 19): the same words at every slot, and — T_stats filled with a
    sentinel before each segment — not one slot of another step touched.  Every form that batches its records (fused, ksteps
    with k = 1, 3, 8, 11, small, concentration-driven, mixed, the scenario axis) and the per-step kernel.  The compensated
    form drops its compensation words at the end of every launch, so its resumed run is a trajectory of its own: each
    segment's records are held to the exact reference of the rows that segment stored, and the sentinels as for the others."""
    x = _inputs(kind, N)
    for label, drive, eng_kw, run_kw in _resume_forms(kind):
        whole = _engine(x, N, drive, **eng_kw)
        whole.run(0, N_STEPS, **run_kw)
        want = _host(whole.T_stats)
        whole.close()
        eng = _engine(x, N, drive, **eng_kw)
        eng._wave_stats()
        for a, b in SEGMENTS:
            eng.T_stats.fill_(SENTINEL)
            eng.run(a, b, **run_kw)
            got = _host(eng.T_stats)
            if "compensated" in label:            # its compensation words start at zero in every launch (include/fiveeq.h): a
                T = _host(eng.T)[a:b]             # resumed run is another trajectory, held to the reference of its OWN rows
                _check(got[:, a:b], T, "small tile" if "small" in label else "flush", (kind, N, label, (a, b)))
            else:
                assert _same_bits(got[..., a:b, :], want[..., a:b, :]), (kind, N, label, (a, b), "records differ from the single run's")
            rest = np.delete(got, np.arange(a, b), axis=-2)
            assert rest.size and np.all(rest == SENTINEL), (kind, N, label, (a, b), "a slot of another step was written")
        eng.close()


# ---- member sub-ranges through the C ABI -------------------------------------------------------------------------------------------
LD = 330
RANGES = ((64, 194), (128, 321))


def _abi_calls(lib, kind, sfx):
    """(label, route of a packed/scalar run, call(eng, t0, t1, m0, n)) of the entry points that take a member sub-range."""
    def plain(name, *extra):
        def call(eng, t0, t1, m0, n):
            eng._wave_stats()
            rc = getattr(lib, f"fiveeq_{name}_{sfx}")(*eng._run_args(t0, t1, m0, n), *extra, eng._stream())
            assert rc == 0, lib.fiveeq_last_error()
        return call
    flush, ladder = ("packed flush", "packed ladder") if sfx == "f32" else ("flush", "ladder")
    out = [("run", ladder, plain("run")), ("run_fused", flush, plain("run_fused")), ("run_ksteps 3", flush, plain("run_ksteps", 3)),
           ("run_small 1", "small tile", plain("run_small", 1))]
    if kind == "co2":
        out.append(("run_small 4", "small tile", plain("run_small", 4)))
    return out


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_member_sub_ranges_write_their_own_records_only(lib, kind, prec):
    """Members [64, 194) and [128, 321) of an ld = 330 allocation, T_stats offset by first_record * n_steps * 4 words (both
    ranges start at an even member: fp32 lanes stay packed, and the range's first record is the SECOND half of a packed wave
    in the whole run, the first half here).  Full records: the whole run's words bit for bit; the range's ragged last record
    (2 members, 1 member): the reference of its own members; every record outside the range keeps its sentinel, and so do the
    T rows of the members outside it.  Then the whole ensemble in chunks of 128 members by hand (a chunk-major schedule:
    every chunk runs all steps before the next starts): bit for bit the whole run's records."""
    x = _inputs(kind, LD)
    dtype = torch.float64 if prec == "f64" else torch.float32
    for label, route, call in _abi_calls(lib, kind, prec):
        whole = _engine(x, LD, dtype=dtype)
        call(whole, 0, N_STEPS, 0, LD)
        want, T_whole = _host(whole.T_stats), _host(whole.T)
        whole.close()
        _check(want, T_whole, route, (kind, prec, label, "whole"))
        for m0, m1 in RANGES:
            eng = _engine(x, LD, dtype=dtype)
            eng._wave_stats().fill_(SENTINEL)
            call(eng, 0, N_STEPS, m0, m1 - m0)
            got, T = _host(eng.T_stats), _host(eng.T)
            eng.close()
            what = (kind, prec, label, (m0, m1))
            assert _same_bits(T[:, m0:m1], T_whole[:, m0:m1]), (*what, "T rows")
            assert not T[:, :m0].any() and not T[:, m1:].any(), (*what, "T rows outside the range")
            r0, r_full, r1 = m0 // 64, m1 // 64, (m1 + 63) // 64
            assert _same_bits(got[r0:r_full], want[r0:r_full]), (*what, "full records")
            _check(got[r0:r1], T[:, m0:m1], route, what, first=m0)
            outside = np.concatenate([got[:r0], got[r1:]])
            assert outside.size and np.all(outside == SENTINEL), (*what, "a record outside the range was written")
        eng = _engine(x, LD, dtype=dtype)
        eng._wave_stats().fill_(SENTINEL)
        for m0 in range(0, LD, 128):
            call(eng, 0, N_STEPS, m0, min(128, LD - m0))
        assert _same_bits(_host(eng.T_stats), want), (kind, prec, label, "chunks of 128")
        eng.close()
    _report()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_chunked_and_two_stream_schedules_write_the_same_records(lib, dtype):
    """The engine's own chunk-major schedule (chunk_members=256 at 321 members: chunks of 256 and 65) and a per-step run whose
    launches are split over two streams (per_step_streams=2 at 1089 members: parts [0, 512) and [512, 1089)): every record
    against the reference, and bit for bit the unsplit run's."""
    for N, kw in ((321, dict(chunk_members=256, per_step_streams=1)), (1089, dict(chunk_members=None, per_step_streams=2))):
        x = _inputs("multigas", N)
        plain = _engine(x, N, dtype=dtype, chunk_members=None, per_step_streams=1)
        plain.run(mode="per_step")
        want = _host(plain.T_stats)
        plain.close()
        for mode in ("per_step", "graph"):
            eng = _engine(x, N, dtype=dtype, **kw)
            assert len(eng.per_step_launches()) == 2 and (N != 1089 or len(eng.per_step_stream_list()) == 2)
            eng.run(mode=mode)
            got, T = _host(eng.T_stats), _host(eng.T)
            eng.close()
            _check(got, T, "ladder", (N, dtype, mode, kw))
            assert _same_bits(got, want), (N, dtype, mode, kw)
    _report()


# ---- host folds ---------------------------------------------------------------------------------------------------------------------
def _check_moments(st, T, what):
    """stats() against exact moments of the rows: count, min, max exact; mean within gamma(20 + R) fsum|v| / N; var within
    err(s2) / N + 2 |mean| err(mean) + err(mean)^2 + gamma(5) s2_ref / N (stats_reference: THE HOST FOLDS).  Returns the worst
    (mean, var) error-to-bound ratios."""
    n_steps, N = T.shape
    R = (N + 63) // 64
    ex = sr.exact_moments(T)
    got = {k: _host(v) for k, v in st.items()}
    assert got["count"].tolist() == [float(N)] * n_steps, what
    assert _same_bits(got["min"], ex["min"]) and _same_bits(got["max"], ex["max"]), what
    e_mean = sr.gamma(20 + R) * ex["abs1"] / N
    e_var = sr.gamma(20 + R) * ex["s2"] / N + 2.0 * np.abs(ex["mean"]) * e_mean + e_mean ** 2 + sr.gamma(5) * ex["s2"] / N
    r_mean, r_var = np.abs(got["mean"] - ex["mean"]) / e_mean, np.abs(got["var"] - ex["var"]) / e_var
    assert r_mean.max() <= 1.0 and r_var.max() <= 1.0, (what, float(r_mean.max()), float(r_var.max()))
    return float(r_mean.max()), float(r_var.max())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("N", [1, 63, 65, 128, 193, 321])
@pytest.mark.parametrize("kind", KINDS)
def test_host_folds_against_exact_moments(lib, kind, N, dtype):
    worst = [0.0, 0.0]
    x = _inputs(kind, N)
    for mode in ("per_step", "fused", "small"):
        eng = _engine(x, N, dtype=dtype, small_lanes=1)
        eng.run(mode=mode)
        T = _host(eng.T).astype(np.float64)
        sr.check_inputs(T)
        r = _check_moments(eng.stats(), T, (kind, N, dtype, mode))
        worst = [max(a, b) for a, b in zip(worst, r)]
        eng.close()
    print(f"  stats() {kind} N={N} {dtype}: worst mean error / bound = {worst[0]:.4f}, var error / bound = {worst[1]:.4f}")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("cut", [64, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_half_ensembles_add_up_to_the_whole(lib, kind, cut, dtype):
    """stats_sums() of members [0, cut) and [cut, 321) run as ensembles of their own, added by hand: count, min and max equal
    the whole run's bit for bit; the sums lie within the bound of the exact sums of the whole run's rows (each side: gamma(20 +
    R) of fsum|v| resp. of the exact sum of squares, and one more addition here)."""
    N = 321
    x = _inputs(kind, N)
    for mode in ("per_step", "fused"):
        whole = _engine(x, N, dtype=dtype)
        whole.run(mode=mode)
        want, T = _host(whole.stats_sums()), _host(whole.T).astype(np.float64)
        whole.close()
        parts = []
        for a, b in ((0, cut), (cut, N)):
            eng = _engine(_sliced(kind, N, a, b), b - a, dtype=dtype)
            eng.run(mode=mode)
            assert _same_bits(_host(eng.T).astype(np.float64), T[:, a:b]), (kind, cut, dtype, mode, "members do not interact")
            parts.append(_host(eng.stats_sums()))
            eng.close()
        added = np.stack([parts[0][:, 0] + parts[1][:, 0], parts[0][:, 1] + parts[1][:, 1], parts[0][:, 2] + parts[1][:, 2],
                          np.minimum(parts[0][:, 3], parts[1][:, 3]), np.maximum(parts[0][:, 4], parts[1][:, 4])], axis=1)
        for col in (0, 3, 4):
            assert _same_bits(added[:, col], want[:, col]), (kind, cut, dtype, mode, col)
        ex = sr.exact_moments(T)
        R = (N + 63) // 64
        for got in (added, want):
            assert np.all(np.abs(got[:, 1] - ex["s1"]) <= sr.gamma(21 + R) * ex["abs1"]), (kind, cut, dtype, mode)
            assert np.all(np.abs(got[:, 2] - ex["s2"]) <= sr.gamma(21 + R) * ex["s2"]), (kind, cut, dtype, mode)
