"""The kernels everything else is measured WITH, held to bits: the three bandwidth-yardstick copies (stream_copy_kernel,
stream_copy_wide_kernel, stream_copy_nt_kernel: every element, its bit pattern, nothing beside it, at every n where another loop
or branch of the kernel starts to run), busy_kernel's value, hfc_conc_kernel at the edges of its LDS tiles and lhs_kernel at the
edges of its Feistel domain — all through the C ABI.  References: the source itself, exact rational arithmetic, the library's
host twin and the NumPy twin, a 50-digit exp (tests/utility_reference.py).  Bytes only: rates belong to bench.py."""
import ctypes

import numpy as np
import pytest
import torch

from fiveeqscm_amd import _capi
from fiveeqscm_amd import params as prm
from utility_reference import bits, busy_chain, exp_neg_reference, strata, strata_slow, ulp_errors

pytestmark = pytest.mark.gpu

# The launch shapes of the copies, restated once (the library exports none of them); every size below derives from these.
BLOCK = 256                    # fiveeq_device.hpp:44    #define FIVEEQ_BLOCK 256
NARROW_CAP = 8192              # fiveeq_capi.hip:1306    fiveeq_stream_copy_f64: member_blocks(n) < 8192 ? member_blocks(n) : 8192
WIDE_CAP = 16384               # fiveeq_capi.hip:1278    fiveeq_stream_copy_wide_f64: blocks = tiles < 16384 ? tiles : 16384
TILE = 4 * BLOCK               # fiveeq_capi.hip:1277, 1294    4 * FIVEEQ_BLOCK: the wide copy's tile (double2) and the NT copy's (double)
S = NARROW_CAP * BLOCK         # the narrow copy's grid stride (elements) once its cap binds
G = WIDE_CAP * TILE            # double2 per sweep of the wide copy once its cap binds

GUARD = 1024                   # guard elements on either side of a destination
SENT = 0x7FF85EA71E55C0DE      # the sentinel: a NaN with a payload no kernel here produces; sources are redrawn where they hit it
I64 = torch.iinfo(torch.int64)


def _ptr(t, elements=0):
    return ctypes.c_void_p(t.data_ptr() + 8 * elements)


def _last_error(lib):
    return (lib.fiveeq_last_error() or b"").decode()


def _random_words(n, seed):
    """n random 64-bit patterns (signalling NaNs, payloads, -0.0, subnormals, infinities among them), none the sentinel."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.randint(I64.min, I64.max, (n,), dtype=torch.int64, device="cuda", generator=gen)
    while True:
        hit = w == SENT
        k = int(hit.sum())
        if k == 0:
            return w
        w[hit] = torch.randint(I64.min, I64.max, (k,), dtype=torch.int64, device="cuda", generator=gen)


def _copy_case(name, n, *, shift=0, stream=None):
    """One copy of n fp64 words, source and destination bases `shift` elements past a 16-byte boundary: the destination holds the
    source's bits, the guards on both sides the sentinel, the source what it held."""
    lib = _capi.load()
    fn = getattr(lib, name)
    words = _random_words(n + shift, 1000 + n % 997)
    src = words[shift:].view(torch.float64)                    # the kernels' view of it; compared as int64
    keep = words.clone()
    buf = torch.full((GUARD + shift + n + GUARD,), SENT, dtype=torch.int64, device="cuda")
    lo = GUARD + shift
    assert (buf.data_ptr() + 8 * lo) % 16 == 8 * (shift % 2) and src.data_ptr() % 16 == 8 * (shift % 2)
    torch.cuda.synchronize()                                   # the buffers are ready whichever stream the copy runs on
    rc = fn(n, _ptr(src), _ptr(buf, lo), None if stream is None else ctypes.c_void_p(stream.cuda_stream))
    assert rc == _capi.OK, (name, n, _last_error(lib))
    if stream is None:
        torch.cuda.synchronize()
    else:
        stream.synchronize()                                   # ONLY the stream it was handed: the launch must have gone there
    assert torch.equal(buf[lo:lo + n], words[shift:]), (name, n, "destination != source")
    assert bool((buf[:lo] == SENT).all()) and bool((buf[lo + n:] == SENT).all()), (name, n, "a guard element was written")
    assert torch.equal(words, keep), (name, n, "the source changed")


def _refused(name, n, *, src_off=0, dst_off=0, null=None):
    """The call must return E_INVALID with a message and leave the destination (n elements and guards, all allocated) alone."""
    lib = _capi.load()
    words = _random_words(max(n, 0) + 2, 77)
    buf = torch.full((GUARD + max(n, 0) + 2 + GUARD,), SENT, dtype=torch.int64, device="cuda")
    src = None if null == "src" else _ptr(words, src_off)
    dst = None if null == "dst" else _ptr(buf, GUARD + dst_off)
    torch.cuda.synchronize()
    rc = getattr(lib, name)(n, src, dst, None)
    torch.cuda.synchronize()
    assert rc == _capi.E_INVALID, (name, n, src_off, dst_off, null, rc)
    assert _last_error(lib), "a refusal without a message"
    assert bool((buf == SENT).all()), (name, n, "a refused call wrote to the destination")


# ---- 1. the three copies -------------------------------------------------------------------------------------------------
# one workgroup; the grid cap; the first n at which the unrolled loop runs (lane 0 only: 3S + 1); unrolled and tail iterations in one
# lane; two unrolled rounds
NARROW_SIZES = [1, 255, 256, 257, S - 1, S, S + 1, 3 * S, 3 * S + 1, 3 * S + 257, 4 * S, 4 * S + 1, 7 * S + 300, 8 * S + 1]
# a lone partial tile shorter / longer than one 256-stride; a whole tile; whole + partial; the grid cap; a second sweep of one
# element; a second sweep of one whole and one partial tile; a third sweep
WIDE_SIZES = [1, 255, 256, 257, 1023, 1024, 1025, 2047, G - 1, G, G + 1, G + TILE + 300, 2 * G + 1]
NT_SIZES = [TILE, 2 * TILE, TILE * 255, TILE * 256, TILE * 257, TILE * (NARROW_CAP + 1)]


def test_the_sizes_cross_every_path_of_the_copies():
    """The lists are written in terms of the caps; this pins what they are meant to cross (a changed cap moves both)."""
    assert (BLOCK, TILE) == (256, 1024) and WIDE_SIZES[4:8] == [TILE - 1, TILE, TILE + 1, 2 * TILE - 1]
    unrolled = [n for n in NARROW_SIZES if n > 3 * S]          # lane 0 enters the 4-in-flight loop from 3 S + 1 on
    assert unrolled[0] == 3 * S + 1 and 3 * S in NARROW_SIZES and any(n > 7 * S for n in unrolled)
    sweeps = [-(-n2 // G) for n2 in WIDE_SIZES]
    assert sorted(set(sweeps)) == [1, 2, 3]


@pytest.mark.parametrize("n", NARROW_SIZES)
def test_stream_copy_copies_every_element_and_nothing_else(n):
    _copy_case("fiveeq_stream_copy_f64", n)


def test_stream_copy_accepts_bases_that_are_only_8_byte_aligned():
    _copy_case("fiveeq_stream_copy_f64", 3 * S + 257, shift=1)


@pytest.mark.parametrize("n2", WIDE_SIZES)
def test_stream_copy_wide_copies_every_element_and_nothing_else(n2):
    _copy_case("fiveeq_stream_copy_wide_f64", 2 * n2)


@pytest.mark.parametrize("n", NT_SIZES)
def test_stream_copy_nt_copies_every_element_and_nothing_else(n):
    _copy_case("fiveeq_stream_copy_nt_f64", n)


@pytest.mark.parametrize("name,n", [("fiveeq_stream_copy_f64", 3 * S + 257), ("fiveeq_stream_copy_wide_f64", 2 * (G + TILE + 300)),
                                    ("fiveeq_stream_copy_nt_f64", TILE * 257)])
def test_the_copies_run_on_the_stream_they_are_handed(name, n):
    """The timing tools bracket these launches with events on their own stream: the result is checked after a synchronize of
    that stream alone."""
    _copy_case(name, n, stream=torch.cuda.Stream())


def test_stream_copy_wide_refuses_what_its_kernel_cannot_copy():
    name, n = "fiveeq_stream_copy_wide_f64", 2 * (TILE + 1)
    _refused(name, n + 1)                                      # odd
    _refused(name, 1)
    _refused(name, 0)
    _refused(name, n, src_off=1)                               # 8 bytes off a 16-byte boundary, either side
    _refused(name, n, dst_off=1)
    _refused(name, n, null="src")
    _refused(name, n, null="dst")


def test_stream_copy_nt_refuses_every_partial_tile():
    """stream_copy_nt_kernel returns from a tile it cannot copy whole: only the host's refusal keeps that from dropping data."""
    name = "fiveeq_stream_copy_nt_f64"
    for n in (0, 1, TILE - 1, TILE + 1, 3 * TILE + TILE // 2):
        _refused(name, n)
    _refused(name, TILE, null="src")
    _refused(name, TILE, null="dst")


def test_stream_copy_refuses_an_empty_copy_and_null_pointers():
    name = "fiveeq_stream_copy_f64"
    _refused(name, 0)
    _refused(name, BLOCK, null="src")
    _refused(name, BLOCK, null="dst")


# ---- 2. busy_kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [0, 1, 2, 7, 1000])
def test_busy_kernel_leaves_lane_zeros_chain(iters):
    """out[0] = x <- fma(x, 0.999999, 1e-9), `iters` times from 0.0, in exact IEEE fp64: one iteration more or fewer, or another
    lane's store (their chains start at 1e-9 * lane), are other bits."""
    lib = _capi.load()
    out = torch.full((2,), SENT, dtype=torch.int64, device="cuda")
    assert lib.fiveeq_busy(iters, _ptr(out), None) == _capi.OK, _last_error(lib)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[0] == bits(busy_chain(iters)), (iters, got[:1].view(np.float64)[0].hex(), busy_chain(iters).hex())
    assert got[1] == SENT, "busy_kernel wrote past out[0]"
    assert len({bits(busy_chain(k)).item() for k in (0, 1, 2, 6, 7, 8, 999, 1000, 1001)}) == 9     # neighbours do differ


# ---- 3. hfc_conc_kernel at its LDS-tile edges ---------------------------------------------------------------------------
# Worst error of the device exp(-t) against the 50-digit value over all the time grids below, measured on an MI355X (ROCm 7):
EXP_ULP_MEASURED = 0.7770
EXP_ULP_BOUND = min(2.0 * EXP_ULP_MEASURED, 2.0)              # twice the measurement, so another exp is seen; never past 2 ulp
_EXP_REF = {}


def _hfc_time(K):
    """K distinct times: an increasing grid over [-2, 30], shuffled — no two tile slots hold the same exp."""
    grid = np.linspace(-2.0, 30.0, K)
    assert np.all(np.diff(grid) > 0)
    t = np.random.default_rng(K).permutation(grid)
    if K not in _EXP_REF:
        _EXP_REF[K] = exp_neg_reference(t)
    return t, _EXP_REF[K]


@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("K", [1, 255, 256, 257, 511, 512, 513, 769])
def test_hfc_conc_at_the_tile_edges_to_the_bit(K, N):
    """out[k][m] = e0[m] * exp(-time[k]) with ld = N + 3.  The member with e0 = 1.0 holds d[k] = exp(-time[k]) itself; every other
    column must be the ONE rounded product e0[m] * d[k] (exact on the host: no libm in it), so a stale or foreign LDS entry,
    a wrong tile index or another member's e0 is another bit pattern.  d[k] against the 50-digit exp: the worst error measured
    over these eight grids on the MI355X is 0.7770 ulp (K = 256 and 511, t = 7.2862745...; per grid 0.20, 0.61, 0.78, 0.76, 0.78, 0.69, 0.76, 0.76), held in
    EXP_ULP_MEASURED; asserted at twice that, 1.554 ulp (never more than the 2 ulp of the golden test)."""
    lib = _capi.load()
    ld = N + 3
    time, ref = _hfc_time(K)
    rng = np.random.default_rng(1000 * K + N)
    e0 = rng.normal(size=N) * 10.0
    e0[:min(N, 4)] = [2.0, 0.0, -1.0, 3.0e-300][:min(N, 4)]
    one = N // 2
    e0[one] = 1.0
    out = torch.full((K * ld + 1,), SENT, dtype=torch.int64, device="cuda")
    d_e0, d_time = torch.from_numpy(e0).cuda(), torch.from_numpy(time).cuda()
    assert lib.fiveeq_hfc_conc_f64(N, ld, K, _ptr(d_e0), _ptr(d_time), _ptr(out), None) == _capi.OK, _last_error(lib)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[-1] == SENT, "guard word"
    got = got[:-1].reshape(K, ld)
    assert np.all(got[:, N:] == SENT), "padding columns [N, ld)"
    val = got[:, :N].view(np.float64)
    d = val[:, one].copy()
    want = e0[None, :] * d[:, None]                            # one IEEE multiply per element
    bad = np.argwhere(bits(want) != got[:, :N])
    assert bad.size == 0, (K, N, "first mismatch (k, m)", bad[0].tolist(), len(bad))
    err = ulp_errors(d, ref)
    print(f"hfc_conc K={K} N={N}: worst exp error {err.max():.4f} ulp at t={time[err.argmax()]!r}")
    assert err.max() <= EXP_ULP_BOUND, (K, N, int(err.argmax()), float(err.max()))


def test_hfc_conc_without_time_points_writes_nothing():
    lib = _capi.load()
    out = torch.full((64,), SENT, dtype=torch.int64, device="cuda")
    e0 = torch.ones(5, dtype=torch.float64, device="cuda")
    assert lib.fiveeq_hfc_conc_f64(5, 8, 0, _ptr(e0), _ptr(e0), _ptr(out), None) == _capi.OK
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ---- 4. lhs_kernel at the edges of its domain --------------------------------------------------------------------------
DIM0, N_DIM, PAD = 5, 3, 7
# around every small power of four (the Feistel domain 2^(2 half_bits) grows there, and the cycle-walk goes from never looping
# at n_total = 4^j to looping three times in four at 4^j + 1)
LHS_TOTALS = [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 4 ** 6 - 1, 4 ** 6, 4 ** 6 + 1, 4 ** 9, 4 ** 9 + 1]


def _lhs_device(n_total, m0, n, dim0=DIM0, n_dim=N_DIM):
    """Members [m0, m0 + n) on the device with ld = n + PAD into a sentinel-filled block: [n_dim, n] int64 bit patterns."""
    lib = _capi.load()
    ld = n + PAD
    out = torch.full((n_dim * ld + 1,), SENT, dtype=torch.int64, device="cuda")
    rc = lib.fiveeq_lhs_rows_f64(prm.LHS_SEED, n_total, m0, n, dim0, n_dim, ld, _ptr(out), None)
    assert rc == _capi.OK, (n_total, m0, n, _last_error(lib))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[-1] == SENT, "guard word"
    got = got[:-1].reshape(n_dim, ld)
    assert np.all(got[:, n:] == SENT), "padding columns [n, ld)"
    return got[:, :n]


def _lhs_host(n_total, m0, n, dim0=DIM0, n_dim=N_DIM):
    lib = _capi.load()
    ld = n + PAD
    out = np.full((n_dim, ld), SENT, dtype=np.int64)
    rc = lib.fiveeq_lhs_rows_host_f64(prm.LHS_SEED, n_total, m0, n, dim0, n_dim, ld, out.ctypes.data_as(ctypes.c_void_p))
    assert rc == _capi.OK and np.all(out[:, n:] == SENT)
    return out[:, :n]


@pytest.mark.parametrize("n_total", LHS_TOTALS)
def test_lhs_kernel_whole_designs_and_their_shards(n_total):
    whole = _lhs_device(n_total, 0, n_total)
    assert np.array_equal(whole, _lhs_host(n_total, 0, n_total)), "kernel != host twin"
    assert np.array_equal(whole, bits(prm.lhs_rows(n_total, range(DIM0, DIM0 + N_DIM)))), "kernel != NumPy twin"
    # three shards: the first holds one member, the last starts at n_total - 1 (for n_total <= 2 some are empty: nothing is written)
    a = min(1, n_total)
    b = max(n_total - 1, a)
    shards = [_lhs_device(n_total, lo, hi - lo) for lo, hi in ((0, a), (a, b), (b, n_total))]
    assert np.array_equal(np.concatenate(shards, axis=1), whole), "the shards are not the whole"
    u = whole.view(np.float64)
    assert np.all((u > 0.0) & (u < 1.0))
    for k in range(N_DIM):                                     # one member per stratum, strata from the bits in exact integers
        assert np.array_equal(np.sort(strata(u[k], n_total)), np.arange(n_total)), (n_total, k)
    if n_total <= 65:
        assert np.array_equal(strata(u, n_total), strata_slow(u.ravel(), n_total).reshape(u.shape))


def test_lhs_kernel_at_the_largest_design():
    lib = _capi.load()
    n_total, n = _capi.LHS_MAX_TOTAL, 70_001
    got = _lhs_device(n_total, n_total - n, n)
    assert np.array_equal(got, _lhs_host(n_total, n_total - n, n))
    u = got.view(np.float64)
    assert np.all((u > 0.0) & (u < 1.0))
    out = torch.full((N_DIM * (n + PAD),), SENT, dtype=torch.int64, device="cuda")
    rc = lib.fiveeq_lhs_rows_f64(prm.LHS_SEED, n_total + 1, n_total + 1 - n, n, DIM0, N_DIM, n + PAD, _ptr(out), None)
    torch.cuda.synchronize()
    assert rc == _capi.E_INVALID and _last_error(lib) and bool((out == SENT).all())


def test_lhs_kernel_with_three_hundred_dimensions():
    """grid.y = 300, far past the 11 rows the engine asks for: row k is dimension dim0 + k, the same bits as a call for it alone."""
    n, n_dim = 257, 300
    got = _lhs_device(n, 0, n, n_dim=n_dim)
    alone = np.concatenate([_lhs_device(n, 0, n, dim0=DIM0 + k, n_dim=1) for k in range(n_dim)])
    assert np.array_equal(got, alone)
    assert np.array_equal(got, _lhs_host(n, 0, n, n_dim=n_dim))
    assert len({row.tobytes() for row in got}) == n_dim        # 300 different permutations
