"""THE BIN RULE (include/fiveeq.h) and every counting pass held to EXACT counts: no slack anywhere, every comparison an
equality of integers or of bits.  The reference is oracle/summary_passes.bin_rule, proved against rational arithmetic in
tests/test_hist_reference_cpu.py; the rows are those of tests/hist_exact_rows.py.

 (2) fiveeq_hist_rows_* / fiveeq_hist_rows_ranged_* / fiveeq_select_bins_* on CONSTRUCTED rows: every edge of the range (the
     arithmetic edges lo + k w and, solved from the rule itself, the first value of every bin) with both neighbours, lo, hi,
     +-0, +-inf, the extreme normals, subnormals, NaNs at the first, last and mid-wave positions, the operand triples on
     which a double-rounded FMA is wrong; ranges near zero, far from zero, with an exact inv_w, too narrow for fp32
     constants, at -1e30; 1 to 4096 bins; hi <= lo; every launch shape (below a wave to a second chunk, ld > n with a sentinel in
     the padding, an offset row pointer, 1 / 2 / 5 rows, a non-zero histogram); rows that crowd into one bin in the first load
     of a group of four only, in the others only, in some waves only, in 15 / 16 / 17 lanes of a wave (the threshold), in NaNs.
 (3) fiveeq_hist_bins on PRESCRIBED indices: 0, n_bins - 1, 0xFFFF and values in [n_bins, 0xFFFF) (all skipped), the
     16-byte and the narrow path, the two-loads loop, its leftover stride, the tail, a second chunk, crowding per lane of a
     load; nothing outside hist[row][0 .. n_bins - 1] changes (canaries, neighbouring rows left non-zero).
 (4) the IN-LOOP forms (fused + ring, per-step BINS, streamed, packed, split runs) against the rule applied to the stored
     T — not against another kernel that calls the same hist_bin — with NaN members and members at +-1e30.

TEETH, measured on the CPU on the fp32 rows of (2) (153 rows: 25 range x n_bins rows of 60 to 24631 members, 128 triple
rows of 3; tests/test_hist_reference_cpu.py recomputes them): members counted in another bin by
    the fp64 formula applied to fp32 rows        33082   (143 rows)
    the double-rounded FMA                          128   (128 rows: the triples, nothing else)
    truncate (to int32) before the clamp            174   ( 20 rows: +-inf, +-max, +-1e30)
    clamp the member before the multiply          24629   (  4 rows: the range of width 1e-40)
    one packed component's pos for both members   37475   ( 18 rows)
Every variant fails these tests; none fails on 200k uniform values.

FINDINGS on the MI355X (2026-10-18): none.  Every test here passes as first written against the kernels as they were: the device
agrees with the reference and with the header on every row, fp32 and fp64 — the rows with hi <= lo (+-inf in bin 0), the
clamped constants of the 1e-40 range and the 128 double-rounding triples included — and fiveeq_hist_bins skips every index
>= n_bins, which the header now says.
"""
import ctypes

import numpy as np
import pytest

import hist_exact_rows as hx
from oracle.summary_passes import bin_rule

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
DT = {"f64": F64, "f32": F32}
PAD = 64                                                     # canary words before and after every histogram handed over
CANARY = 0x5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from fiveeqscm_amd import _capi
    return _capi.load()                                      # the HIP library must be the thing that runs: no fallback


def _p(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset)


def _device_rows(rows, ld, off, fill):
    """[K, n] host rows laid out with leading dimension ld >= n, `off` elements into a buffer whose every other element —
    the padding between rows, before the first and after the last — is `fill`.  Returns (device buffer, byte offset)."""
    K, n = rows.shape
    assert ld >= n
    buf = np.full(off + K * ld + 8, fill, dtype=rows.dtype)
    for k in range(K):
        buf[off + k * ld: off + k * ld + n] = rows[k]
    return torch.from_numpy(buf).cuda(), off * rows.dtype.itemsize


def _hist_buffer(K, nb, init):
    """K target rows of nb counters between PAD canary words and one NON-ZERO neighbouring row on each side (a row of
    another step).  Returns (host image, element offset of the target)."""
    h = np.full(2 * PAD + (K + 2) * nb, CANARY, dtype=np.int64)
    h[PAD:PAD + nb] = 1000 + np.arange(nb)
    h[PAD + (K + 1) * nb: PAD + (K + 2) * nb] = 2000 + np.arange(nb)
    h[PAD + nb: PAD + (K + 1) * nb] = 0 if init is None else np.asarray(init).reshape(-1)
    return h, PAD + nb


def _call(lib, fn, *args):
    from fiveeqscm_amd import _capi
    _capi.check(lib, getattr(lib, fn)(*args))
    torch.cuda.synchronize()


def _check_counts(h0, at, got, want, what):
    """The whole buffer: the target rows grew by exactly `want`, nothing else changed."""
    exp = h0.copy()
    exp[at:at + want.size] += want.reshape(-1)
    if not np.array_equal(got, exp):
        d = got - exp
        where = np.nonzero(d)[0]
        raise AssertionError(f"{what}: {where.size} counters differ, {int(np.abs(d[at:at + want.size]).sum()) // 2} members moved; "
                             f"first at word {where[:6] - at} (got - want = {d[where[:6]]})")


def _hist_rows(lib, sfx, rows, nb, rg, *, ld=None, off=0, init=None, what=""):
    """fiveeq_hist_rows_<sfx> (rg = (lo, hi)) or fiveeq_hist_rows_ranged_<sfx> (rg = [K, 2] array) on [K, n] rows, against
    bincount of the reference, exactly — with a sentinel from the middle of the range in all padding."""
    K, n = rows.shape
    ranged = not isinstance(rg, tuple)
    rgs = np.asarray(rg, dtype=F64).reshape(-1, 2) if ranged else np.array([rg] * K, dtype=F64)
    with np.errstate(over="ignore"):
        fill = rows.dtype.type(0.5 * rgs[0, 0] + 0.5 * rgs[0, 1])
    d_rows, boff = _device_rows(rows, ld or n, off, fill)
    h0, at = _hist_buffer(K, nb, init)
    d_hist = torch.from_numpy(h0.copy()).cuda()
    if ranged:
        d_rg = torch.from_numpy(rgs.copy()).cuda()
        _call(lib, f"fiveeq_hist_rows_ranged_{sfx}", K, n, ld or n, _p(d_rows, boff), _p(d_rg), nb, _p(d_hist, at * 8), None)
    else:
        _call(lib, f"fiveeq_hist_rows_{sfx}", K, n, ld or n, _p(d_rows, boff), float(rg[0]), float(rg[1]), nb, _p(d_hist, at * 8), None)
    want = np.stack([hx.counts(rows[k], rgs[k, 0], rgs[k, 1], nb, rows.dtype.type) for k in range(K)])
    assert want.sum(1).tolist() == (~np.isnan(rows)).sum(1).tolist()
    _check_counts(h0, at, d_hist.cpu().numpy(), want, f"hist_rows{'_ranged' if ranged else ''}_{sfx} {what}")
    return want


# ---- (2) the rule on constructed rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_every_edge_of_every_range_is_counted_in_the_bin_the_rule_names(lib, sfx):
    """Every range x n_bins of hx.RANGES x hx.N_BINS: all edges with both neighbours and the special values, NaNs at the first,
    last and mid-wave positions; through the scalar entry point one range at a time, then all ranges of one n_bins as the
    rows of ONE ranged call (each row its own range — and each row's range on every other row's members, which a kernel
    that read one range for all rows would count differently)."""
    dt = DT[sfx]
    for nb in hx.N_BINS:
        pools = [hx.edge_pool(lo, hi, nb, dt) for lo, hi in hx.RANGES]
        n = max(len(q) for q in pools) | 1
        for (lo, hi), q in zip(hx.RANGES, pools):
            _hist_rows(lib, sfx, hx.row_of(q, n, hx.NAN_AT)[None, :], nb, (lo, hi), what=f"({lo}, {hi}) x {nb}")
        rows = np.stack([hx.row_of(q, n, hx.NAN_AT) for q in pools])
        _hist_rows(lib, sfx, rows, nb, np.array(hx.RANGES), what=f"all ranges x {nb}")
        _hist_rows(lib, sfx, rows, nb, np.array(hx.RANGES[1:] + hx.RANGES[:1]), what=f"ranges rotated against the rows x {nb}")


def test_the_double_rounding_triples_fall_where_one_rounding_puts_them(lib):
    """fp32 rows: the 128 triples of hx.double_rounding_triples, each with its two neighbours, in the range that gives the
    triple's constants — one row per triple of ONE ranged call, and four of them through the scalar entry point.  The exact
    fma is pred(k): bin k - 1; a double-rounded one says k."""
    tr = hx.double_rounding_triples()
    rows, rgs = [], []
    for x, s, o, k in tr:
        rg = hx.triple_range(s, o, 4096)
        assert rg is not None
        rows.append(np.resize(np.array([x, np.nextafter(x, F32(-1)), np.nextafter(x, F32(1))], dtype=F32), 67))
        rgs.append(rg)
    rows, rgs = np.stack(rows), np.array(rgs)
    want = _hist_rows(lib, "f32", rows, 4096, rgs, what="triples")
    ks = np.array([t[3] for t in tr])
    assert (want[np.arange(len(tr)), ks - 1] >= 23).all()                   # the triple itself (23 of 67 members) is in bin k - 1
    for j in (0, 1, 50, 127):
        _hist_rows(lib, "f32", rows[j:j + 1], 4096, (float(rgs[j, 0]), float(rgs[j, 1])), what=f"triple {j}")


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_a_row_whose_range_is_empty_or_reversed_is_counted_in_bin_zero(lib, sfx):
    """The ranged entry points, hi == lo and hi < lo: every non-NaN member, +-inf included (pos = inf * 0 = NaN clamps to 0),
    is counted in bin 0, as the header says; a third row with a proper range sits between them."""
    dt = DT[sfx]
    for nb in (1, 7, 4096):
        q = hx.edge_pool(-0.3, 7.1, nb, dt)
        n = len(q) | 1
        rows = np.stack([hx.row_of(q, n, hx.NAN_AT)] * 3)
        rgs = np.array([[2.5, 2.5], [-0.3, 7.1], [7.1, -0.3]])
        want = _hist_rows(lib, sfx, rows, nb, rgs, what=f"hi <= lo x {nb}")
        assert np.isinf(rows[0]).sum() >= 2
        assert want[0, 0] == want[2, 0] == n - np.isnan(rows[0]).sum() and want[0, 1:].sum() == 0 and want[2, 1:].sum() == 0


SHAPES_N = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 16383, 16384, 16385, 32773)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_every_launch_shape_counts_every_member_once(lib, sfx):
    """n from one member to a second chunk (the four-load loop starts at 1024 members, a second chunk above 16384) x 1 / 2 / 5
    rows x ld = n or ld > n (a sentinel in the padding must not be counted) x a row pointer offset by one element x
    accumulation into a non-zero histogram — scalar and ranged entry points."""
    dt = DT[sfx]
    lo, hi, nb = -0.3, 7.1, 4096
    q = hx.edge_pool(lo, hi, nb, dt)
    rng = np.random.default_rng(8)
    for i, n in enumerate(SHAPES_N):
        K = (1, 2, 5)[i % 3]
        rows = np.stack([hx.row_of(np.roll(q, 1000 * k + i), n, hx.NAN_AT) for k in range(K)])
        for ld, off in ((n, 0), (n + 3, 0), (n, 1), (n + 8, 1)):
            init = rng.integers(0, 1 << 40, size=(K, nb)) if (ld + off) % 2 else None
            _hist_rows(lib, sfx, rows, nb, (lo, hi), ld=ld, off=off, init=init, what=f"n={n} K={K} ld={ld} off={off}")
        _hist_rows(lib, sfx, rows, nb, np.array([[lo, hi]] * K), ld=n + 5, off=1, init=rng.integers(0, 9, size=(K, nb)),
                   what=f"ranged n={n} K={K}")


def _crowd_rows(vals, n):
    """Rows of bins by position (vals[b] is a value of bin b; 4096 bins).  The crowded-or-plain choice of hist_rows_kernel is made
    per wave and group of four loads (members m, m + 256, m + 512, m + 768 of a period of 1024), on the first load."""
    pos = np.arange(n)
    per, lane, wave = pos % 1024, pos % 64, (pos // 64) % 4
    spread = 100 + per                                                                  # distinct within a period
    bins = {
        "first load crowded, the other three spread": np.where(per < 256, 7, spread),
        "first load spread, the other three crowded": np.where(per < 256, spread, 7),
        "waves 1 and 3 crowded, waves 0 and 2 spread": np.where(wave % 2 == 1, 9, spread),
        "15 lanes of a wave share a bin": np.where(lane < 15, 11, spread),
        "16 lanes of a wave share a bin": np.where(lane < 16, 11, spread),
        "17 lanes of a wave share a bin": np.where(lane < 17, 11, spread),
        "the shared bin is not the first lane's": np.where((lane >= 5) & (lane < 40), 13, spread),
        "all one bin": np.full(n, 4095),
        "all distinct": pos % 4096,
    }
    rows = {k: vals[b] for k, b in bins.items()}
    x = vals[spread].copy()
    x[lane < 20] = np.nan                                                               # the crowd is of NaNs: counted nowhere
    rows["20 lanes of a wave are NaN"] = x
    return rows


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_crowded_and_spread_lanes_mixed_inside_one_group_of_loads(lib, sfx):
    dt = DT[sfx]
    lo, hi, nb = -0.3, 7.1, 4096
    vals = np.concatenate([[dt(lo - 1.0)], hx.edges_of_rule(lo, hi, nb, dt)])
    assert np.array_equal(bin_rule(vals, lo, hi, nb, dt), np.arange(nb))
    for n in (2 * 4096 + 1024 + 301, 16384 + 4096 + 77):                                  # whole groups + the tail; a second chunk
        rows = _crowd_rows(vals, n)
        for name, x in rows.items():
            _hist_rows(lib, sfx, x[None, :], nb, (lo, hi), what=f"{name}, n={n}")
        _hist_rows(lib, sfx, np.stack(list(rows.values())), nb, np.array([[lo, hi]] * len(rows)), ld=n + 3, off=1,
                   what=f"all crowding rows, ranged, n={n}")


def _bits_sorted(x):
    return np.sort(np.ascontiguousarray(x).view(np.int64 if x.dtype == F64 else np.int32))


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_selection_takes_exactly_the_members_the_rule_puts_in_the_marked_bins(lib, sfx):
    """fiveeq_select_bins_* on the edge rows: the candidates of the marked bins, as a multiset of BIT PATTERNS, are the
    members the reference puts there, and cand_n is their count — for fp32 as for fp64, on the 16-byte path (n a multiple
    of 4) and the narrow one (odd n)."""
    dt = DT[sfx]
    rng = np.random.default_rng(9)
    for nb in (3, 4096):
        pools = [hx.edge_pool(lo, hi, nb, dt) for lo, hi in hx.RANGES]
        for n in ((max(len(q) for q in pools) + 3) // 4 * 4, max(len(q) for q in pools) | 1):
            rows = np.stack([hx.row_of(q, n, hx.NAN_AT) for q in pools])
            K = len(rows)
            rgs = np.array(hx.RANGES, dtype=F64)
            marked = rng.uniform(size=(K, nb)) < 0.3
            marked[:, [0, nb - 1]] = True
            words = (nb + 31) // 32
            bits = np.zeros((K, words * 32), dtype=np.uint8)
            bits[:, :nb] = marked
            mask = np.packbits(bits.reshape(K, words, 32), axis=2, bitorder="little").view(np.uint32).reshape(K, words)
            d_rows, d_rg = torch.from_numpy(rows).cuda(), torch.from_numpy(rgs).cuda()
            d_mask = torch.from_numpy(mask.view(np.int32).copy()).cuda()
            cand = torch.full((K, n), -777.0, dtype=d_rows.dtype, device="cuda")
            cand_n = torch.zeros(K, dtype=torch.int64, device="cuda")
            _call(lib, f"fiveeq_select_bins_{sfx}", K, n, n, _p(d_rows), _p(d_rg), nb, _p(d_mask), _p(cand), n, _p(cand_n), None)
            got_n, got = cand_n.cpu().numpy(), cand.cpu().numpy()
            for k in range(K):
                b = bin_rule(rows[k], rgs[k, 0], rgs[k, 1], nb, dt)
                want = rows[k][(b >= 0) & marked[k][np.maximum(b, 0)]]
                assert got_n[k] == want.size, (sfx, nb, n, k, int(got_n[k]), want.size)
                assert np.array_equal(_bits_sorted(got[k, :want.size]), _bits_sorted(want)), (sfx, nb, n, k)
                assert (got[k, want.size:] == -777.0).all()


# ---- (3) the ring pass on prescribed indices ------------------------------------------------------------------------------------
def _hist_bins(lib, rows, nb, *, ld=None, off=0, init=None, what=""):
    K, n = rows.shape
    d_rows, boff = _device_rows(rows, ld or n, off, np.uint16(min(nb - 1, 2)))            # the padding holds a VALID index
    h0, at = _hist_buffer(K, nb, init)
    d_hist = torch.from_numpy(h0.copy()).cuda()
    _call(lib, "fiveeq_hist_bins", K, n, ld or n, _p(d_rows, boff), nb, _p(d_hist, at * 8), None)
    want = np.stack([np.bincount(r[r < nb].astype(np.int64), minlength=nb) for r in rows]).astype(np.int64)
    _check_counts(h0, at, d_hist.cpu().numpy(), want, f"hist_bins {what}")
    return (d_rows.data_ptr() + boff) % 16 == 0 and ((ld or n) * 2) % 16 == 0            # did the 16-byte path run?


def _index_row(rng, n, nb):
    """Valid indices with the edges 0 and nb - 1 and, a third of the row, indices the pass must skip: 0xFFFF (a NaN), nb,
    nb + 1, 4096 and 4097 (past the 4096-word LDS histogram), 0xFFFE."""
    x = rng.integers(0, nb, size=n).astype(np.uint16)
    kind = rng.integers(0, 12, size=n)
    skip = np.array([0xFFFF, nb, nb + 1, 4096, 4097, 0xFFFE, 0x8000], dtype=np.uint16)
    x = np.where(kind == 0, np.uint16(0), np.where(kind == 1, np.uint16(nb - 1), x))
    x = np.where(kind >= 8, skip[rng.integers(0, len(skip), size=n)], x)
    return x.astype(np.uint16)


BINS_N = (1, 7, 8, 9, 2047, 2048, 2049, 4095, 4096, 4097, 6144, 6145, 16384, 16385, 18433)


def test_prescribed_indices_are_counted_exactly_and_indices_past_n_bins_skipped(lib):
    """fiveeq_hist_bins, every size (the two-loads loop from 4096, its leftover stride at 2048 and 6144, the tail, a second
    chunk above 16384) x the 16-byte path (aligned pointer, ld a multiple of 8) and the narrow one (pointer offset by one
    element, or an odd ld) x 1 / 3 rows x 1 / 7 / 4096 bins x accumulation.  Every index >= n_bins is skipped and nothing
    outside hist[row][0 .. n_bins - 1] changes: canary words on both sides, the neighbouring rows non-zero."""
    rng = np.random.default_rng(10)
    ran_wide = 0
    for i, n in enumerate(BINS_N):
        for nb in (1, 7, 4096):
            K = (1, 3)[(i + nb) % 2]
            rows = np.stack([_index_row(rng, n, nb) for _ in range(K)])
            ld8 = (n + 7) // 8 * 8
            for ld, off in ((ld8, 0), (ld8 + 8, 8), (ld8, 1), (ld8 + 1, 0), (n, 0)):
                init = rng.integers(0, 1 << 40, size=(K, nb)) if off else None
                w = _hist_bins(lib, rows, nb, ld=ld, off=off, init=init, what=f"n={n} nb={nb} K={K} ld={ld} off={off}")
                ran_wide += w
                if off == 1:
                    assert not w
                if off in (0, 8) and ld % 8 == 0:
                    assert w
    assert ran_wide >= 2 * 3 * len(BINS_N)


def test_ring_rows_that_crowd_in_some_lanes_of_a_load_only(lib):
    """The crowded-or-plain choice of hist_bins_kernel is made per wave and 16-byte load, on each lane's FIRST member (members
    = 0 mod 8): rows where those share a bin and the other seven are spread, the converse, rows where only some waves are
    crowded, a crowd of skipped indices, all-one-bin and all-distinct rows — on both paths."""
    rng = np.random.default_rng(11)
    for nb in (1, 7, 4096):
        for n in (6144 + 2048 + 301, 18433):
            pos = np.arange(n)
            spread = (pos * 7 + 3) % nb
            wave = (pos // 512) % 4                                                  # 8 members per lane: 512 per wave-load
            lane = (pos // 8) % 64
            rows = np.stack([
                np.where(pos % 8 == 0, nb // 2, spread),
                np.where(pos % 8 == 0, spread, nb // 2),
                np.where(wave % 2 == 1, nb - 1, spread),
                np.where((pos % 8 == 0) & (lane < 16), 0, spread),
                np.where((pos % 8 == 0) & (lane < 15), 0, spread),
                np.where(pos % 8 == 0, 0xFFFF, spread),                              # the crowd is of NaN indices
                np.where(pos % 8 == 0, nb, spread),                                  # ... of the first index past the histogram
                np.where(pos % 8 == 0, spread, 0xFFFF),
                np.full(n, nb - 1),
                pos % nb,
            ]).astype(np.uint16)
            ld8 = (n + 7) // 8 * 8
            assert _hist_bins(lib, rows, nb, ld=ld8, what=f"crowding, 16-byte path, nb={nb} n={n}")
            assert not _hist_bins(lib, rows, nb, ld=ld8, off=1, init=rng.integers(0, 99, size=(len(rows), nb)),
                                  what=f"crowding, narrow path, nb={nb} n={n}")


# ---- (4) the in-loop forms against the rule itself ------------------------------------------------------------------------------
N_STEPS = 12
IN_LOOP = [("f64", 1, 201, 7), ("f64", 1, 4098, 4096), ("f64", 1, 4099, 7), ("f32", 1, 202, 4096), ("f32", 1, 4098, 7),
           ("f32", 0, 202, 7), ("f32", 0, 4099, 4096), ("f32", 1, 201, 4096), ("f32", 1, 4099, 7), ("f32", 1, 4099, 4096)]


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    word = {8: np.int64, 4: np.int32}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(word), b.view(word))


@pytest.mark.parametrize("prec,packing,N,nb", IN_LOOP)
def test_in_loop_histograms_are_the_rule_applied_to_the_stored_T(lib, prec, packing, N, nb):
    """Engines with hist=(lo, hi, nb) and a stored T: T_hist[t] == bincount(rule(T[t])) for every step, by the REFERENCE —
    fused with a ring of 1 and of 3 steps, per-step BINS on one and on two streams (member chunks of 256 in one of them),
    a run split mid-way fused -> per-step and per-step -> fused; fp64, fp32 packed (even N), fp32 with packing off, fp32 with
    an odd N (the half-filled last packed lane).  Members made NaN through R0 (first; even and odd in a packed lane; last of
    a 64-member record; last of all) have no bin; members with S0 = +-1e30 (a finite, huge T: pos overflows in fp32) land in
    the edge bins; the range is tight enough that in-domain members use both edge bins too.  Everybody else's C, T, R, S are
    those of a run without hist=, bit for bit."""
    from fiveeqscm_amd import emissions, params
    from fiveeqscm_amd.engine import EnsembleEngine
    td, dt = (torch.float64, F64) if prec == "f64" else (torch.float32, F32)
    p = params.sample_ensemble(params.default_params("multigas"), N)
    E = emissions.rcp_like_emissions(750, 3)[200:200 + N_STEPS] * 1.7
    nan_at = [0, 10, 11, 63, N - 1]
    huge_at = {5: 1e30, 20: -1e30, 21: 1e30, 64: -1e30, N - 2: 1e30}
    lib.fiveeq_set_f32_packing(int(packing))
    try:
        probe = EnsembleEngine(p, N, E, device="cuda:0", dtype=td, store_trajectory=False)
        R0, S0 = np.zeros(tuple(probe.R.shape)), np.zeros(tuple(probe.S.shape))
        probe.close()
        R0[:, nan_at] = np.nan
        for m, v in huge_at.items():
            S0[:, m] = v
        kw = dict(device="cuda:0", dtype=td, R0=R0, S0=S0)
        ref = EnsembleEngine(p, N, E, **kw)
        ref.run(mode="fused")
        torch.cuda.synchronize()
        want_rows = {k: getattr(ref, k).cpu().numpy() for k in ("C", "T", "R", "S")}
        T = want_rows["T"]
        assert T.dtype == dt and np.isnan(T[:, nan_at]).all()
        plain = np.setdiff1d(np.arange(N), nan_at + list(huge_at))
        assert np.isfinite(T[:, plain]).all()
        with np.errstate(invalid="ignore"):
            assert (np.abs(T[:, list(huge_at)].astype(F64)) > 1e25).any(axis=1).all()    # finite and huge, at every step
        lo, hi = (float(v) for v in np.quantile(T[:, plain].astype(F64), [0.1, 0.9]))
        b_plain = bin_rule(T[:, plain], lo, hi, nb, dt)
        assert (b_plain == 0).any() and (b_plain == nb - 1).any()                       # in-domain members use both edge bins
        want = np.stack([hx.counts(T[t], lo, hi, nb, dt) for t in range(N_STEPS)])
        assert want.sum(1).tolist() == (N - np.isnan(T).sum(1)).tolist() and want.sum(1).max() <= N - len(nan_at)
        forms = {
            "fused, ring of 1": (dict(hist_ring_steps=1), [(0, N_STEPS, "fused")]),
            "fused, ring of 3": (dict(hist_ring_steps=3), [(0, N_STEPS, "fused")]),
            "per-step, one stream": (dict(per_step_streams=1, chunk_members=0), [(0, N_STEPS, "per_step")]),
            "per-step, two streams, chunks of 256": (dict(per_step_streams=2, chunk_members=256), [(0, N_STEPS, "per_step")]),
            "fused then per-step": (dict(hist_ring_steps=3), [(0, 5, "fused"), (5, N_STEPS, "per_step")]),
            "per-step then fused": (dict(hist_ring_steps=2, per_step_streams=2), [(0, 7, "per_step"), (7, N_STEPS, "fused")]),
        }
        is_nan = np.isnan(T).any(0)                                   # (the members made NaN; a huge member may follow them)
        others, nan_m = np.nonzero(~is_nan)[0], np.nonzero(is_nan)[0]
        for name, (fkw, runs) in forms.items():
            eng = EnsembleEngine(p, N, E, hist=(lo, hi, nb), **fkw, **kw)
            for t0, t1, mode in runs:
                eng.run(t0, t1, mode=mode)
            torch.cuda.synchronize()
            got = eng.T_hist.cpu().numpy()
            if not np.array_equal(got, want):
                bad = np.nonzero((got != want).any(1))[0]
                raise AssertionError(f"{name}: T_hist differs from the rule at steps {bad.tolist()}: "
                                     f"{[int(np.abs(got[t] - want[t]).sum()) for t in bad]} counts")
            assert np.array_equal(eng.hist_edge_counts().cpu().numpy(), want[:, [0, -1]]), name
            for k, w in want_rows.items():
                g = getattr(eng, k).cpu().numpy()
                assert _bits_equal(g[..., others], w[..., others]), (name, k)
                assert np.array_equal(np.isnan(g[..., nan_m]), np.isnan(w[..., nan_m])), (name, k)
            eng.close()
        ref.close()
    finally:
        lib.fiveeq_set_f32_packing(1)
