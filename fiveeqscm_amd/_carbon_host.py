"""NumPy restatement of the CARBON ROWS pass of the C ABI (include/fiveeq.h, "CARBON ROWS": fiveeq_carbon_rows_f64 / _f32;
csrc/fiveeq_carbon.hpp).  Used by the tests only: the package's carbon_rows() has no CPU path.

What the twin is good for, and how far:
  * airborne, cumE, uptake, fraction and sink are THE KERNEL'S BITS: single IEEE operations in the rows' precision (one
    subtraction and one product; one subtraction; one division; a subtraction, a division and a subtraction), which NumPy
    performs as the kernel does.  The cumulative emissions of a concentration-driven gas are one fma per row, done exactly here.
  * iirf is the kernel's bits too: three nested fma, each formed exactly (integer arithmetic on the operands' ratios, one
    rounding) — fma() below — and the IEEE minNum against iirf_max.
  * alpha = g0 exp(iirf / g1) is within the bound of the device's exp (tests/math_reference.py) plus one ulp for each of the two
    products: NumPy calls libm's exp where the kernel evaluates its own routine.
"""
import numpy as np

WANT = ("airborne", "cumE", "uptake", "fraction", "iirf", "alpha", "sink")


def _round_ratio(num, den, dtype):
    """num / den (integers, den > 0) rounded ONCE to dtype, ties to even."""
    d = num / den                                              # int / int: correctly rounded to double
    if dtype == np.float64:
        return d
    f = np.float32(d)
    # double rounding: d is the exact value rounded to 53 bits; rounding d again to 24 bits errs only where d lies exactly
    # half way between two floats while the exact value does not
    if (np.float64(d).view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000):
        dn, dd = d.as_integer_ratio()
        side = num * dd - dn * den                             # sign of (exact - d)
        if side:
            lo, hi = np.nextafter(np.float32(d), np.float32(-np.inf)), np.nextafter(np.float32(d), np.float32(np.inf))
            cands = sorted({float(f), float(lo), float(hi)})
            below = max(c for c in cands if c <= d)
            above = min(c for c in cands if c >= d)
            f = np.float32(above if side > 0 else below)
    return f


def fma(a, b, c, dtype):
    """a * b + c with ONE rounding in dtype (float32 / float64), elementwise over broadcast operands: what fe_fma() does on the
    device.  Non-finite operands take the IEEE result of the separate operations (NaN and infinities propagate alike)."""
    dtype = np.dtype(dtype).type
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype), np.asarray(c, dtype=dtype))
    out = np.empty(a.shape, dtype=dtype)
    of = out.reshape(-1)
    with np.errstate(all="ignore"):
        loose = (a * b + c).reshape(-1)
    fin = (np.isfinite(a) & np.isfinite(b) & np.isfinite(c)).reshape(-1)
    af, bf, cf = (x.reshape(-1).astype(np.float64).tolist() for x in (a, b, c))
    for i in range(of.size):
        if not fin[i]:
            of[i] = loose[i]
            continue
        n1, d1 = af[i].as_integer_ratio()
        n2, d2 = bf[i].as_integer_ratio()
        n3, d3 = cf[i].as_integer_ratio()
        num = n1 * n2 * d3 + n3 * d1 * d2
        of[i] = _round_ratio(num, d1 * d2 * d3, dtype) if num else loose[i]       # an exact zero keeps IEEE's sign
    return out


def cum_end_table(E, dt):
    """The shared cumulative emissions at the END of each step, fp64 [n_steps, G]: np.cumsum(E dt) — the sum make_drive puts
    into column 3 + g of step t + 1."""
    E = np.asarray(E, dtype=np.float64)
    return np.cumsum((E[:, None] if E.ndim == 1 else E) * float(dt), axis=0)


def kernel_constants(params, dt, dtype):
    """The model's constants as the kernel holds them (make_kmodel): computed in fp64, rounded to the rows' precision."""
    from .params import make_model
    m = make_model(params, dt)
    t = np.dtype(dtype).type
    gases = [dict(C0=t(m.gas[g].C0), inv_c=t(1.0 / m.gas[g].emis2conc), ra=t(m.gas[g].ra), g0=t(m.gas[g].g0),
                  inv_g1=t(1.0 / m.gas[g].g1)) for g in range(int(m.n_gas))]
    return gases, t(m.iirf_max), t(m.dt)


def carbon_rows_host(rows, steps, params, *, r=None, drive, dt=1.0, T_rows=None, concentration_gases=(), gases=None,
                     want=("fraction",), cum0=None, airborne0=None, cum_table=None):
    """carbon.carbon_rows over host arrays: dict with the entries of `want` (each [n_rows, n_sel, N]) plus "cum_end" [G, N]
    (the cumulative emissions of the concentration-driven gases after the last row; 0 elsewhere) and "airborne_end" [G, N]
    (G_a of the selected gases after the last row).  rows [n_rows, G, N] in the rows' precision; r [3 G, N]; drive [n_steps, 8]
    (or [n_steps, G]) host values; cum_table fp64 [n_steps, G] (default: cum_end_table of the drive's emission columns)."""
    x = np.asarray(rows)
    t = x.dtype.type
    K, G, N = x.shape
    st = np.asarray(steps, dtype=np.int64)
    drv = np.asarray(drive, dtype=np.float64)
    table = cum_end_table(drv[:, :G], dt) if cum_table is None else np.asarray(cum_table, dtype=np.float64)
    kg, iirf_max, dtt = kernel_constants(params, dt, t)
    conc = set(int(g) for g in concentration_gases)
    sel = list(range(G)) if gases is None else [int(g) for g in gases]
    need_alpha = "iirf" in want or "alpha" in want
    out = {w: np.empty((K, len(sel), N), dtype=t) for w in WANT}
    cum_end = np.zeros((G, N), dtype=t) if cum0 is None else np.array(cum0, dtype=t)
    ga_end = np.zeros((G, N), dtype=t) if airborne0 is None else np.array(airborne0, dtype=t)
    with np.errstate(all="ignore"):
        for slot, g in enumerate(sel):
            c = kg[g]
            shared = drv[st, g].astype(t)[:, None]
            if g in conc:
                Cg, E = np.broadcast_to(shared, (K, N)), x[:, g]
                cumE = np.empty((K, N), dtype=t)
                run = cum_end[g].copy()
                for k in range(K):
                    run = fma(E[k], dtt, run, t)
                    cumE[k] = run
                cum_end[g] = run
            else:
                Cg, E = x[:, g], np.broadcast_to(shared, (K, N))
                cumE = np.broadcast_to(table[st, g].astype(t)[:, None], (K, N))
            Ga = ((Cg - c["C0"]) * c["inv_c"]).astype(t)
            Gu = (cumE - Ga).astype(t)
            out["airborne"][:, slot], out["cumE"][:, slot], out["uptake"][:, slot] = Ga, cumE, Gu
            out["fraction"][:, slot] = Ga / cumE
            if need_alpha:
                rr = np.asarray(r, dtype=t)
                Tr = np.asarray(T_rows, dtype=t)
                ii = fma(c["ra"], Ga, fma(rr[3 * g + 2][None, :], Tr, fma(rr[3 * g + 1][None, :], Gu, rr[3 * g][None, :], t), t), t)
                ii = np.fmin(ii, iirf_max)
                out["iirf"][:, slot] = ii
                out["alpha"][:, slot] = c["g0"] * np.exp((ii * c["inv_g1"]).astype(t))
            prev = np.concatenate([ga_end[g][None, :], Ga[:-1]], axis=0)
            out["sink"][:, slot] = E - ((Ga - prev).astype(t) / dtt).astype(t)
            if K:
                ga_end[g] = Ga[-1]
    res = {w: out[w] for w in want}
    res["cum_end"], res["airborne_end"] = cum_end, ga_end
    return res
