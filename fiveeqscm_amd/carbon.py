"""The carbon cycle of a run, diagnosed from its STORED rows: airborne emissions, cumulative emissions and uptake, airborne
fraction, iIRF100, the lifetime scaling alpha and the sink flux.

The stepping kernels form G_a, G_u, the iIRF and alpha in registers and drop them; they are functions of what a run stores (the
concentrations C — for a concentration-driven gas the diagnosed emissions E — and the warming T), of the member's r0, rC, rT and
of the shared drive table, so ONE streaming HIP pass recomputes them afterwards — iirf and alpha with the statements of the
stepping kernels — for rows of every mode, drive and precision (include/fiveeq.h, "CARBON ROWS"; csrc/fiveeq_carbon.hpp):

    res = carbon_rows(eng.C, eng.out_steps, params, r=eng.r, drive=eng.drive, dt=eng.dt, T_rows=eng.T, want=("fraction", "alpha"))
    res = eng.carbon_rows(want=("fraction", "alpha"))                 # the same, wired to the engine

    airborne  G_a = (C - C0) / emis2conc, the emissions still airborne      cumE      the cumulative emissions (shared table, or
    uptake    G_u = cumE - G_a, what land and ocean took up                           per member for a concentration-driven gas)
    fraction  G_a / cumE, the airborne fraction                             iirf      the iIRF100 the NEXT step uses, capped
    alpha     g0 exp(iirf / g1), the lifetime scaling the NEXT step uses    sink      E - (G_a - G_a_prev) / dt, the sink flux

Where the rows go: `constrain.score_rows(res.sink[:, 0], steps, Observations...)` scores a carbon-budget record;
`res.fraction[k:k + 1, 0]` (a one-row block) goes into distributed.gather_summary / gather_weighted_summary for percentiles; any
row goes into EnsembleEngine.drivers / joint.sensitivity as y.
Device rows only: there is no CPU path (_carbon_host.py is the NumPy twin of the tests).
"""
import ctypes
from dataclasses import dataclass

import numpy as np

WANT = ("airborne", "cumE", "uptake", "fraction", "iirf", "alpha", "sink")
_NEED_CUM = ("cumE", "uptake", "fraction", "iirf", "alpha")


@dataclass
class CarbonRows:
    """What carbon_rows returns: device tensors [n_rows, n_sel, N] in the rows' precision, None for what was not asked for;
    `gases` the selected gas indices (axis 1).  cum_end [G, N]: the cumulative emissions of the concentration-driven gases after
    the last row (None when nothing carried them) and airborne_end [G, N]: G_a after the last row (with "sink" or airborne0
    only) — cum0 / airborne0 of a later call over LATER rows; rows of unselected gases hold what came in."""
    airborne: object = None
    cumE: object = None
    uptake: object = None
    fraction: object = None
    iirf: object = None
    alpha: object = None
    sink: object = None
    cum_end: object = None
    airborne_end: object = None
    gases: tuple = ()


def cum_end_table(E, dt):
    """The shared cumulative emissions at the END of each step, fp64 [n_steps, G]: np.cumsum(E dt, axis=0) — the sum
    emissions.make_drive puts into column 3 + g of step t + 1."""
    E = np.asarray(E, dtype=np.float64)
    return np.cumsum((E[:, None] if E.ndim == 1 else E) * float(dt), axis=0)


def _selected(gases, G):
    sel = tuple(range(G)) if gases is None else tuple(gases)
    if not sel or any(not isinstance(g, (int, np.integer)) or not 0 <= g < G for g in sel) or list(sel) != sorted(set(sel)):
        raise ValueError(f"gases={gases!r}: want distinct, increasing gas indices in 0..{G - 1}")
    return tuple(int(g) for g in sel)


def carbon_rows(rows, steps, params, *, r, drive, dt, T_rows=None, concentration_gases=(), gases=None, want=("fraction",),
                cum0=None, airborne0=None, cum_table=None):
    """The carbon-cycle quantities of STORED rows — one streaming HIP pass.
    rows [n_rows, G, N]: the stored fp32 / fp64 rows ON THE GPU (engine.C: concentrations, and for a concentration-driven gas the
    diagnosed emissions; or row / member slices of it), read in place whenever the member stride is 1, copied otherwise.
    steps [n_rows]: the model step each row holds, strictly increasing.  params: the parameter dict of the run.  r [3 G, N]
    device rows (engine.r: r0, rC, rT of gas 0, then gas 1, ...).  drive: the shared drive table — a device table [n_steps, 8]
    in the rows' precision (engine.drive), or host values [n_steps, 8] / [n_steps, G] (emissions, targets for a driven gas).
    dt: the run's step.  T_rows [n_rows, N]: the stored warming, needed for "iirf" and "alpha".  concentration_gases: the gases
    that were concentration-driven.  gases: the gases to diagnose (default: all), increasing.
    want: any of "airborne", "cumE", "uptake", "fraction", "iirf", "alpha", "sink".
    cum0 [G, N] / airborne0 [G, N]: the cumulative emissions of the concentration-driven gases and G_a BEFORE the first row — the
    cum_end / airborne_end of an earlier call over EARLIER rows: the result is, bit for bit, that of one call over all the rows
    (None: 0).  cum_table: the shared cumulative emissions at the end of each step, fp64 host [n_steps, G] (cum_end_table());
    default: formed from the emission columns of a host `drive`, or for a device table read back from it (column 3 + g of step
    t + 1; the last step from the table's own emissions — exact for an fp64 table).
    "sink", and "cumE" / "uptake" / "fraction" / "iirf" / "alpha" of a concentration-driven gas, need rows of consecutive model
    steps: ValueError otherwise, naming the first gap.  TypeError for host rows: there is no CPU path.  Runs on the current
    stream; reads its inputs, allocates its results."""
    import torch

    from . import _capi
    from ._rowargs import call, dev_rows, drive_table, model_steps, ptr, steps_i32, steps_in_tables, walk_in_place
    from .diagnose import check_consecutive
    from .emissions import concentration_mask
    from .params import make_model
    want = tuple(want)
    if not want or any(w not in WANT for w in want):
        raise ValueError(f"want: {want!r}; any of {WANT}")
    if not isinstance(rows, torch.Tensor) or rows.dim() != 3:
        raise ValueError("rows: want a tensor [n_rows, G, N]")
    K, G, N = rows.shape
    dev, dtp = rows.device, rows.dtype
    model = make_model(params, dt)
    if int(model.n_gas) != G:
        raise ValueError(f"rows hold {G} gases, params {int(model.n_gas)}")
    if N < 1:
        raise ValueError("rows: no members")
    conc_mask = concentration_mask(concentration_gases, G)
    sel = _selected(gases, G)
    gas_mask = sum(1 << g for g in sel)
    st = model_steps(steps, K)
    need_T = "iirf" in want or "alpha" in want
    if need_T and T_rows is None:
        raise ValueError("iirf and alpha need T_rows")
    need_cum = bool(gas_mask & conc_mask) and any(w in _NEED_CUM for w in want)
    need_ga = "sink" in want or airborne0 is not None
    if "sink" in want or airborne0 is not None:
        check_consecutive(st, "the sink flux")
    if need_cum or cum0 is not None:
        check_consecutive(st, "the cumulative emissions of a concentration-driven gas")
    # (after every refusal that needs no device, so that each of them is raised for host rows too)
    if not rows.is_cuda or rows.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"rows must be fp32 / fp64 rows on a GPU (got {rows.dtype} on {rows.device}): the carbon rows run "
                        "through the HIP kernel and have no CPU fallback")

    # the shared tables: the drive table as the kernel reads it, the cumulative emissions at the end of each step
    if isinstance(drive, torch.Tensor):
        drv = drive_table(drive, (), "drive (a device table)", dtp, dev)
        host = None
    else:
        host = np.asarray(drive, dtype=np.float64)
        if host.ndim != 2 or host.shape[1] < G:
            raise ValueError(f"drive: want a table [n_steps, 8] or [n_steps, {G}]")
        table = np.zeros((host.shape[0], _capi.DRIVE_STRIDE))
        table[:, :G] = host[:, :G]
        drv = torch.from_numpy(table).to(dev, dtp)
    n_steps = int(drv.shape[0])
    steps_in_tables(st, n_steps)
    if cum_table is None:
        if host is not None:
            cum_table = cum_end_table(host[:, :G], dt)
        else:
            d64 = drv.to(torch.float64).cpu().numpy()
            cum_table = cum_end_table(d64[:, :G], dt)
            cum_table[:-1] = d64[1:, 3:3 + G]
    cum_table = np.asarray(cum_table, dtype=np.float64)
    if cum_table.shape != (n_steps, G):
        raise ValueError(f"cum_table: want [{n_steps}, {G}]")
    ce = np.zeros((n_steps, _capi.MAX_GAS))
    ce[:, :G] = cum_table
    ce = torch.from_numpy(ce).to(dev, dtp)

    # per-member rows the kernel reads with ONE row stride ld: r as it lies when its columns are contiguous, the carried state
    # laid out to match
    r_rows, ld = None, N
    if need_T:
        r_rows, (ld,) = walk_in_place(dev_rows(r, (3 * G, N), "r", dtp, dev), N)
    x, (c_row, c_gas) = walk_in_place(rows, N)
    tr, t_row = None, N
    if need_T:
        tr, (t_row,) = walk_in_place(dev_rows(T_rows, (K, N), "T_rows", dtp, dev), N)
    res = CarbonRows(gases=sel)
    # every output row starts 16-byte aligned: one row length for all of them, N rounded up to 16 bytes of the rows' type
    per16 = 16 // x.element_size()
    ld_out = (N + per16 - 1) // per16 * per16
    for w in WANT:
        if w in want:
            setattr(res, w, torch.empty((K, len(sel), ld_out), dtype=dtp, device=dev)[..., :N])
    cum_io = ga_io = None
    if need_cum or cum0 is not None:
        cum_io = torch.zeros((G, ld), dtype=dtp, device=dev)[:, :N]
        if cum0 is not None:
            cum_io.copy_(dev_rows(cum0, (G, N), "cum0", dtp, dev))
    if need_ga:
        ga_io = torch.zeros((G, ld), dtype=dtp, device=dev)[:, :N]
        if airborne0 is not None:
            ga_io.copy_(dev_rows(airborne0, (G, N), "airborne0", dtp, dev))
    st32 = steps_i32(st, dev)
    call(_capi.load(), _capi, "fiveeq_carbon_rows", dtp, dev, ctypes.byref(model), K, N, ld, ptr(x) if K else None, c_row, c_gas,
         ptr(tr) if K else None, t_row, ptr(st32) if K else None, ptr(drv), ptr(ce), n_steps, ptr(r_rows), conc_mask, gas_mask,
         *(ptr(getattr(res, w)) for w in WANT), ld_out, ptr(cum_io), ptr(ga_io))
    res.cum_end, res.airborne_end = cum_io, ga_io
    return res
