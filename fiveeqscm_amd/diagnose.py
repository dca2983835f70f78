"""Forcing, energy imbalance and heat uptake of a run, diagnosed from its STORED rows.

The stepping kernels form the effective radiative forcing F in registers and drop it; it is a pure function of what a run
stores (the step's concentrations, the member's forcing scales, the step's shared F_ext and category record), so ONE streaming
HIP pass recomputes it afterwards — with the device function the stepping kernels call, hence with their bits — for rows of
every mode and precision (include/fiveeq.h, "FORCING ROWS"; csrc/fiveeq_forcrows.hpp):

    res = forcing_rows(eng.C, eng.out_steps, params, q=eng.q, F_ext=eng.drive, dt=eng.dt, T_rows=eng.T, want=("F", "N", "H"))
    res = eng.forcing_rows(want=("F", "N", "H"))                      # the same, wired to the engine

    F      effective radiative forcing, W m-2                         F_gas  its split by gas
    N      top-of-atmosphere energy imbalance  N = F - T / (q0 + q1)  (the two-box model's equilibrium is T = (q0 + q1) F: its
           feedback parameter is 1 / (q0 + q1))
    H      cumulated heat uptake  H += dt N, fp64, W yr m-2           (times W_YR_M2_TO_ZJ: zettajoules)

Where the rows go: `constrain.score_rows(res.H, steps, Observations...)` scores a heat-content record (res.F against an
assessed forcing range alike); `res.F[k:k + 1]` (a one-row block) goes into distributed.gather_summary /
gather_weighted_summary for percentiles; any row goes into EnsembleEngine.drivers / joint.sensitivity as y.
Device rows only: there is no CPU path (_diagnose_host.py is the NumPy twin of the tests).
"""
import ctypes
from dataclasses import dataclass

import numpy as np

# W yr m-2 (per unit area of the Earth's surface, cumulated over years) -> zettajoules:
#     1 W yr m-2  =  1 J/s  x  (365.25 d x 86400 s/d = 31 557 600 s)  x  5.100656e14 m2 (the Earth's surface)
#                 =  1.609644...e22 J  =  16.09644... ZJ          (1 ZJ = 1e21 J)
EARTH_SURFACE_M2 = 5.100656e14
SECONDS_PER_YEAR = 365.25 * 86400.0
W_YR_M2_TO_ZJ = EARTH_SURFACE_M2 * SECONDS_PER_YEAR / 1e21

WANT = ("F", "F_gas", "N", "H")


@dataclass
class ForcingRows:
    """What forcing_rows returns: device tensors, None for what was not asked for.  F, N [n_rows, N] and F_gas [n_rows, G, N] in
    the rows' precision; H [n_rows, N] fp64 (the heat uptake after each row); S_end [2, N] the two boxes after the last row and
    replay_mismatches (an int: the (row, member) whose replayed T differs in bits from the stored one) with S_begin only."""
    F: object = None
    F_gas: object = None
    N: object = None
    H: object = None
    S_end: object = None
    replay_mismatches: object = None


def check_consecutive(steps, what):
    """ValueError unless `steps` are consecutive model steps, naming the first gap: the heat integral and the replay take every
    row as one model step after the last, so a gap would give a silently partial result."""
    st = np.asarray(steps, dtype=np.int64)
    gaps = np.nonzero(np.diff(st) != 1)[0]
    if gaps.size:
        k = int(gaps[0])
        raise ValueError(f"steps: {what} needs rows of consecutive model steps; row {k} holds step {int(st[k])}, row {k + 1} step "
                         f"{int(st[k + 1])}: the result would silently cover part of the run")


def forcing_rows(C_rows, steps, params, *, q, F_ext, dt, T_rows=None, fscale=None, X=None, want=("F",), heat0=None, S_begin=None):
    """The forcing of STORED rows — one streaming HIP pass, F bit for bit what the stepping kernel formed at that step.
    C_rows [n_rows, G, N]: fp32 / fp64 concentrations ON THE GPU (engine.C, or row / member slices of it), read in place
    whenever the member stride is 1, copied otherwise.  steps [n_rows]: the model step each row holds, strictly increasing.
    params: the parameter dict of the run (its gases' PI_conc and f, d, and the pool layout).  q [2, N] device rows.  F_ext: the
    shared external forcing [n_steps] (host), or a device drive table [n_steps, 8] in the rows' precision (engine.drive: F_ext
    in column 6), read in place.  dt: the run's step.  T_rows [n_rows, N]: the stored warming, needed for N, H and the replay.
    fscale [G + K, N] device rows and X (an ExternalForcings, a host table [n_steps, K], or engine.fext, the device table
    [n_steps, 4]): the forcing scales of a forcing= run; both None for a plain run.
    want: any of "F", "F_gas", "N", "H".  heat0 [N] fp64 / S_begin [2, N]: the heat uptake and the box temperatures BEFORE the
    first row — the H[-1] and S_end of an earlier call over EARLIER rows: the result is that of one call over all the rows
    (heat0 None: 0).  S_begin asks for THE REPLAY: the thermal step is repeated on the diagnosed F and compared with the stored T;
    replay_mismatches == 0 proves that the rows, the parameters and the forcing belong together.
    "H" and the replay need rows of consecutive model steps: ValueError otherwise, naming the first gap.  TypeError for host
    rows: there is no CPU path.  Runs on the current stream; reads its inputs, allocates its results."""
    import torch

    from . import _capi
    from ._rowargs import call, dev_rows, drive_table, forcing_tables, model_steps, ptr, steps_i32, steps_in_tables, walk_in_place
    from .forcing import ExternalForcings
    from .params import make_model
    want = tuple(want)
    if not want and S_begin is None or any(w not in WANT for w in want):
        raise ValueError(f"want: {want!r}; any of {WANT} (or S_begin= for the replay alone)")
    if not isinstance(C_rows, torch.Tensor) or C_rows.dim() != 3:
        raise ValueError("C_rows: want a tensor [n_rows, G, N]")
    if not C_rows.is_cuda or C_rows.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"C_rows must be fp32 / fp64 rows on a GPU (got {C_rows.dtype} on {C_rows.device}): the forcing rows run "
                        "through the HIP kernel and have no CPU fallback")
    K, G, N = C_rows.shape
    dev, dtp = C_rows.device, C_rows.dtype
    model = make_model(params, dt)
    if int(model.n_gas) != G:
        raise ValueError(f"C_rows hold {G} gases, params {int(model.n_gas)}")
    if N < 1:
        raise ValueError("C_rows: no members")
    st = model_steps(steps, K)
    need_T = "N" in want or "H" in want or S_begin is not None or heat0 is not None
    if need_T and T_rows is None:
        raise ValueError("N, H and the replay need T_rows")
    if "H" in want or heat0 is not None:
        check_consecutive(st, "the heat uptake H")
    if S_begin is not None:
        check_consecutive(st, "the replay")

    # the shared tables: F_ext as a drive table, X padded to the C ABI's four columns
    drive = drive_table(F_ext, (), "F_ext (a drive table)", dtp, dev)
    n_steps = int(drive.shape[0])
    steps_in_tables(st, n_steps)

    def host_table(X):
        fx = X if isinstance(X, ExternalForcings) else ExternalForcings(np.asarray(X, dtype=np.float64).reshape(n_steps, -1))
        if fx.n_steps != n_steps:
            raise ValueError(f"X: table of {fx.n_steps} steps, F_ext of {n_steps}")
        return fx

    n_fext, fext, fscale = forcing_tables(
        fscale, X, (), G, N, n_steps, dtp, dev, x_name="X (a device table)", host_table=host_table,
        together="fscale and X come together: the scale rows and the category table of a forcing= run (a table without "
                 "categories will do)")
    # per-member rows the kernel reads with ONE row stride ld: q as it lies when its columns are contiguous, the scales and
    # the carried state laid out to match
    q, (ld,) = walk_in_place(dev_rows(q, (2, N), "q", dtp, dev), N)
    if fscale is not None and (fscale.stride(0) != ld or (N > 1 and fscale.stride(1) != 1)):
        buf = torch.empty((G + n_fext, ld), dtype=dtp, device=dev)[:, :N]
        buf.copy_(fscale)
        fscale = buf
    x, (c_row, c_gas) = walk_in_place(C_rows, N)
    tr, t_row = None, N
    if need_T:
        tr, (t_row,) = walk_in_place(dev_rows(T_rows, (K, N), "T_rows", dtp, dev), N)
    res = ForcingRows()
    # every output row starts 16-byte aligned: one row length for all of them, N rounded up to 16 bytes of the rows' type
    per16 = 16 // x.element_size()
    ld_out = (N + per16 - 1) // per16 * per16
    out = lambda lead, dtype=dtp: torch.empty(lead + (ld_out,), dtype=dtype, device=dev)[..., :N]      # noqa: E731
    res.F = out((K,)) if "F" in want else None
    res.F_gas = out((K, G)) if "F_gas" in want else None
    res.N = out((K,)) if "N" in want else None
    res.H = out((K,), torch.float64) if "H" in want else None
    H_io = S_io = mism = None
    if "H" in want or heat0 is not None:
        H_io = torch.zeros((ld,), dtype=torch.float64, device=dev)[:N]
        if heat0 is not None:
            H_io.copy_(dev_rows(heat0, (N,), "heat0", torch.float64, dev))
    if S_begin is not None:
        S_io = torch.empty((2, ld), dtype=dtp, device=dev)[:, :N]
        S_io.copy_(dev_rows(S_begin, (2, N), "S_begin", dtp, dev))
        mism = torch.zeros((1,), dtype=torch.int64, device=dev)
    st32 = steps_i32(st, dev)
    call(_capi.load(), _capi, "fiveeq_forcing_rows", dtp, dev, ctypes.byref(model), K, N, ld, ptr(x) if K else None, c_row, c_gas,
         ptr(tr) if K else None, t_row, ptr(st32) if K else None, ptr(drive), n_steps, ptr(q), ptr(fscale), n_fext, ptr(fext),
         ptr(res.F), ptr(res.F_gas), ptr(res.N), ptr(res.H), ld_out, ptr(H_io), ptr(S_io), ptr(mism))
    if S_io is not None:
        res.S_end = S_io
        res.replay_mismatches = int(mism.item())
    return res
